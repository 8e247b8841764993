"""rm_field_ambient without a GPU: the library's own arithmetic (raymarcher_amd/csrc/rm_field_ambient.h, compiled into a stand-alone
program under the address and undefined-behaviour sanitizers) against the NumPy definition (tests/field_ambient_spec.py) in every
word, on the fixture the GPU tests use; the fixture's own conditions; and the pieces of the definition one by one."""
import numpy as np
import pytest

import field_ambient_helpers as M
import field_ambient_spec as A
import field_handle_helpers as H
from raymarcher_amd import abi, hemisphere_directions

f32 = np.float32


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("ambient_cpu")
    return M.build_cpu_program(d), d


def _both(program, points, normals, K, sets, mode, sparse, dense=None, origin=None, step=None, bias=M.BIAS, max_distance=M.MAX_DISTANCE, iso=M.ISO,
          steps=M.MAX_STEPS, bl=None):
    if dense is None:
        dense, origin, step = M.lattice()
    if sparse and bl is None:
        bl = M.block_list()
    table = hemisphere_directions(K, sets)
    want = A.ambient(dense, origin, step, points, normals, table, K, sets, bias, max_distance, iso, steps, mode, None, bl if sparse else None)
    got = M.run_cpu_program(program[0], program[1], dense, origin, step, points, normals, table, K, sets, bias, max_distance, iso, steps, mode, None,
                            bl if sparse else None)
    return got, want


def test_the_fixture_exercises_both_branches():
    """By the NumPy definition alone, at 64 directions, HARD: at least 10 % of all rays hit, at least 10 % miss, and at least 50
    records lie strictly between 0 and 1."""
    dense, origin, step = M.lattice()
    p, n = M.points()
    want = A.ambient(dense, origin, step, p, n, hemisphere_directions(64), 64, 1, M.BIAS, M.MAX_DISTANCE, M.ISO, M.MAX_STEPS, A.HARD)
    assert (want["hits"] >= 0).all()
    fraction = want["hits"].sum() / (64.0 * len(p))
    assert 0.10 <= fraction <= 0.90, fraction
    assert ((want["visibility"] > 0) & (want["visibility"] < 1)).sum() >= 50
    assert (want["visibility"] == 1).sum() >= 10 and (want["hits"] == 64).sum() >= 1


@pytest.mark.parametrize("K, sets, mode, sparse, given", [
    (1, 1, A.SOFT, False, False), (1, 3, A.HARD, True, True), (4, 3, A.HARD, True, False), (4, 1, A.SOFT, False, True),
    (64, 1, A.HARD, False, True), (64, 3, A.SOFT, True, False), (256, 1, A.SOFT, True, True), (256, 3, A.HARD, False, False),
    (16, 2, A.SOFT, True, True), (128, 8, A.HARD, True, False)])
def test_the_header_equals_the_definition_on_the_fixture(program, K, sets, mode, sparse, given):
    p, n = M.points()
    got, want = _both(program, p, n if given else None, K, sets, mode, sparse)
    M.assert_records_equal(got, want, f"K = {K}, {sets} sets, mode {mode}, sparse {sparse}, normals given {given}")
    if not given and sparse:
        assert (want["hits"] == abi.RM_FIELD_UNLISTED).sum() >= 10  # the points off every surface


def test_edge_points(program):
    p, n, labels = M.edge_points()
    code = dict(zip(labels, range(len(labels))))
    for sparse in (False, True):
        for mode in (A.SOFT, A.HARD):
            got, want = _both(program, p, n, 16, 3, mode, sparse)
            M.assert_records_equal(got, want, f"edge points, normals given, sparse {sparse}, mode {mode}")
            for label in ("NaN coordinate", "inf coordinate", "zero normal", "negative zero normal", "NaN normal"):
                r = want[code[label]]
                assert r["hits"] == abi.RM_RAY_INVALID and not A.as_words(want[code[label]:code[label] + 1])[0, :7].any(), label
            for label in ("n = +z", "n = -z", "n.z = -0", "n.z = +0", "non-unit normal", "tiny normal", "valid 0", "valid 3"):
                assert want[code[label]]["hits"] >= 0, label
            assert want[code["n = +z"]]["visibility"] > 0 and (want[code["n.z = -0"]]["normal"] == n[code["n.z = -0"], 0:3]).all()
            got, want = _both(program, p, None, 16, 3, mode, sparse)
            M.assert_records_equal(got, want, f"edge points, the lattice's normals, sparse {sparse}, mode {mode}")
            assert want[code["outside the box"]]["hits"] == abi.RM_FIELD_OUTSIDE and want[code["just outside the box"]]["hits"] == abi.RM_FIELD_OUTSIDE
            assert want[code["unlisted block"]]["hits"] == (abi.RM_FIELD_UNLISTED if sparse else 0)
            assert want[code["NaN coordinate"]]["hits"] == abi.RM_RAY_INVALID


def test_small_budgets_and_the_clamp(program):
    p, n = M.points()
    for steps, max_distance in ((0, M.MAX_DISTANCE), (1, M.MAX_DISTANCE), (M.MAX_STEPS, 0.0)):
        for sparse in (False, True):
            got, want = _both(program, p[:150], n[:150], 4, 3, A.SOFT, sparse, steps=steps, max_distance=max_distance)
            M.assert_records_equal(got, want, f"{steps} samples, maxDistance {max_distance}, sparse {sparse}")
            if steps == 0:  # nothing is sampled: every ray is a miss with the factor 1
                assert (want["hits"] == 0).all() and (want["visibility"] == 1).all()
    # negative_lattice: nothing hits, t falls below 0 and the penumbra factor with it — the clamp h.t > 0 ? h.t : 0 decides
    dense, origin, step = H.negative_lattice(M.BLOCKS)
    bl = H.campaign_list(M.BLOCKS, "checker")
    for sparse in (False, True):
        got, want = _both(program, p[:150], n[:150], 16, 1, A.SOFT, sparse, dense, origin, step, iso=H.NEGATIVE_ISO, steps=24, bl=bl)
        M.assert_records_equal(got, want, f"the negative lattice, sparse {sparse}")
        assert (want["hits"] == 0).all() and (want["visibility"] >= 0).all() and (want["visibility"] == 0).sum() >= 10


def test_the_frame_is_orthonormal_and_has_no_singular_direction():
    rng = np.random.default_rng(5)
    n = rng.normal(size=(2000, 3))
    n = (n / np.linalg.norm(n, axis=1)[:, None]).astype(f32)
    n[:6] = [[0, 0, 1], [0, 0, -1], [1, 0, 0.0], [1, 0, -0.0], [0, -1, 0], [0.6, 0.8, -0.0]]
    T, B = A.frame(n)
    assert np.isfinite(T).all() and np.isfinite(B).all()
    m = np.stack([T, B, n], axis=1).astype(np.float64)
    gram = m @ m.transpose(0, 2, 1)
    assert np.abs(gram - np.eye(3)).max() < 1e-6
    assert (np.linalg.det(m) > 0.999).all()  # right-handed: T × B = n
    assert (T[1] == [1, 0, 0]).all() and (B[1] == [0, -1, 0]).all()  # n.z = −1: s = −1, a = 0.5


def test_the_tree_is_the_pairwise_one():
    x = np.array([[1.0, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24]], f32)[:, :, None]
    assert A.tree(x)[0, 0] == f32(1.0) + f32(2.0 ** -23)  # (1 + ε) + (ε + ε) with ε half an ulp: the left pair loses it, the right pair keeps both
    assert ((f32(1.0) + f32(2.0 ** -24)) + f32(2.0 ** -24)) + f32(2.0 ** -24) == f32(1.0)  # the sequential sum differs
    rng = np.random.default_rng(9)
    leaves = rng.uniform(0, 1, (7, 256, 4)).astype(f32)
    s = leaves.copy()
    for level in range(8):  # the xor butterfly: every lane adds its partner, and every lane ends with the tree's sum
        partner = np.arange(256) ^ (1 << level)
        s = s + s[:, partner]
    assert (s.view(np.uint32) == A.tree(leaves).view(np.uint32)[:, None, :]).all()
