"""rm_field_ambient on the GPU against the NumPy definition (tests/field_ambient_spec.py) in every word — and against the composition
a caller writes without it: the definition's rays through the shipped rm_field_trace, then the NumPy tree —, every record between
guard rows, on the dense and the block handle of field_ambient_helpers' fixture; the edge points, the small budgets, two plain
facts, the query refusals, which need a live handle, and the Python layer.  No comparison here has a tolerance."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import field_ambient_helpers as M
import field_ambient_spec as A
import field_handle_helpers as H
import field_handle_spec as S
import helpers as h
from raymarcher_amd import abi, hemisphere_directions, lib
from test_gpu_field import ptr, up
from test_gpu_field_handle import Field

pytestmark = pytest.mark.gpu
f32 = np.float32
INVALID = abi.RM_ERR_INVALID_ARGUMENT
COUNTS = (1, 17, 197, 600)  # the last wave ragged at segment and at wave granularity, and the last workgroup at wave granularity


def ambient(f, points, normals, table, K, sets, bias, max_distance, iso, steps, mode):
    """The C entry point on handle f into a poisoned output between guard rows → AMBIENT records; every word inside written and no
    guard word touched."""
    r = f.r
    pts, nrm, tab = up(r, points, f32), up(r, normals, f32), up(r, table, f32)
    g = h.Guarded((len(pts), 8), torch.float32, h.FLOAT_POISON, r.device)
    path = lib().rm_debug_last_path()
    st = lib().rm_field_ambient(f.handle, ptr(pts), ptr(nrm), len(pts), ptr(tab), K, sets, float(bias), float(max_distance), float(iso), steps, mode,
                                ptr(g.payload), r._stream())
    assert st == abi.RM_OK, lib().rm_last_error().decode()
    g.check()
    assert lib().rm_debug_last_path() == path, "not a render launch"
    return g.payload.cpu().numpy().view(A.AMBIENT).reshape(-1)


def fixture_field(renderer, sparse):
    dense, origin, step = M.lattice()
    return Field(renderer, dense, None, origin, step, M.block_list() if sparse else None)


@functools.lru_cache(maxsize=None)
def fixture_want(K, sets, mode, sparse, given):
    """The definition on all 600 points: record i depends on i and not on numPoints, so a call of fewer points has the first of them."""
    dense, origin, step = M.lattice()
    p, n = M.points()
    want = A.ambient(dense, origin, step, p, n if given else None, hemisphere_directions(K, sets), K, sets, M.BIAS, M.MAX_DISTANCE, M.ISO,
                     M.MAX_STEPS, mode, None, M.block_list() if sparse else None)
    want.setflags(write=False)
    return want


def test_the_fixture_exercises_both_branches():
    want = fixture_want(64, 1, A.HARD, False, True)
    fraction = want["hits"].sum() / (64.0 * len(want))
    assert (want["hits"] >= 0).all() and 0.10 <= fraction <= 0.90, fraction
    assert ((want["visibility"] > 0) & (want["visibility"] < 1)).sum() >= 50


@pytest.mark.parametrize("given", (True, False), ids=("normals", "gradient"))
@pytest.mark.parametrize("sparse", (False, True), ids=("dense", "blocks"))
@pytest.mark.parametrize("mode", (A.SOFT, A.HARD), ids=("soft", "hard"))
@pytest.mark.parametrize("sets", (1, 3))
@pytest.mark.parametrize("K", (1, 4, 64, 256))
def test_bit_equality_with_the_definition_and_with_the_composition(renderer, K, sets, mode, sparse, given):
    dense, origin, step = M.lattice()
    p, n = M.points()
    table = hemisphere_directions(K, sets)
    want = fixture_want(K, sets, mode, sparse, given)
    with fixture_field(renderer, sparse) as f:
        for count in COUNTS:
            got = ambient(f, p[:count], n[:count] if given else None, table, K, sets, M.BIAS, M.MAX_DISTANCE, M.ISO, M.MAX_STEPS, mode)
            M.assert_records_equal(got, want[:count], f"{count} points")
        # the composition through the shipped entry: the definition's rays, field.trace on the device, the NumPy tree
        count = 197
        march = lambda rows: f.trace(rows, M.ISO, M.MAX_STEPS, S.OCCLUSION if mode == A.SOFT else S.NO_NORMAL)  # noqa: E731
        composed = A.ambient(dense, origin, step, p[:count], n[:count] if given else None, table, K, sets, M.BIAS, M.MAX_DISTANCE, M.ISO,
                             M.MAX_STEPS, mode, None, M.block_list() if sparse else None, march=march)
        M.assert_records_equal(composed, want[:count], "rm_field_trace and the NumPy tree")


def test_edge_points_among_valid_ones(renderer):
    p, n, labels = M.edge_points()
    at = dict(zip(labels, range(len(labels))))
    dense, origin, step = M.lattice()
    table = hemisphere_directions(16, 3)
    for sparse in (False, True):
        bl = M.block_list() if sparse else None
        with fixture_field(renderer, sparse) as f:
            for mode in (A.SOFT, A.HARD):
                for normals in (n, None):
                    want = A.ambient(dense, origin, step, p, normals, table, 16, 3, M.BIAS, M.MAX_DISTANCE, M.ISO, M.MAX_STEPS, mode, None, bl)
                    got = ambient(f, p, normals, table, 16, 3, M.BIAS, M.MAX_DISTANCE, M.ISO, M.MAX_STEPS, mode)
                    M.assert_records_equal(got, want, f"sparse {sparse}, mode {mode}, normals {'given' if normals is not None else 'NULL'}")
                    assert got[at["NaN coordinate"]]["hits"] == abi.RM_RAY_INVALID and got[at["inf coordinate"]]["hits"] == abi.RM_RAY_INVALID
                    if normals is not None:
                        for label in ("zero normal", "negative zero normal", "NaN normal"):
                            assert got[at[label]]["hits"] == abi.RM_RAY_INVALID and not A.as_words(got[at[label]:at[label] + 1])[0, :7].any(), label
                        for label in ("n = +z", "n = -z", "n.z = -0", "n.z = +0", "non-unit normal", "valid 0", "valid 3"):
                            assert got[at[label]]["hits"] >= 0 and (got[at[label]]["normal"] == n[at[label], 0:3]).all(), label
                    else:
                        assert got[at["outside the box"]]["hits"] == abi.RM_FIELD_OUTSIDE
                        assert got[at["unlisted block"]]["hits"] == (abi.RM_FIELD_UNLISTED if sparse else 0)


def test_small_budgets_and_the_clamp(renderer):
    dense, origin, step = M.lattice()
    p, n = M.points()
    p, n = p[:197], n[:197]
    table = hemisphere_directions(4, 3)
    for sparse in (False, True):
        bl = M.block_list() if sparse else None
        with fixture_field(renderer, sparse) as f:
            for steps, max_distance in ((0, M.MAX_DISTANCE), (1, M.MAX_DISTANCE), (M.MAX_STEPS, 0.0)):
                for mode in (A.SOFT, A.HARD):
                    want = A.ambient(dense, origin, step, p, n, table, 4, 3, M.BIAS, max_distance, M.ISO, steps, mode, None, bl)
                    got = ambient(f, p, n, table, 4, 3, M.BIAS, max_distance, M.ISO, steps, mode)
                    M.assert_records_equal(got, want, f"{steps} samples, maxDistance {max_distance}, sparse {sparse}, mode {mode}")
                    if steps == 0:
                        assert (got["hits"] == 0).all() and (got["visibility"] == 1).all()
    # the negative lattice with a negative iso: nothing hits, the penumbra factor falls below 0 and the clamp decides
    dense, origin, step = H.negative_lattice(M.BLOCKS)
    table = hemisphere_directions(16, 1)
    for bl in (None, H.campaign_list(M.BLOCKS, "checker")):
        with Field(renderer, dense, None, origin, step, bl) as f:
            want = A.ambient(dense, origin, step, p, n, table, 16, 1, M.BIAS, M.MAX_DISTANCE, H.NEGATIVE_ISO, 24, A.SOFT, None, bl)
            got = ambient(f, p, n, table, 16, 1, M.BIAS, M.MAX_DISTANCE, H.NEGATIVE_ISO, 24, A.SOFT)
            M.assert_records_equal(got, want, f"the negative lattice, sparse {bl is not None}")
            assert (got["hits"] == 0).all() and (got["visibility"] >= 0).all() and (got["visibility"] == 0).sum() >= 10


def test_no_point_writes_nothing(renderer):
    with fixture_field(renderer, False) as f:
        g = h.Guarded((4, 8), torch.float32, h.FLOAT_POISON, renderer.device)
        table = up(renderer, hemisphere_directions(16), f32)
        st = lib().rm_field_ambient(f.handle, ptr(g.payload), None, 0, ptr(table), 16, 1, 0.05, 1.0, 0.001, 64, 0, ptr(g.payload), None)
        assert st == abi.RM_OK
        assert lib().rm_field_ambient(f.handle, None, None, 0, None, 16, 1, 0.05, 1.0, 0.001, 64, 1, None, None) == abi.RM_OK
        torch.cuda.synchronize()
        assert bool(g._unwritten(g.buf).all()), "numPoints = 0 writes nothing"


def test_two_plain_facts(renderer):
    # 1. a flat lattice, value = z: nothing above the plane is hit, so HARD visibility is the tree sum of the weights in every bit
    # and bent points along +z
    _first, origin, step = H.campaign_lattice(M.BLOCKS)
    z = origin[2] + np.arange(8 * M.BLOCKS[2] + 1, dtype=f32) * step[2]
    flat = np.ascontiguousarray(np.broadcast_to(z[:, None, None], (len(z), 8 * M.BLOCKS[1] + 1, 8 * M.BLOCKS[0] + 1)), f32)
    rng = np.random.default_rng(3)
    p = np.zeros((97, 4), f32)
    p[:, 0:2], p[:, 2] = rng.uniform(-0.5, 0.5, (97, 2)), 0.0
    n = np.zeros((97, 4), f32)
    n[:, 2] = 1
    for K in (4, 64, 256):
        table = hemisphere_directions(K, 1)
        table[:, 3] = (rng.uniform(0.5, 1.5, K) / K).astype(f32)  # weights whose sum depends on the order
        # at n = +z the frame is T = (1, 0, −0), B = (0, 1, −0): d is the table's entry in every bit, and a leaf is w·(x, y, z, 1)
        sums = A.tree((table[:, 3:4] * np.concatenate([table[:, 0:3], np.ones((K, 1), f32)], axis=1))[None])[0]
        with Field(renderer, flat, None, origin, step) as f:
            got = ambient(f, p, n, table, K, 1, M.BIAS, M.MAX_DISTANCE, M.ISO, M.MAX_STEPS, A.HARD)
        assert (got["hits"] == 0).all()
        assert (got["visibility"].view(np.uint32) == sums[3].view(np.uint32)).all(), K
        assert (got["bent"].view(np.uint32) == sums[0:3].view(np.uint32)).all() and (got["bent"][:, 2] > 0).all(), K
    # and with every direction along the normal bent is parallel to +z: exactly (0, 0, 1)
    up_only = np.tile(np.array([0, 0, 1, 0.25], f32), (4, 1))
    with Field(renderer, flat, None, origin, step) as f:
        got = ambient(f, p, n, up_only, 4, 1, M.BIAS, M.MAX_DISTANCE, M.ISO, M.MAX_STEPS, A.HARD)
    assert (got["bent"][:, 0:2] == 0).all() and (got["bent"][:, 2] == 1).all() and (got["visibility"] == 1).all()
    # 2. the floor under the second sphere's overhang sees less than the floor far from both spheres
    pts = np.stack([M.OVERHANG_POINT, M.OPEN_POINT])
    nrm = np.array([[0, 0, 1, 0], [0, 0, 1, 0]], f32)
    with fixture_field(renderer, True) as f:
        got = ambient(f, pts, nrm, hemisphere_directions(64), 64, 1, M.BIAS, M.MAX_DISTANCE, M.ISO, M.MAX_STEPS, A.HARD)
    assert got["visibility"][0] < got["visibility"][1] and got["hits"][0] > got["hits"][1]


def test_query_refusals_in_order(renderer):
    nan, inf = float("nan"), float("inf")
    host = np.zeros(4096, f32)
    hp = C.c_void_p(host.ctypes.data + (-host.ctypes.data) % 16)
    buf = torch.zeros((64, 8), dtype=torch.float32, device=renderer.device)
    table = up(renderer, hemisphere_directions(16, 4), f32)
    dev, tab = C.c_void_p(buf.data_ptr()), C.c_void_p(table.data_ptr())
    fake, odd = C.c_void_p(0x1000), C.c_void_p(0x1008)

    def refused(status, text):
        return status == INVALID and text in lib().rm_last_error().decode()

    for sparse in (False, True):
        with fixture_field(renderer, sparse) as f:
            def call(n=5, p=fake, nrm=fake, d=fake, K=16, sets=4, bias=0.05, dist=1.0, iso=0.001, steps=64, mode=0, o=fake):
                return lib().rm_field_ambient(f.handle, p, nrm, n, d, K, sets, bias, dist, iso, steps, mode, o, None)

            for n in (-1, -2 ** 31):
                assert refused(call(n=n, K=3), "negative numPoints")
            for K in (0, -1, 3, 48, 257, 512, 2 ** 31 - 1):
                assert refused(call(K=K, sets=0), "numDirs must be a power of two")
            for K, sets in ((16, 0), (16, -1), (16, 65), (256, 5), (1, 1025), (2, 2 ** 30)):
                assert refused(call(K=K, sets=sets, bias=nan), "numSets")
            for v in (nan, inf, -inf):
                assert refused(call(bias=v, steps=-1), "bias must be finite")
                assert refused(call(dist=v, steps=-1), "maxDistance must be finite and not negative")
                assert refused(call(iso=v, steps=-1), "iso must be finite")
            assert refused(call(dist=-1e-30, steps=-1), "maxDistance") and refused(call(bias=nan, dist=-1.0), "bias")
            for steps in (-1, 65537, 2 ** 31 - 1):
                assert refused(call(steps=steps, mode=4), "maxSteps must be 0 … RM_MAX_FIELD_STEPS")
            for mode in (2, 3, 4, 0x80000000):
                assert refused(call(mode=mode, n=0), "mode bits other than RM_AMBIENT_HARD")
            for mode in (0, 1):
                assert call(n=0, mode=mode) == abi.RM_OK and call(n=0, mode=mode, p=None, nrm=None, d=None, o=None, steps=65536, dist=0.0) == abi.RM_OK
            for k in ("p", "d", "o"):
                assert refused(call(**{k: None}), "null d_points, d_dirs or d_out"), k
                assert refused(call(**{k: None, "nrm": odd}), "null"), k  # null comes before misaligned
            for k in ("p", "nrm", "d", "o"):
                assert refused(call(**{k: odd}), "misaligned"), k
            assert refused(call(p=hp, nrm=None, d=tab, o=dev), "d_points is not device-accessible")
            assert refused(call(p=dev, nrm=hp, d=tab, o=dev), "d_normals is not device-accessible")
            assert refused(call(p=dev, nrm=None, d=hp, o=dev), "d_dirs is not device-accessible")
            assert refused(call(p=dev, nrm=dev, d=tab, o=hp), "d_out is not device-accessible")
            assert refused(call(p=hp, nrm=odd, d=tab, o=dev), "misaligned")  # misaligned comes before the device-memory check
            if torch.cuda.device_count() > 1:
                try:
                    assert lib().rm_set_device(1) == abi.RM_OK
                    assert refused(call(p=dev, nrm=None, d=tab, o=dev), "another device")
                finally:
                    assert lib().rm_set_device(0) == abi.RM_OK
                    torch.cuda.set_device(renderer.device)
            assert call(p=dev, nrm=None, d=tab, o=dev) == abi.RM_OK and call(p=dev, nrm=dev, d=tab, o=dev, mode=1) == abi.RM_OK  # the handle still works
            torch.cuda.synchronize()
        assert refused(lib().rm_field_ambient(None, dev, None, 5, tab, 16, 4, 0.05, 1.0, 0.001, 64, 0, dev, None), "null or stale RmField handle")


def test_the_python_layer(renderer):
    dense, origin, step = M.lattice()
    p, n = M.points()
    bl = M.block_list()
    import sdf_blocks_spec as B
    grid = up(renderer, B.pack_blocks(dense, bl, f32(np.nan)), f32)
    diagonal = float(np.sqrt(sum((float(step[a]) * 8 * M.BLOCKS[a]) ** 2 for a in range(3))))

    def rows(parts):
        return torch.cat([q.view(torch.float32).reshape(len(q), -1) for q in parts], dim=1).cpu().numpy().view(A.AMBIENT).reshape(-1)

    with renderer.lattice_field_blocks(grid, up(renderer, bl, np.int32), M.BLOCKS, origin, step) as field:
        # the defaults: 16 directions, one set, bias twice the step, the box's diagonal, SOFT, 64 samples
        want = A.ambient(dense, origin, step, p, n, hemisphere_directions(16), 16, 1, M.BIAS, f32(diagonal), 0.001, 64, A.SOFT, None, bl)
        bent, visibility, normal, hits = field.ambient(p, n)
        assert hits.dtype == torch.int32 and visibility.shape == (len(p),) and bent.shape == (len(p), 3)
        M.assert_records_equal(rows((bent, visibility, normal, hits)), want, "the defaults")
        assert list(field._tables) == [(16, 1)]
        field.ambient(p[:5], n[:5])
        assert list(field._tables) == [(16, 1)], "the table is built once per (dirs, sets)"
        # a ready table, sets, HARD, the lattice's own normals, the caller's tensor
        table = hemisphere_directions(64, 3)
        out = torch.empty((len(p), 8), dtype=torch.float32, device=renderer.device)
        got = field.ambient(p[:, 0:3], None, directions=torch.from_numpy(table), sets=3, max_distance=M.MAX_DISTANCE, bias=M.BIAS, soft=False, out=out)
        assert got[0].data_ptr() == out.data_ptr()
        want = A.ambient(dense, origin, step, p, None, table, 64, 3, M.BIAS, M.MAX_DISTANCE, 0.001, 64, A.HARD, None, bl)
        M.assert_records_equal(out.cpu().numpy().view(A.AMBIENT).reshape(-1), want, "a ready table")
        got = field.ambient(p, None, directions=64, sets=3, max_distance=M.MAX_DISTANCE, bias=M.BIAS, soft=False)
        M.assert_records_equal(rows(got), want, "the same table, built")
        assert field.ambient(np.zeros((0, 3), f32))[1].shape == (0,)
        with pytest.raises(ValueError):
            field.ambient(p, n[:5])
        with pytest.raises(ValueError):
            field.ambient(p, n, directions=torch.zeros((7, 4)), sets=2)
    with pytest.raises(ValueError):
        field.ambient(p, n)  # closed


def test_bake_mesh_pruned_ambient(renderer):
    import sdf_helpers as V
    objs, no, g, s = V.scene("sphere_cube")
    lights = (abi.RmLight * 1)(h.make_light(abi.RM_LIGHT_DIRECTIONAL, (1, 1, 1), (-0.3, -1, -0.5)))
    for i in range(no):
        for k in range(3):
            objs[i].cAmbient[k], objs[i].cDiffuse[k] = 0.3, 0.8
    t = h.tables_of((h.make_camera((0, 0, 5), (0, 0, -1), (0, 1, 0), 40.0, 8, 8), objs, no, lights, 1, g))
    plain = renderer.bake_mesh_pruned(t, s, 20, 0.001)
    shaded = renderer.bake_mesh_pruned_ambient(t, s, 20, 16, 0.001)
    same = renderer.bake_mesh_pruned_ambient(t, s, 20, None, 0.001)
    assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(plain, same))
    assert int(plain[5].max()) > 0
    for a, b in zip(plain[:5], shaded[:5]):
        assert (a is None and b is None) or torch.equal(a, b)
    assert shaded[5].dtype == torch.uint8 and shaded[5].shape == plain[5].shape
    assert bool((shaded[5] <= plain[5]).all())
    dist, obj, bl, blocks, origin, step = renderer.scene_field_pruned(t, s, 20, 0.001)
    with renderer.lattice_field_blocks(dist, bl, blocks, origin, step, obj) as field:
        visibility = field.ambient(plain[0], plain[3], directions=16)[1]
        want = torch.clamp(torch.round(plain[5].to(torch.float32) * visibility.clamp(0.0, 1.0)[:, None]), 0.0, 255.0).to(torch.uint8)
        assert torch.equal(shaded[5], want)
        print("mean visibility", float(visibility.mean()), "vertices darkened", int((shaded[5] < plain[5]).any(dim=1).sum()), "of", len(visibility))
        assert bool(((visibility >= 0) & (visibility <= 1)).all()) and float(visibility.mean()) > 0.05
