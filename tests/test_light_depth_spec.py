"""The probe depth moments without a GPU: the library's own arithmetic (raymarcher_amd/csrc/rm_light_depth.h and the visible step of
rm_light_grid.h, compiled into a stand-alone program under the address and undefined-behaviour sanitizers and run as a program)
against the NumPy definitions (tests/light_depth_spec.py) in every word on the GPU tests' fixtures; rm_probe_depth_weights against
its float64 definition; and properties of the definitions themselves: every texel's weights sum to 1, far depth records give
rm_light_grid_irradiance's records in every word, and a wall at distance 1 hides a point at 2 and shows one at 0.5."""
import numpy as np
import pytest

import light_depth_helpers as M
import light_depth_spec as D
import light_grid_helpers as MG
import light_grid_spec as G
import light_probes_spec as L
from raymarcher_amd import probe_depth_weights, sphere_directions

f32 = np.float32


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("light_depth_cpu")
    return M.build_cpu_program(d), d


# ---------------------------------------------------------------- the host program against the definitions
def seeded_distances(n, K, dist, seed):
    """What rm_trace_rays could store: hits between 0 and dist, misses at dist exactly, a zero, a denormal; float32 (n·K)."""
    rng = np.random.default_rng(8700 + seed)
    t = rng.uniform(0, dist, n * K).astype(f32)
    kind = rng.integers(0, 8, n * K)
    t[kind == 0] = f32(dist)
    t[kind == 1] = f32(0.0)
    t[kind == 2] = f32(1e-41)
    return t


@pytest.mark.parametrize("K", M.DIRS + (16, 1024))
def test_the_bakes_header_equals_the_definition(program, K):
    """Every shape of the GPU test, and 16 and 1024 directions: a subtree below a pass, and sixteen passes with four pending levels."""
    for n in M.PROBES if K <= 128 else (3,):
        positions = M.bake_positions((0.0, 0.5, -1.0), 2.0, n, K)
        for sets in M.SETS:
            for label, table in M.tables(K, sets):
                for kind, weights in (("seeded", M.seeded_weights(K, sets, n)), ("own", probe_depth_weights(table, sets))):
                    t = seeded_distances(n, K, 3.0, K + n + sets)
                    want = D.moments(positions, table, weights, K, sets, t)
                    got = M.run_cpu_bake(program[0], program[1], positions, table, weights, K, sets, t)
                    D.assert_depth_equal(got, want, f"K = {K}, {n} probes, {sets} sets, {label}, {kind} weights")
                    bad = ~L.valid_positions(positions)
                    assert bad.sum() == (1 if n >= 3 else 0) and not D.as_words(want[bad]).any(), "a non-finite probe stores zeros"
                    assert np.isfinite(want["moments"]).all()
    if K >= 64:  # with fewer rows the last variant's rows are all invalid: every leaf is a zero
        assert len(np.unique(D.as_words(want[~bad])[:, 0])) == (~bad).sum(), "every probe should have other moments"


@pytest.mark.parametrize("bias", M.BIASES)
@pytest.mark.parametrize("facing", [False, True])
@pytest.mark.parametrize("name", list(MG.GRIDS))
def test_the_lookups_header_equals_the_definition(program, name, facing, bias):
    dims, origin, step, bad, _ = MG.GRIDS[name]
    rec, depth = MG.records(name), M.depth_records(name)
    seen = []
    for n in MG.COUNTS:
        pts, nrm = MG.points(name, n)
        want = D.grid_light_visible(rec, depth, dims, origin, step, pts, nrm, facing, bias)
        got = M.run_cpu_look(program[0], program[1], rec, depth, dims, origin, step, pts, nrm, facing, bias)
        G.assert_records_equal(got, want, f"{name}, {n} points, facing {facing}, bias {bias}")
        ok = G.valid_points(pts, nrm)
        assert (want["probes"][~ok] == G.INVALID).all() and np.isfinite(want["e"]).all() and np.isfinite(want["weight"]).all()
        plain = G.grid_light(rec, dims, origin, step, pts, nrm, facing)
        seen.append((G.as_words(want) != G.as_words(plain)).any(axis=1)[ok].mean())
    assert seen[-1] > 0.3, "the depth records should change most of the fixture's points"


def test_the_depth_fixture_holds_what_it_promises():
    for name in MG.GRIDS:
        bad = MG.GRIDS[name][3]
        d = M.depth_records(name)["moments"]
        assert np.isnan(d[bad]).all() and np.isfinite(np.delete(d, bad, axis=0)).all()
        m, m2 = np.delete(d[:, :, 0], bad, axis=0), np.delete(d[:, :, 1], bad, axis=0)
        words = np.delete(d, bad, axis=0).view(np.uint32)
        assert (((words & 0x7F800000) == 0) & ((words & 0x007FFFFF) != 0)).any(), "denormals"
        assert (m < 0).any() and (m > 0).any() and (m2 < 0).any() and (words == 0x80000000).any() and (words == 0).any()
        assert (m2 == m * m).any() and (m2 < m * m).any() and (m2 > m * m).any(), "no variance, less than none, some"


# ---------------------------------------------------------------- rm_probe_depth_weights
@pytest.mark.parametrize("K, sets", [(1, 1), (2, 1), (2, 3), (64, 1), (64, 3), (256, 1)])
def test_depth_weights_equal_the_float64_definition_rounded_once(K, sets):
    for label, table in M.tables(K, sets):
        for sharpness in (0.0, 50.0, 1e4) if K <= 64 else (50.0,):
            got = probe_depth_weights(table, sets, sharpness)
            want = D.depth_weights(table, K, sets, sharpness)
            assert got.dtype == f32 and got.shape == (K * sets, 64)
            assert (got.view(np.uint32) == want.view(np.uint32)).all(), (K, sets, label, sharpness, np.abs(got - want).max())
            assert not got[~L.valid_rows(table)].view(np.uint32).any(), "an invalid row has +0 on every texel"


@pytest.mark.parametrize("sharpness", [0.0, 50.0, 1e4])
@pytest.mark.parametrize("K", [1, 2, 64])
def test_every_texels_weights_sum_to_one(K, sharpness):
    """K roundings of at most half an ulp of a value <= 1 each: |Σ − 1| <= K·2⁻²⁴ (the sum itself in float64).  The nearest-row
    fallback gives exactly 1."""
    for sets in (1, 3):
        w = probe_depth_weights(sphere_directions(K, sets), sets, sharpness).reshape(sets, K, 64)
        total = w.astype(np.float64).sum(axis=1)
        print(f"K = {K}, sharpness {sharpness}, {sets} sets: largest |Σ − 1| = {np.abs(total - 1).max():.3e}, bound {K * 2.0 ** -24:.3e}")
        assert (np.abs(total - 1) <= K * 2.0 ** -24).all() and (w >= 0).all()
        fallback = ((w == 1).sum(axis=1) == 1) & ((w != 0).sum(axis=1) == 1)
        if sharpness == 1e4 and K <= 2:
            assert fallback.any(), "at this sharpness some texel is out of every lobe's reach: the nearest row takes it whole"
        if K == 1:
            assert (w == 1).all()


def test_the_fallback_takes_the_nearest_valid_row_and_the_lowest_of_a_tie():
    """Three rows that point down, the same direction in other lengths, and an invalid row that would point up.  The 24 texels of
    the upper half and the 16 on the equator (1 − |u| − |v| is exactly 0 there) are out of every lobe's reach."""
    table = np.zeros((4, 16), f32)
    table[0, 0:3], table[1, 0:3], table[2, 0:3], table[3, 0:3] = (0, 0, -2), (0, 0, -1), (0, 0, -1), (np.nan, 0, 1)
    w = probe_depth_weights(table, 1, 50.0)
    up = D.texel_centres()[:, 2] >= 0
    assert (w[3] == 0).all() and not w[3].view(np.uint32).any(), "the invalid row takes no part, though it is nearest"
    assert up.sum() == 40 and (w[0, up] == 1).all() and (w[1:, up] == 0).all(), "out of reach: rows 0, 1, 2 tie, the lowest k has it"
    assert (np.abs(w[:, ~up].astype(np.float64).sum(axis=0) - 1) <= 3 * 2.0 ** -24).all() and (w[0:3, ~up] > 0).all()
    assert (w.view(np.uint32) == D.depth_weights(table, 4, 1, 50.0).view(np.uint32)).all()


# ---------------------------------------------------------------- two properties of the lookup's definition
@pytest.mark.parametrize("facing", [False, True])
@pytest.mark.parametrize("name", list(MG.GRIDS))
def test_far_depth_gives_the_plain_lookups_records_in_every_word(program, name, facing):
    dims, origin, step, _, _ = MG.GRIDS[name]
    rec, depth = MG.records(name), M.depth_records(name, far=True)
    pts, nrm = (np.array(a) for a in MG.points(name, 257))
    pts[(np.abs(pts[:, 0:3]) > 1e29).any(axis=1)] = pts[0]  # the two points at ±3e38 are farther than any finite mean
    for bias in M.BIASES:
        want = G.grid_light(rec, dims, origin, step, pts, nrm, facing)
        G.assert_records_equal(D.grid_light_visible(rec, depth, dims, origin, step, pts, nrm, facing, bias), want, f"{name}: the definition")
        got = M.run_cpu_look(program[0], program[1], rec, depth, dims, origin, step, pts, nrm, facing, bias)
        G.assert_records_equal(got, want, f"{name}, facing {facing}, bias {bias}: the header's code")


def test_a_wall_at_distance_one_hides_what_is_behind_it():
    """m = 1, m2 = 1 on every texel: no variance, so a point beyond the wall gets the floor and a point before it 1."""
    depth = np.ones((1, 64, 2), f32)
    rng = np.random.default_rng(3)
    u = rng.normal(size=(200, 3))
    u = u / np.linalg.norm(u, axis=1, keepdims=True)
    u[0:6] = np.concatenate([np.eye(3), -np.eye(3)])  # the axes: the map's centre, its corners and edge midpoints
    probe = np.array([[0.25, -1.0, 2.0]], f32)
    for r, want in ((2.0, D.FLOOR), (0.5, f32(1)), (0.0, f32(1))):
        q = (probe + f32(r) * u).astype(f32)
        vis = D.visibility(q, np.repeat(probe, len(q), axis=0), np.repeat(depth, len(q), axis=0))
        assert (vis == want).all(), (r, np.unique(vis))
    # and through the whole lookup: one cell whose probes all have that wall; a point 2 away from every corner has weight floor·Σt
    rec = np.zeros(8, G.PROBE)
    rec["sh"][:, 0, :] = f32(1)
    walls = np.zeros(8, D.DEPTH)
    walls["moments"] = f32(1)
    dims, origin, step = (2, 2, 2), (0.0, 0.0, 0.0), (4.0, 4.0, 4.0)
    p, n = np.array([[2.0, 2.0, 2.0, 0.0]], f32), np.array([[0.0, 0.0, 1.0, 0.0]], f32)  # sqrt(12) from every corner
    hidden = D.grid_light_visible(rec, walls, dims, origin, step, p, n, False, 0.0)
    plain = G.grid_light(rec, dims, origin, step, p, n, False)
    assert plain["weight"][0] == 1 and hidden["weight"][0] == f32(8) * (f32(0.125) * D.FLOOR) and hidden["probes"][0] == 8
    near = np.array([[0.25, 0.25, 0.25, 0.0]], f32)  # within 1 of corner 0 only
    got = D.grid_light_visible(rec, walls, dims, origin, step, near, n, False, 0.0)
    t0 = (f32(1) - f32(0.0625)) * (f32(1) - f32(0.0625)) * (f32(1) - f32(0.0625))
    assert got["probes"][0] == 8 and abs(float(got["weight"][0]) - float(t0)) < 1e-6, "corner 0 in full, the others at the floor"
