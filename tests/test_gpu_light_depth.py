"""rm_light_probes_depth, rm_light_grid_irradiance_visible and their Python layer on the GPU, no tolerance on a record.
The bake: every word equals trace_rays(mode="closest", normals=False)'s t pushed through the NumPy leaves and tree
(tests/light_depth_spec.py), on the table walk and on both Mandelbulb classes, for 1, 3 and 65 probes (one with a non-finite
position), 1, 2, 64 and 128 directions, one and three sets, tables with invalid rows, seeded weights and probe_depth_weights' own,
into poisoned, guarded buffers; probes asked alone; the memory; a frame before and after.  The lookup: every word equals the NumPy
definition on light_grid_helpers' grids and points with seeded depth records; far depth gives rm_light_grid_irradiance's records;
an invalid probe's depth words are not read.  End to end: a wall between a lit and an unlit side, and a grid that spans both."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import helpers as h
import light_depth_helpers as M
import light_depth_spec as D
import light_grid_helpers as MG
import light_grid_spec as G
import light_probes_spec as L
import shade_helpers as S
import trace_helpers as T
from raymarcher_amd import LightGrid, abi, lib, probe_depth_weights, sphere_directions

pytestmark = pytest.mark.gpu
f32 = np.float32
CASES = ("generic_nosec", "plain_bulb_nosec", "moved_bulb_nosec")  # the three march classes: table walk, plain and general Mandelbulb


def case_distance(name):
    scene, _, _ = S.case(name)
    centre, radius = T.cull_bounds(scene[1], scene[2], scene[5])
    return centre, radius, 1.5 * radius  # from probes up to 1.6 radii out: rays that end on the surface and rays that end at maxDistance


def depth_guarded(renderer, scene, s, res, positions, table, weights, K, sets, dist):
    """Renderer.light_probes_depth into a poisoned, guarded buffer, checked → DEPTH records."""
    out, check = h.guarded((len(positions), 64, 2), device=renderer.device)
    rec = renderer.light_probes_depth(S.tables_of(scene, res), s, np.array(positions), directions=K, sets=sets, max_distance=dist,
                                      table=np.array(table), weights=np.array(weights), out=out)
    assert lib().rm_debug_last_path() == abi.RM_PATH_LIGHT_PROBES_DEPTH == 22 and lib().rm_debug_last_split() == 0
    check()
    assert rec.data_ptr() == out.data_ptr()
    return np.frombuffer(out.cpu().numpy().tobytes(), D.DEPTH, len(positions))


def composed(renderer, scene, s, res, positions, table, weights, K, sets, dist, first=0):
    """The same records through the shipped entry: rm_trace_rays NO_NORMAL on the n·K rays, then the NumPy leaves and tree."""
    rays = L.rays(positions, table, K, sets, dist, first)
    t = renderer.trace_rays(S.tables_of(scene, res), s, rays, normals=False)[1].cpu().numpy()
    return D.moments(positions, table, weights, K, sets, t, first), t


# ---------------------------------------------------------------- the bake
@pytest.mark.parametrize("name", CASES)
def test_the_bake_equals_trace_rays_through_the_tree_in_every_word(renderer, name):
    scene, s, res = S.case(name)
    centre, radius, dist = case_distance(name)
    saw_hit = saw_miss = False
    for K in M.DIRS:
        for n in M.PROBES:
            positions = M.bake_positions(centre, radius, n, 10 * K + sorted(S.CASES).index(name))
            for sets in M.SETS:
                for label, table in M.tables(K, sets):
                    for kind, weights in (("seeded", M.seeded_weights(K, sets, n)), ("own", probe_depth_weights(table, sets))):
                        what = f"{name}, K = {K}, {n} probes, {sets} sets, {label}, {kind} weights"
                        want, t = composed(renderer, scene, s, res, positions, table, weights, K, sets, dist)
                        got = depth_guarded(renderer, scene, s, res, positions, table, weights, K, sets, dist)
                        D.assert_depth_equal(got, want, what)
                        bad = ~L.valid_positions(positions)
                        assert bad.sum() == (1 if n >= 3 else 0) and not D.as_words(got[bad]).any(), what
                        saw_hit, saw_miss = saw_hit or ((t > 0) & (t < f32(dist))).any(), saw_miss or (t == f32(dist)).any()
    assert saw_hit and saw_miss, "the case should hold rays that end on the surface and rays that end at maxDistance"


@pytest.mark.parametrize("name, K, n, sets", [("generic_nosec", 2, 65, 3), ("plain_bulb_nosec", 128, 3, 3), ("moved_bulb_nosec", 64, 3, 1)])
def test_probes_asked_alone_give_the_same_words(renderer, name, K, n, sets):
    scene, s, res = S.case(name)
    centre, radius, dist = case_distance(name)
    positions = M.bake_positions(centre, radius, n, 77)
    table, weights = sphere_directions(K, sets), M.seeded_weights(K, sets, 5)
    together = depth_guarded(renderer, scene, s, res, positions, table, weights, K, sets, dist)
    for i in range(n):
        rows = slice((i % sets) * K, (i % sets + 1) * K)  # alone the probe is probe 0 and takes set 0: hand it its own set
        alone = depth_guarded(renderer, scene, s, res, positions[i:i + 1], table[rows], weights[rows], K, 1, dist)
        D.assert_depth_equal(alone, together[i:i + 1], f"{name}: probe {i} alone")


def test_the_built_weights_defaults_memory_and_a_frame_around(renderer):
    name, K, n, W, H = "generic_nosec", 64, 16, 64, 36
    scene, s, res = S.case(name, W, H)
    t = S.tables_of(scene, res)
    before = renderer.render(t, s, W, H).cpu().numpy()
    path, split = lib().rm_debug_last_path(), lib().rm_debug_last_split()
    centre, radius, dist = case_distance(name)
    pos = np.array(M.bake_positions(centre, radius, n, 3))
    dev = torch.from_numpy(pos).to(renderer.device)
    rec = renderer.light_probes_depth(t, s, dev, directions=K, max_distance=dist)  # builds and keeps the table and its weights
    assert tuple(rec.shape) == (n, 64, 2) and rec.dtype == torch.float32
    table = sphere_directions(K, 1)
    want, _ = composed(renderer, scene, s, res, pos, table, probe_depth_weights(table, 1, 50.0), K, 1, dist)
    D.assert_depth_equal(np.frombuffer(rec.cpu().numpy().tobytes(), D.DEPTH, n), want, "the built table and weights")
    # (n, 3) positions and max_distance=None: the scene camera's initialFar
    rec3 = renderer.light_probes_depth(t, s, pos[:, 0:3], directions=K)
    want, _ = composed(renderer, scene, s, res, pos, table, probe_depth_weights(table, 1, 50.0), K, 1, scene[0].initialFar)
    D.assert_depth_equal(np.frombuffer(rec3.cpu().numpy().tobytes(), D.DEPTH, n), want, "max_distance=None")
    del rec, rec3
    # the call allocates its result and nothing else: n·512 B
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated(renderer.device)
    rec = renderer.light_probes_depth(t, s, dev, directions=K, max_distance=dist)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(renderer.device) - held == n * 512 == rec.numel() * 4
    assert lib().rm_debug_last_path() == abi.RM_PATH_LIGHT_PROBES_DEPTH
    assert tuple(renderer.light_probes_depth(t, s, np.zeros((0, 4), f32), directions=K).shape) == (0, 64, 2)
    with pytest.raises(ValueError):
        renderer.light_probes_depth(t, s, dev, directions=K, weights=np.zeros((K, 63), f32))
    with pytest.raises(ValueError):
        renderer.light_probes_depth(t, s, dev, directions=K, out=torch.empty((n, 128), device=renderer.device))
    after = renderer.render(t, s, W, H).cpu().numpy()
    assert (lib().rm_debug_last_path(), lib().rm_debug_last_split()) == (path, split)
    S.assert_bits(after, before, "a single frame around rm_light_probes_depth")


def test_the_bake_refuses_host_pointers_and_touches_nothing(renderer):
    scene, s, res = S.case("generic_nosec")
    _, objs, no, _, _, g = scene
    n, K = 8, 16
    pos = torch.zeros((n, 4), device=renderer.device)
    table = torch.from_numpy(sphere_directions(K, 1)).to(renderer.device)
    weights = torch.zeros((K, 64), device=renderer.device)
    out, check = h.guarded((n, 64, 2), device=renderer.device)
    host =np.zeros(4096 + 4, f32)
    hp = (host.ctypes.data + 15) & ~15

    def call(p, d, w, o):
        return lib().rm_light_probes_depth(C.c_void_p(p), n, C.c_void_p(d), C.c_void_p(w), K, 1, 2.0, objs, no, C.byref(g), C.byref(s),
                                           C.c_void_p(o), None)

    good = (pos.data_ptr(), table.data_ptr(), weights.data_ptr(), out.data_ptr())
    for at, word in enumerate(("d_positions", "d_dirs", "d_weights", "d_out")):
        args = list(good)
        args[at] = hp
        assert call(*args) == abi.RM_ERR_INVALID_ARGUMENT and word in lib().rm_last_error().decode(), word
    torch.cuda.synchronize()
    assert bool((out.view(torch.int32) == h._i32(h.FLOAT_POISON)).all()), "a refused call wrote into d_out"
    assert call(*good) == abi.RM_OK
    torch.cuda.synchronize()
    check()


# ---------------------------------------------------------------- the lookup
def grid_of(renderer, name, depth):
    dims, origin, step, _, _ = MG.GRIDS[name]
    probes = torch.from_numpy(np.array(MG.records(name)).view(f32).reshape(-1, 40)).to(renderer.device)
    grid = LightGrid(renderer, probes, origin, step, dims)
    return grid.set_depth(None if depth is None else np.array(depth["moments"]))


def look_guarded(grid, pts, nrm, facing, **kw):
    out, check = h.guarded((len(pts), 8), device=grid.probes.device)
    e, weight, probes = grid.irradiance_visible(np.array(pts), np.array(nrm), facing=facing, out=out, **kw)
    check()
    assert e.data_ptr() == out.data_ptr()
    return np.frombuffer(out.cpu().numpy().tobytes(), G.GRIDLIGHT, len(pts))


@functools.lru_cache(maxsize=None)
def look_spec(name, n, facing, bias):
    dims, origin, step, _, _ = MG.GRIDS[name]
    pts, nrm = MG.points(name, n)
    want = D.grid_light_visible(MG.records(name), M.depth_records(name), dims, origin, step, pts, nrm, facing, bias)
    want.setflags(write=False)
    return want


@pytest.mark.parametrize("facing", [False, True])
@pytest.mark.parametrize("name", list(MG.GRIDS))
def test_the_lookup_equals_the_definition_in_every_word(renderer, name, facing):
    grid = grid_of(renderer, name, M.depth_records(name))
    path = lib().rm_debug_last_path()
    for bias in M.BIASES:
        for n in MG.COUNTS:
            pts, nrm = MG.points(name, n)
            got = look_guarded(grid, pts, nrm, facing, normal_bias=bias)
            G.assert_records_equal(got, look_spec(name, n, facing, bias), f"{name}, {n} points, facing {facing}, bias {bias}")
    assert lib().rm_debug_last_path() == path, "not a render launch"
    # the plain entry on the same grid is untouched by the depth records, and irradiance follows the grid
    pts, nrm = MG.points(name, 257)
    dims, origin, step, _, _ = MG.GRIDS[name]
    plain = G.grid_light(MG.records(name), dims, origin, step, pts, nrm, facing)
    G.assert_records_equal(look_guarded(grid, pts, nrm, facing, visible=False), plain, f"{name}: visible=False")
    grid.set_depth(grid.depth, normal_bias=0.1)
    e, weight, probes = grid.irradiance(np.array(pts), np.array(nrm), facing=facing)
    got = np.zeros(len(pts), G.GRIDLIGHT)
    got["e"], got["weight"], got["probes"] = e.cpu().numpy(), weight.cpu().numpy(), probes.cpu().numpy()
    G.assert_records_equal(got, look_spec(name, 257, facing, 0.1), f"{name}: irradiance follows the grid, facing {facing}")


@pytest.mark.parametrize("name", list(MG.GRIDS))
def test_far_depth_and_an_invalid_probes_depth_words(renderer, name):
    dims, origin, step, bad, _ = MG.GRIDS[name]
    pts, nrm = (np.array(a) for a in MG.points(name, 257))
    far_pts = pts.copy()
    far_pts[(np.abs(pts[:, 0:3]) > 1e29).any(axis=1)] = pts[0]  # the two points at ±3e38 are farther than any finite mean
    without = grid_of(renderer, name, None)
    far = grid_of(renderer, name, M.depth_records(name, far=True))
    for facing in (False, True):
        e, weight, probes = without.irradiance(far_pts, nrm, facing=facing)
        want = np.zeros(len(pts), G.GRIDLIGHT)
        want["e"], want["weight"], want["probes"] = e.cpu().numpy(), weight.cpu().numpy(), probes.cpu().numpy()
        for bias in M.BIASES:
            G.assert_records_equal(look_guarded(far, far_pts, nrm, facing, normal_bias=bias), want, f"{name}: far depth, facing {facing}, bias {bias}")
    # the invalid probe's depth words: NaN in the fixture, then finite, then infinite — nothing changes
    base = look_guarded(grid_of(renderer, name, M.depth_records(name)), pts, nrm, True, normal_bias=0.1)
    for value in (0.5, np.inf):
        other = np.array(M.depth_records(name))
        other["moments"][bad] = f32(value)
        G.assert_records_equal(look_guarded(grid_of(renderer, name, other), pts, nrm, True, normal_bias=0.1), base, f"{name}: {value} in the invalid probe")
    with pytest.raises(ValueError):
        without.irradiance_visible(pts, nrm, visible=True)
    with pytest.raises(ValueError):
        without.set_depth(np.zeros((3, 64, 2), f32))


# ---------------------------------------------------------------- end to end: a wall between a lit and an unlit side
def wall_scene():
    """A thin cube as a wall in the plane x = 0 on a floor whose top is y = −1, lit by one directional light that comes from +x:
    the side x > 0 is lit, the side x < 0 lies in the wall's shadow.  No ambient term, a dark background."""
    wall = h.make_object(abi.RM_CUBE, model=h.translate(0, 1, 0) @ h.scale(0.1, 6, 8), scale_factor=0.1)
    floor = h.make_object(abi.RM_CUBE, model=h.translate(0, -1.5, 0) @ h.scale(8, 1, 8), scale_factor=1.0)
    objs, no = h.table([wall, floor])
    lights = (abi.RmLight * 1)(h.make_light(abi.RM_LIGHT_DIRECTIONAL, (1, 1, 1), (-1.0, -0.5, 0.0)))
    cam = h.make_camera((3, 1, 6), (-3, -1, -6), (0, 1, 0), 45.0, 16, 16)
    return (cam, objs, no, lights, 1, h.make_globals()), abi.default_settings(features=abi.RM_FEAT_DARK_BACKGROUND)


def test_a_wall_keeps_the_lit_sides_light_off_its_unlit_face(renderer):
    scene, s = wall_scene()
    t = S.tables_of(scene)
    dims, bounds = (6, 4, 6), ((-2.5, -0.5, -2.5), (2.5, 2.5, 2.5))  # step 1: probes half a step from the wall on either side
    grid = renderer.light_grid_visible(t, s, dims, bounds=bounds, directions=256)
    assert grid.depth is not None and tuple(grid.depth.shape) == (144, 64, 2) and (grid.probes[:, 36].view(torch.int32) >= 0).all()
    plain = renderer.light_grid(t, s, dims, bounds=bounds, directions=256)
    assert plain.depth is None and torch.equal(plain.probes.view(torch.int32), grid.probes.view(torch.int32)), "the same SH records"
    # the unlit face of the wall, x = −0.05, normal −x: between the probes at x = −0.5 and the lit ones at x = +0.5
    yz = np.array([(y, z) for y in (-0.25, 0.2, 0.75, 1.3, 1.9) for z in (-1.7, -0.6, 0.15, 0.9, 1.45)], f32)
    face = np.zeros((len(yz), 4), f32)
    face[:, 0], face[:, 1:3] = -0.05, yz
    normal = np.tile(np.array([-1.0, 0.0, 0.0, 0.0], f32), (len(yz), 1))
    for facing in (False, True):
        leaky = plain.irradiance(face, normal, facing=facing)[0].cpu().numpy()[:, 0:3].astype(np.float64)
        tight = grid.irradiance(face, normal, facing=facing)[0].cpu().numpy()[:, 0:3].astype(np.float64)
        print(f"unlit face, facing {facing}: e.rgb with / without visibility, per point: {np.round((tight / leaky).mean(axis=1), 4).tolist()}")
        assert (leaky > 0).all(), "without visibility the lit side's probes light the unlit face"
        assert (tight < leaky).all(), "with visibility the unlit face gets strictly less"
    # the lit side, two steps from the wall: floor points right below a probe.  Three of the four corners with weight have the
    # trilinear weight +0, the fourth is 0.25 above q and at least 0.5 from all geometry, so its mean distances are at least
    # 0.5·Σw and it sees q: vis = 1 and the records are the same words.
    lit = np.array([(1.5, -1.0, z, 0.0) for z in (-1.5, -0.5, 0.5, 1.5)] + [(2.5, -1.0, 0.5, 0.0)], f32)
    up = np.tile(np.array([0.0, 1.0, 0.0, 0.0], f32), (len(lit), 1))
    a, b = plain.irradiance(lit, up), grid.irradiance(lit, up)
    assert (a[0].cpu().numpy()[:, 0:3] > 0).all(), "the lit floor is lit"
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), "a point that its probe sees: nothing changes"
    # generic lit-side points with EIGHT corners of non-zero weight: surfaces of something that moves through the lit room, in the
    # cell x 1.5 … 2.5, y 0.5 … 1.5, z −0.5 … 0.5.  Every corner probe is at least 1.45 from the wall and 1.5 from the floor, every ray
    # of it is at least 1.44 long (a hit's t lies within the march's surface distance of the surface), the weights of a texel are
    # not negative and sum to 1 within 256·2⁻²⁴, and a bilinear blend of such means is one: m >= 1.43.  p is within 0.15 of the
    # cell's centre per axis, at most sqrt(3)·0.65 = 1.126 from a corner, and q = p + 0.25·n at most 1.376: r < m for every corner,
    # vis = 1 eight times, the same words.
    rng = np.random.default_rng(97)
    air = np.zeros((24, 4), f32)
    air[:, 0:3] = np.array([2.0, 1.0, 0.0]) + rng.uniform(-0.15, 0.15, (24, 3))
    dirs = rng.normal(size=(24, 3))
    turned = np.zeros((24, 4), f32)
    turned[:, 0:3] = dirs / np.linalg.norm(dirs, axis=1, keepdims=True)
    q = air[:, 0:3].astype(np.float64) + 0.25 * turned[:, 0:3]
    corners = np.array([[1.5 + (c & 1), 0.5 + ((c >> 1) & 1), -0.5 + ((c >> 2) & 1)] for c in range(8)])
    assert np.linalg.norm(q[:, None, :] - corners[None, :, :], axis=2).max() < 1.38, "the fixture: q nearer to every corner than any surface is"
    for facing in (False, True):
        a, b = plain.irradiance(air, turned, facing=facing), grid.irradiance(air, turned, facing=facing)
        assert (a[2].cpu().numpy() == 8).all(), "eight corners take part"
        for x, y in zip(a, b):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f"eight probes that all see the point, facing {facing}: nothing changes"
    # generic points ON the lit floor, two steps from the wall.  Whether each of their corners sees them is not argued here (a probe
    # half a step above the floor has the floor in most of its lobes), so no equality is asserted.  What holds by construction:
    # 0 < vis <= 1, so no corner's weight grows and, rounding being monotone, neither does their sum; and e is a blend of the same
    # eight E_c with weights that are not negative, so per channel it stays between the least and the largest E_c — which
    # irradiance gives exactly at the probes' own positions with facing off (weight 1 on one corner) — but for the rounding of
    # eight products, seven sums and one division, 32·2⁻²⁴ of the largest |E_c| at the most.
    ground = np.zeros((16, 4), f32)
    ground[:, 0], ground[:, 1], ground[:, 2] = rng.uniform(1.6, 2.4, 16), -1.0, rng.uniform(-1.4, 1.4, 16)
    up = np.tile(np.array([0.0, 1.0, 0.0, 0.0], f32), (16, 1))
    cell = np.floor(ground[:, [0, 2]].astype(np.float64) + 2.5)
    at = np.zeros((16, 8, 4), f32)
    for c in range(8):
        at[:, c, 0], at[:, c, 1], at[:, c, 2] = cell[:, 0] + (c & 1) - 2.5, -0.5 + ((c >> 1) & 1), cell[:, 1] + ((c >> 2) & 1) - 2.5
    E = plain.irradiance(at.reshape(-1, 4), np.repeat(up, 8, axis=0), facing=False)[0].cpu().numpy().reshape(16, 8, 4).astype(np.float64)
    slack = 32 * 2.0 ** -24 * np.abs(E).max(axis=1)
    for facing in (False, True):
        a, b = plain.irradiance(ground, up, facing=facing), grid.irradiance(ground, up, facing=facing)
        ea, eb = a[0].cpu().numpy().astype(np.float64), b[0].cpu().numpy().astype(np.float64)
        print(f"lit floor, facing {facing}: e.rgb with / without visibility, per point: {np.round((eb[:, 0:3] / ea[:, 0:3]).mean(axis=1), 4).tolist()}; "
              f"weight with / without: {np.round(b[1].cpu().numpy() / a[1].cpu().numpy(), 4).tolist()}")
        assert (b[1].cpu().numpy() <= a[1].cpu().numpy()).all() and (b[1].cpu().numpy() > 0).all(), "no corner's weight grows"
        for e in (ea, eb):
            assert (e >= E.min(axis=1) - slack).all() and (e <= E.max(axis=1) + slack).all(), "a blend of the corners' light stays between them"
    # render_indirect follows the grid
    W = H = 16
    with_wall = renderer.render_indirect(t, s, W, H, grid)
    without = renderer.render_indirect(t, s, W, H, plain)
    assert with_wall.shape == without.shape == (1, H, W, 4) and not torch.equal(with_wall, without)
