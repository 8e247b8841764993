"""rm_shade_rays_indirect / rm_light_probes_indirect and the Python layer over them on the GPU.  Every word of shade_rays_indirect
against the composition through shipped entries — shade_rays, trace_rays with tMax = far, LightGrid.irradiance / irradiance_visible
and the NumPy term (tests/light_bounce_spec.py) — on every case of shade_helpers.CASES, which covers the twelve kernel classes, on
seeded grids laid over the case's bounds, with and without depth records, facing off and on, bias 0 and 0.1, for 1, 64, 65 and 257
rays.  The composition's dif is kd·cDiffuse of the table; its palette factor comes from a second shade_rays call on a copy of the
tables with no lights, ka = 1, cAmbient = 1 and AO, reflection and refraction off, whose colour is 8c on the bulb, c on the sponge
and 1 elsewhere.  Hits of textured objects are held to arbiter_numpy's getDiffuse with test_resource_arbiter's margin and tolerance.
Then the bake against light_probes_spec's tree over shade_rays_indirect's colours, a grid of zeros, rays asked alone, the path, the
memory, a frame around the calls, the refusals that need the device, render_lit, and two bounces in a room behind a wall."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import arbiter_numpy as an
import helpers as h
import light_bounce_helpers as M
import light_bounce_spec as B
import light_depth_helpers as MD
import light_grid_helpers as MG
import light_grid_spec as G
import light_probes_helpers as MP
import light_probes_spec as L
import shade_helpers as S
import trace_helpers as T
from raymarcher_amd import LightGrid, RaymarcherError, abi, camera_rays, lib, mesh_bounds, sphere_directions
from test_gpu_light_depth import wall_scene
from test_resource_arbiter import TEX_B

pytestmark = pytest.mark.gpu

f32 = np.float32
FAR = 100.0
NAMES = list(S.CASES)
COUNTS = (1, 64, 65, 257)
GRID_NAMES = sorted(MG.GRIDS)  # (5, 4, 3), (2, 2, 2), (3, 2, 4) probes
# (with depth records, facing, bias): every combination the lookup has
CONFIGS = ((False, False, 0.0), (False, True, 0.0), (True, False, 0.0), (True, True, 0.0), (True, False, 0.1), (True, True, 0.1))


# ---------------------------------------------------------------- the fixtures
def bounds_of(name):
    scene, _, res = S.case(name)
    try:
        lo, hi = mesh_bounds(S.tables_of(scene, res))
    except ValueError:
        lo, hi = np.array([-1.5, -1.5, -1.5], f32), np.array([1.5, 1.5, 1.5], f32)
    # shrunk by another factor on every axis: the step of a grid over it is anisotropic whatever its dims, and hits lie inside
    # the box, on its border and outside it
    mid, half = (lo.astype(np.float64) + hi) / 2, (hi.astype(np.float64) - lo) / 2 * np.array([1.0, 0.85, 0.7])
    return mid - half, mid + half


def grid_of(renderer, name, grid_name, with_depth):
    """light_grid_helpers' seeded records — both signs, one invalid probe of NaN coefficients — laid over the case's bounds: the
    first probe at lo, the last at hi, so the step is anisotropic; light_depth_helpers' seeded depth records with them."""
    dims = MG.GRIDS[grid_name][0]
    lo, hi = bounds_of(name)
    origin, step = lo.astype(f32), ((hi - lo) / (np.array(dims) - 1)).astype(f32)
    assert len(set(step.tolist())) == 3, "an anisotropic step"
    probes = torch.from_numpy(np.array(MG.records(grid_name)).view(f32).reshape(-1, 40)).to(renderer.device)
    grid = LightGrid(renderer, probes, origin, step, dims)
    return grid.set_depth(np.array(MD.depth_records(grid_name)["moments"]) if with_depth else None)


@functools.lru_cache(maxsize=None)
def rays_of(name, n):
    """n seeded rays from around the case's cull ball towards and past it → read-only float32 (n, 8); tMax holds junk that
    shade_rays does not read; from three rays on one is invalid (a zero direction), neither first nor last, from 64 on a NaN
    origin too; one direction of length 2."""
    scene, _, _ = S.case(name)
    centre, radius = T.cull_bounds(scene[1], scene[2], scene[5])
    rng = np.random.default_rng(6100 + 17 * n + NAMES.index(name))
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    origin = np.asarray(centre) + u * (rng.uniform(1.3, 2.5, (n, 1)) * radius)
    target = np.asarray(centre) + rng.normal(size=(n, 3)) * (0.55 * radius)
    d = target - origin
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = T.make_rays(origin, d, rng.uniform(-1, 1, n))
    if n >= 3:
        rays[n // 2, 4:7] = (0.0, -0.0, 0.0)
    if n >= 64:
        rays[n // 3, 1] = f32(np.nan)
        rays[5, 4:7] *= f32(2.0)
    rays.setflags(write=False)
    return rays


def composed(renderer, name, rays, grid, facing, bias, strength, far=FAR):
    """light_bounce_helpers.composed_indirect on a case of shade_helpers.CASES."""
    scene, s, res = S.case(name)
    return M.composed_indirect(renderer, scene, s, res, rays, grid, facing, bias, strength, far)


def shade_guarded(renderer, name, rays, grid, facing, bias, strength, far=FAR):
    scene, s, res = S.case(name)
    out, check = h.guarded((len(rays), 4), device=renderer.device)
    got = renderer.shade_rays_indirect(S.tables_of(scene, res), s, np.array(rays), grid, far=far, strength=strength, facing=facing,
                                       normal_bias=bias, out=out)
    assert lib().rm_debug_last_path() == abi.RM_PATH_SHADE_RAYS_INDIRECT == 23 and lib().rm_debug_last_split() == 0
    check()
    assert got.data_ptr() == out.data_ptr()
    return got.cpu().numpy()


def assert_equals_composition(renderer, name, rays, grid, facing, bias, strength, what):
    """Every word, but on hits of textured objects: there the composition's dif is arbiter_numpy's getDiffuse in binary64, which
    the binary32 texture fetch matches to 1e-3 away from a uv jump (test_resource_arbiter's TEX_B margin and tolerance).  The term
    is linear in dif, so the bound is 1e-3 · ec · k · palette, plus four roundings of the result."""
    got = shade_guarded(renderer, name, rays, grid, facing, bias, strength)
    want, on, textured, q = composed(renderer, name, rays, grid, facing, bias, strength)
    exact = ~textured
    h.assert_bit_equal(got[exact], want[exact], what)
    h.assert_bit_equal(got[~on], q["colour"][~on], what + ": a ray without a term keeps shade_rays' words")
    h.assert_bit_equal(got[:, 3], q["colour"][:, 3], what + ": alpha")
    if textured.any():
        scene, s, res = S.case(name)
        rgb, margin, _ = an.get_diffuse(q["o"], res["textures"], q["k"][textured], q["point"][textured].astype(np.float64), float(scene[5].kd))
        ec = np.maximum(np.nan_to_num(q["e"][textured][:, 0:3].astype(np.float64), nan=0.0), 0.0)
        kk = float(B.scale_of(strength))
        ind = rgb * ec * kk
        lit = q["colour"][textured][:, 0:3].astype(np.float64) + ind
        bound = 1e-3 * ec * abs(kk) + 4 * 2.0 ** -24 * (np.abs(q["colour"][textured][:, 0:3]) + np.abs(ind))
        away = margin >= TEX_B
        err = np.abs(got[textured][:, 0:3] - lit)
        print(f"{what}: {textured.sum()} textured hits, {away.sum()} away from a uv jump, largest error / bound {np.max(err[away] / np.maximum(bound[away], 1e-30), initial=0):.3f}")
        assert (err[away] <= bound[away]).all(), (what, err[away].max())
    return got, want, on, q


# ---------------------------------------------------------------- the kernel equals the composition in every word
@pytest.mark.parametrize("name", NAMES)
def test_kernel_equals_the_composition_in_every_word(renderer, name):
    scene, s, _ = S.case(name)
    assert S.class_of(scene, s) == S.CASES[name][0], "the case is not of the class it is listed under"
    at = NAMES.index(name)
    hits = misses = lit = 0
    for ci, n in enumerate(COUNTS):
        with_depth, facing, bias = CONFIGS[(at + ci) % len(CONFIGS)]
        grid_name = GRID_NAMES[(at + ci) % len(GRID_NAMES)]
        grid = grid_of(renderer, name, grid_name, with_depth)
        strength = (1.0, 0.37)[ci % 2]
        what = f"{name}, {n} rays, grid {grid_name}, depth {with_depth}, facing {facing}, bias {bias}, strength {strength}"
        got, want, on, q = assert_equals_composition(renderer, name, rays_of(name, n), grid, facing, bias, strength, what)
        hits, misses, lit = hits + (q["obj"] >= 0).sum(), misses + (q["obj"] == -1).sum(), lit + (h.bits(got) != h.bits(q["colour"])).any(axis=1).sum()
        if n >= 3:
            bad = q["obj"] == abi.RM_RAY_INVALID
            assert bad.sum() == (2 if n >= 64 else 1) and not bad[0] and not bad[-1] and not h.bits(got[bad]).any(), "an invalid ray stores zeros"
    if scene[2] > 0:
        assert hits > 0 and misses > 0, f"{name}: hits ({hits}) and misses ({misses}) should both occur"
        assert lit > 0, f"{name}: the grid should light some hits ({lit})"
    else:
        assert hits == 0 and lit == 0


def test_every_lookup_configuration_on_one_case(renderer):
    """The rotation above gives every case some configurations; here one table-walk case and one bulb case take all of them on
    every grid, at 257 rays."""
    for name in ("generic_sec", "plain_bulb_nosec"):
        for grid_name in GRID_NAMES:
            for with_depth, facing, bias in CONFIGS:
                grid = grid_of(renderer, name, grid_name, with_depth)
                assert_equals_composition(renderer, name, rays_of(name, 257), grid, facing, bias, 1.0,
                                          f"{name}, grid {grid_name}, depth {with_depth}, facing {facing}, bias {bias}")


def test_a_grid_of_no_valid_probe_changes_no_word(renderer):
    """probes = 0 on every hit: shade_rays' words, a −0 included."""
    for name in ("generic_nosec", "menger_nosec", "moved_bulb_sec", "tex_nosec"):
        scene, s, res = S.case(name)
        dims = (2, 2, 2)
        lo, hi = bounds_of(name)
        probes = np.array(MG.records("one_cell", all_invalid=True)).view(f32).reshape(-1, 40)
        grid = LightGrid(renderer, probes, lo.astype(f32), (hi - lo).astype(f32), dims)
        rays = rays_of(name, 257)
        got = shade_guarded(renderer, name, rays, grid, True, 0.0, 1.0)
        h.assert_bit_equal(got, renderer.shade_rays(S.tables_of(scene, res), s, np.array(rays), far=FAR).cpu().numpy(), name)


def test_rays_asked_alone_give_the_same_words(renderer):
    for name, with_depth in (("generic_sec", True), ("plain_bulb_sec", False), ("moved_bulb_nosec", True)):
        grid = grid_of(renderer, name, "strides", with_depth)
        rays = np.array(rays_of(name, 65))
        together = shade_guarded(renderer, name, rays, grid, True, 0.1, 1.0)
        for i in (0, 7, 31, 32, 63, 64):
            h.assert_bit_equal(shade_guarded(renderer, name, rays[i:i + 1], grid, True, 0.1, 1.0), together[i:i + 1], f"{name}: ray {i} alone")


# ---------------------------------------------------------------- the bake
BAKE_SHAPES = tuple(sh for sh in MP.SHAPES if sh[0] in (2, 64, 128))  # one segment per wave at 64, several at 2, two passes at 128
assert len(BAKE_SHAPES) == 3 and all(n <= 65 for _, n in BAKE_SHAPES)


def bake_guarded(renderer, name, positions, table, K, sets, grid, facing, bias, strength, far=FAR):
    scene, s, res = S.case(name)
    out, check = h.guarded((len(positions), 40), device=renderer.device)
    sh, hits = renderer.light_probes_indirect(S.tables_of(scene, res), s, np.array(positions), grid, directions=K, sets=sets, far=far,
                                              table=np.array(table), strength=strength, facing=facing, normal_bias=bias, out=out)
    assert lib().rm_debug_last_path() == abi.RM_PATH_LIGHT_PROBES_INDIRECT == 24 and lib().rm_debug_last_split() == 0
    check()
    assert sh.data_ptr() == out.data_ptr() and tuple(sh.shape) == (len(positions), 9, 4) and hits.dtype == torch.int32
    return np.frombuffer(out.cpu().numpy().tobytes(), L.PROBE, len(positions))


@pytest.mark.parametrize("K, n", BAKE_SHAPES)
@pytest.mark.parametrize("name", ["generic_sec", "plain_bulb_nosec", "moved_bulb_sec", "tex_nosec"])
def test_the_bake_equals_the_tree_over_shade_rays_indirect_in_every_word(renderer, name, K, n):
    scene, s, res = S.case(name)
    t = S.tables_of(scene, res)
    positions = MP.positions(name, K, n)
    at = NAMES.index(name) + K
    for sets in MP.SETS:
        with_depth, facing, bias = CONFIGS[(at + sets) % len(CONFIGS)]
        grid = grid_of(renderer, name, GRID_NAMES[(at + sets) % 3], with_depth)
        shade = lambda rays: renderer.shade_rays_indirect(t, s, rays, grid, far=FAR, strength=0.8, facing=facing, normal_bias=bias).cpu().numpy()  # noqa: E731
        trace = lambda rays: renderer.trace_rays(t, s, rays, normals=False)[3].cpu().numpy()  # noqa: E731
        for label, table in MP.tables(K, sets):
            want = L.probes(scene, s, res, positions, table, K, sets, FAR, shade=shade, trace=trace)
            got = bake_guarded(renderer, name, positions, table, K, sets, grid, facing, bias, 0.8)
            L.assert_records_equal(got, want, f"{name}, K = {K}, {len(positions)} probes, {sets} sets, {label}, depth {with_depth}, facing {facing}")
            plain = L.probes(scene, s, res, positions, table, K, sets, FAR, shade=lambda r: renderer.shade_rays(t, s, r, far=FAR).cpu().numpy(), trace=trace)
            assert (got["hits"] == plain["hits"]).all(), "the hit flag is rm_light_probes'"
    bad = ~L.valid_positions(positions)
    assert (got["hits"][bad] == abi.RM_RAY_INVALID).all() and not L.as_words(got[bad])[:, :36].any()
    if K >= 64:
        assert (L.as_words(got) != L.as_words(plain)).any(), "the grid should change the records"


def test_a_grid_of_zeros_gives_light_probes_records_as_numbers(renderer):
    """e = 0 everywhere: every ray's colour is shade_rays' + 0, the same number (a −0 may become +0)."""
    for name, K, n in (("generic_nosec", 64, 5), ("plain_bulb_sec", 128, 3), ("menger_sec", 2, 33)):
        scene, s, res = S.case(name)
        t = S.tables_of(scene, res)
        lo, hi = bounds_of(name)
        rec = np.zeros(8, G.PROBE)
        rec["hits"] = 3
        grid = LightGrid(renderer, np.array(rec).view(f32).reshape(-1, 40), lo.astype(f32), (hi - lo).astype(f32), (2, 2, 2))
        positions, table = MP.positions(name, K, n), sphere_directions(K, 1)
        got = bake_guarded(renderer, name, positions, table, K, 1, grid, True, 0.0, 1.0)
        sh, hits = renderer.light_probes(t, s, np.array(positions), directions=K, far=FAR, table=table)
        assert (got["sh"] == sh.cpu().numpy()).all() and (got["hits"] == hits.cpu().numpy()).all(), name


def test_probes_asked_alone_give_the_same_words(renderer):
    name, K, sets = "moved_bulb_sec", 128, 3
    grid = grid_of(renderer, name, "anisotropic", True)
    positions, table = np.array(MP.positions(name, K, 3)), sphere_directions(K, sets)
    together = bake_guarded(renderer, name, positions, table, K, sets, grid, True, 0.1, 1.0)
    for i in range(len(positions)):
        own = table[(i % sets) * K:(i % sets + 1) * K]
        L.assert_records_equal(bake_guarded(renderer, name, positions[i:i + 1], own, K, 1, grid, True, 0.1, 1.0), together[i:i + 1], f"probe {i} alone")


# ---------------------------------------------------------------- memory, a frame around the calls, refusals that need the device
def test_memory_and_a_frame_around_the_calls(renderer):
    W, H = 64, 36
    scene, s, res = S.case("generic_nosec", W, H)
    t = S.tables_of(scene, res)
    before = renderer.render(t, s, W, H).cpu().numpy()
    path, split = lib().rm_debug_last_path(), lib().rm_debug_last_split()
    name = "generic_sec"
    sc, ss, rr = S.case(name)
    tt = S.tables_of(sc, rr)
    grid = grid_of(renderer, name, "strides", True)
    rays = torch.from_numpy(np.array(rays_of(name, 257))).to(renderer.device)
    pos = torch.from_numpy(np.array(MP.positions(name, 64, 5))).to(renderer.device)
    renderer.shade_rays_indirect(tt, ss, rays, grid, far=FAR)
    renderer.light_probes_indirect(tt, ss, pos, grid, directions=64, far=FAR)  # builds and keeps the table
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(renderer.device)
    out = renderer.shade_rays_indirect(tt, ss, rays, grid, far=FAR)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(renderer.device) - base == 257 * 16 + (-257 * 16) % 512, "the result alone (512-byte blocks)"
    sh, hits = renderer.light_probes_indirect(tt, ss, pos, grid, directions=64, far=FAR)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(renderer.device) - base == 257 * 16 + (-257 * 16) % 512 + 5 * 160 + (-5 * 160) % 512
    assert tuple(out.shape) == (257, 4) and tuple(sh.shape) == (5, 9, 4)
    # far=None is the camera's far; no rays and no probes launch nothing
    a = renderer.shade_rays_indirect(tt, ss, rays, grid)
    b = renderer.shade_rays_indirect(tt, ss, rays, grid, far=sc[0].initialFar)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert tuple(renderer.shade_rays_indirect(tt, ss, np.zeros((0, 8), f32), grid).shape) == (0, 4)
    assert tuple(renderer.light_probes_indirect(tt, ss, np.zeros((0, 4), f32), grid, directions=64)[0].shape) == (0, 9, 4)
    after = renderer.render(t, s, W, H).cpu().numpy()
    assert lib().rm_debug_last_path() == path and lib().rm_debug_last_split() == split
    S.assert_bits(after, before, "a single frame around the calls")


def test_overlap_host_pointers_and_layers_are_refused(renderer):
    name = "generic_nosec"
    scene, s, res = S.case(name)
    t = S.tables_of(scene, res)
    _, objs, no, lights, nl, g = scene
    grid = grid_of(renderer, name, "strides", True)   # 24 probes
    pos = torch.zeros((24, 4), device=renderer.device)
    # a bake into the grid it reads, whole or in part
    with pytest.raises(RaymarcherError, match="overlaps"):
        renderer.light_probes_indirect(t, s, pos, grid, directions=16, out=grid.probes)
    twice = torch.zeros((48, 40), device=renderer.device)
    part = LightGrid(renderer, twice[12:36], grid.origin, grid.step, grid.dims)
    for lo in (0, 24):
        with pytest.raises(RaymarcherError, match="overlaps"):
            renderer.light_probes_indirect(t, s, pos, part, directions=16, out=twice[lo:lo + 24])
    torch.cuda.synchronize()
    assert not twice.any(), "a refused call wrote"
    beside = LightGrid(renderer, twice[24:48], grid.origin, grid.step, grid.dims)
    renderer.light_probes_indirect(t, s, pos, beside, directions=16, out=twice[0:24])   # buffers that touch are fine
    # host memory in the grid, in the rays, in the result
    out, check = h.guarded((8, 4), device=renderer.device)
    rays = torch.from_numpy(np.array(rays_of(name, 64))[:8].copy()).to(renderer.device)
    host = np.zeros(8192, f32)
    hp = (host.ctypes.data + 15) & ~15

    def call(d_rays, d_out, probes, depth):
        ref = grid.ref()
        ref.d_probes, ref.d_depth = probes, depth
        return lib().rm_shade_rays_indirect(C.c_void_p(d_rays), 8, FAR, objs, no, lights, nl, C.byref(g), C.byref(s), None, C.byref(ref),
                                            C.c_void_p(d_out), None)

    good = (rays.data_ptr(), out.data_ptr(), grid.probes.data_ptr(), grid.depth.data_ptr())
    for at, word in ((0, "d_rays"), (1, "d_rgba"), (2, "grid.d_probes"), (3, "grid.d_depth")):
        args = list(good)
        args[at] = hp
        assert call(*args) == abi.RM_ERR_INVALID_ARGUMENT and word in lib().rm_last_error().decode(), word
    torch.cuda.synchronize()
    assert bool((out.view(torch.int32) == h._i32(h.FLOAT_POISON)).all()), "a refused call wrote into d_rgba"
    assert call(*good) == abi.RM_OK and call(good[0], good[1], good[2], None) == abi.RM_OK
    torch.cuda.synchronize()
    check()
    for feat in (abi.RM_FEAT_TERRAIN, abi.RM_FEAT_CLOUD, abi.RM_FEAT_SEA):
        with pytest.raises(RaymarcherError) as err:
            renderer.shade_rays_indirect(t, abi.default_settings(features=feat), rays, grid)
        assert err.value.status == abi.RM_ERR_UNSUPPORTED
    with pytest.raises(RaymarcherError):
        renderer.shade_rays_indirect(t, s, rays, grid, strength=float("nan"))
    with pytest.raises(ValueError):
        renderer.shade_rays_indirect(t, s, rays, grid_of(renderer, name, "strides", False), visible=True)


# ---------------------------------------------------------------- render_lit
def test_render_lit_is_shade_rays_indirect_on_camera_rays_and_agrees_with_render_indirect(renderer):
    W, H = 24, 16
    scene, s = wall_scene()
    t = S.tables_of(scene)
    grid = renderer.light_grid_visible(t, s, (6, 4, 6), bounds=((-2.5, -0.5, -2.5), (2.5, 2.5, 2.5)), directions=64)
    lit = renderer.render_lit(t, s, W, H, grid, strength=0.9)
    assert tuple(lit.shape) == (1, H, W, 4)
    rays = camera_rays(scene[0], W, H)
    want = renderer.shade_rays_indirect(t, s, rays, grid, far=scene[0].initialFar, strength=0.9)
    assert torch.equal(lit.view(-1, 4).view(torch.int32), want.view(torch.int32)), "tile order and back: every pixel its own ray"
    # the torch route: render_batch + render_gbuffer + light_gbuffer + albedo arithmetic.  Where e >= 0 the two differ by the
    # roundings of the torch route's products alone: eight at the most
    old = renderer.render_indirect(t, s, W, H, grid, strength=0.9).cpu().numpy().astype(np.float64)
    nd, ids, pos = renderer.render_gbuffer(t, s, W, H, [scene[0]], position=True)
    e = grid.light_gbuffer(nd, pos).cpu().numpy()[..., 0:3]
    colour = renderer.render_batch(t, s, W, H, [scene[0]]).cpu().numpy().astype(np.float64)
    new = lit.cpu().numpy().astype(np.float64)
    ok = (e >= 0).all(axis=-1) & (ids.cpu().numpy() >= 0)
    assert ok.sum() > W * H // 4
    ind = np.abs(new[..., 0:3] - colour[..., 0:3])
    bound = 8 * 2.0 ** -24 * (np.abs(colour[..., 0:3]) + ind)
    err = np.abs(new[..., 0:3] - old[..., 0:3])
    print(f"render_lit against render_indirect: {ok.sum()} pixels, largest error / bound {np.max(err[ok] / np.maximum(bound[ok], 1e-30)):.3f}")
    assert (err[ok] <= bound[ok]).all() and (ind[ok] > 0).any()
    miss = ids.cpu().numpy() < 0
    assert (new[miss] == colour[miss]).all()


# ---------------------------------------------------------------- end to end: light reaches the shadowed half by bouncing
def test_bounces_carry_light_behind_the_wall(renderer):
    """test_gpu_light_depth's wall scene: the side x < 0 lies in the wall's shadow and direct light alone leaves it dark.  cDiffuse
    is not negative and there is no fractal, so every bounce adds terms that are not negative to every ray."""
    scene, s = wall_scene()
    t = S.tables_of(scene)
    dims, bounds = (6, 4, 6), ((-2.5, -0.5, -2.5), (2.5, 2.5, 2.5))
    grids = [renderer.light_grid_bounces(t, s, dims, bounces=b, bounds=bounds, directions=256) for b in (0, 1, 2)]
    direct = renderer.light_grid_visible(t, s, dims, bounds=bounds, directions=256)
    assert torch.equal(grids[0].probes.view(torch.int32), direct.probes.view(torch.int32)), "no bounce is light_grid_visible's grid"
    hits = [g.probes[:, 36].view(torch.int32).cpu().numpy() for g in grids]
    assert all((hh == hits[0]).all() for hh in hits) and all(g.depth is not None and torch.equal(g.depth, grids[0].depth) for g in grids)
    live = hits[0] >= 0
    band0 = [g.probes[:, 0:3].cpu().numpy()[live] for g in grids]
    x = G.positions(grids[0].origin, grids[0].step, dims)[live][:, 0]
    shadowed = x < 0
    assert shadowed.sum() == live.sum() // 2
    for a, b, step in ((band0[0], band0[1], "the first bounce"), (band0[1], band0[2], "the second bounce")):
        print(f"{step}: band-0 mean of the shadowed half {a[shadowed].mean():.5f} → {b[shadowed].mean():.5f}, of the lit half {a[~shadowed].mean():.5f} → {b[~shadowed].mean():.5f}")
        assert (b >= a).all(), f"{step}: no probe's band-0 coefficient decreases"
        assert (b[shadowed] > a[shadowed]).all(axis=1).any(), f"{step}: a probe of the shadowed half gains light"
