"""rm_light_grid_irradiance / LightGrid on the GPU: all eight words of every record bit for bit against the NumPy definition
(tests/light_grid_spec.py) — facing off and on, on the three grids of light_grid_helpers.GRIDS with one invalid probe of NaN
coefficients each (and, in the one-cell grid, with every probe invalid), for 1, 64, 65 and 257 points with their edge cases
(light_grid_helpers.points), into poisoned, guarded buffers.  Then: points asked alone, the path, the memory the call allocates, a
frame before and after, Renderer.light_grid against a direct light_probes call and sdf_grid's mask, light_gbuffer against
irradiance, render_indirect against its composition, and the refusals that need the device."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import helpers as h
import light_grid_helpers as M
import light_grid_spec as G
import shade_helpers as S
from raymarcher_amd import LightGrid, abi, lib, light_grid_positions, mesh_bounds

pytestmark = pytest.mark.gpu

f32 = np.float32
CASE = "generic_nosec"  # five primitives, three lights


def as_rows(rec):
    """PROBE records → float32 (n, 40), every word as it is."""
    return np.array(rec).view(f32).reshape(-1, 40)


def grid_of(renderer, name, rec):
    dims, origin, step, _, _ = M.GRIDS[name]
    return LightGrid(renderer, torch.from_numpy(as_rows(rec)).to(renderer.device), origin, step, dims)


def records_of(out):
    return np.frombuffer(out.cpu().numpy().tobytes(), G.GRIDLIGHT, out.shape[0])


def query_guarded(renderer, grid, pts, nrm, facing):
    """LightGrid.irradiance into a poisoned, guarded buffer, checked → GRIDLIGHT records.  pts, nrm: device tensors (n, 4)."""
    n = pts.shape[0]
    out, check = h.guarded((n, 8), device=renderer.device)
    path, split = lib().rm_debug_last_path(), lib().rm_debug_last_split()
    e, weight, probes = grid.irradiance(pts, nrm, facing=facing, out=out)
    assert (lib().rm_debug_last_path(), lib().rm_debug_last_split()) == (path, split), "a lookup is no render launch"
    check()
    assert e.data_ptr() == out.data_ptr() and tuple(e.shape) == (n, 4) and tuple(weight.shape) == (n,) and probes.dtype == torch.int32
    rec = records_of(out)
    assert (rec["probes"] == probes.cpu().numpy()).all() and (rec["weight"].view(np.uint32) == weight.cpu().numpy().view(np.uint32)).all()
    assert (rec["e"].view(np.uint32) == e.cpu().numpy().view(np.uint32)).all()
    return rec


def upload(renderer, *arrays):
    return [torch.from_numpy(np.array(a)).to(renderer.device) for a in arrays]


# ---------------------------------------------------------------- the kernel equals the definition in every word
@pytest.mark.parametrize("facing", [False, True])
@pytest.mark.parametrize("name", list(M.GRIDS))
def test_kernel_equals_the_definition_in_every_word(renderer, name, facing):
    dims, origin, step, _, _ = M.GRIDS[name]
    variants = [("one invalid probe", M.records(name))] + ([("every probe invalid", M.records(name, True))] if name == "one_cell" else [])
    for label, rec in variants:
        grid = grid_of(renderer, name, rec)
        for n in M.COUNTS:
            pts, nrm = M.points(name, n)
            want = G.grid_light(rec, dims, origin, step, pts, nrm, facing)
            got = query_guarded(renderer, grid, *upload(renderer, pts, nrm), facing)
            G.assert_records_equal(got, want, f"{name}, {n} points, facing {facing}, {label}")
            if label == "every probe invalid":
                ok = G.valid_points(pts, nrm)
                assert (got["probes"][ok] == 0).all() and (got["probes"][~ok] == abi.RM_RAY_INVALID).all() and not got["e"].view(np.uint32).any()


def test_numpy_points_of_three_columns_are_uploaded(renderer):
    name = "strides"
    dims, origin, step, _, _ = M.GRIDS[name]
    rec = M.records(name)
    pts, nrm = M.points(name, 65)
    grid = LightGrid(renderer, as_rows(rec), origin, step, dims)  # and NumPy records
    e, weight, probes = grid.irradiance(np.array(pts[:, 0:3]), np.array(nrm[:, 0:3]))  # facing defaults to on
    want = G.grid_light(rec, dims, origin, step, pts, nrm, True)
    got = np.zeros(65, G.GRIDLIGHT)
    got["e"], got["weight"], got["probes"] = e.cpu().numpy(), weight.cpu().numpy(), probes.cpu().numpy()
    G.assert_records_equal(got, want, "(n, 3) NumPy points and normals")
    got = np.ascontiguousarray(light_grid_positions(grid.origin, grid.step, grid.dims)[:, 0:3])
    assert (got.view(np.uint32) == G.positions(origin, step, dims).view(np.uint32)).all()
    e0, w0, p0 = grid.irradiance(np.zeros((0, 3), f32), np.zeros((0, 4), f32))
    assert tuple(e0.shape) == (0, 4) and tuple(w0.shape) == (0,) and tuple(p0.shape) == (0,)
    with pytest.raises(ValueError):
        grid.irradiance(np.array(pts), np.array(nrm[:5]))
    with pytest.raises(ValueError):
        LightGrid(renderer, as_rows(rec)[:-1], origin, step, dims)


# ---------------------------------------------------------------- a point does not depend on the points it shares a call with
@pytest.mark.parametrize("name, facing", [("anisotropic", True), ("strides", False)])
def test_points_asked_alone_equal_the_same_points_of_a_call(renderer, name, facing):
    grid = grid_of(renderer, name, M.records(name))
    pts, nrm = upload(renderer, *M.points(name, 65))
    together = query_guarded(renderer, grid, pts, nrm, facing)
    alone = np.zeros(65, G.GRIDLIGHT)
    out = torch.empty((1, 8), device=renderer.device)
    for i in range(65):
        grid.irradiance(pts[i:i + 1], nrm[i:i + 1], facing=facing, out=out)
        alone[i] = records_of(out)[0]
    G.assert_records_equal(alone, together, f"{name}: every point alone")


# ---------------------------------------------------------------- the memory, the path, a frame before and after
def test_the_call_allocates_its_result_alone_and_leaves_the_renderer_as_it_was(renderer):
    W, H = 64, 36
    scene, s, res = S.case(CASE, W, H)
    t = S.tables_of(scene, res)
    before = renderer.render(t, s, W, H).cpu().numpy()
    path, split = lib().rm_debug_last_path(), lib().rm_debug_last_split()
    name = "anisotropic"
    grid = grid_of(renderer, name, M.records(name))
    pts, nrm = upload(renderer, *M.points(name, 64))
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated(renderer.device)
    e, weight, probes = grid.irradiance(pts, nrm)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(renderer.device) - held == 64 * 32 == e.numel() * 4 + weight.numel() * 4 + probes.numel() * 4 + 64 * 8
    assert (lib().rm_debug_last_path(), lib().rm_debug_last_split()) == (path, split)
    after = renderer.render(t, s, W, H).cpu().numpy()
    assert (lib().rm_debug_last_path(), lib().rm_debug_last_split()) == (path, split)
    S.assert_bits(after, before, "a single frame around rm_light_grid_irradiance")


# ---------------------------------------------------------------- Renderer.light_grid, light_gbuffer, render_indirect
@pytest.fixture(scope="module")
def baked(renderer):
    """Renderer.light_grid on CASE, dims (3, 3, 3), 64 directions: unmasked, then masked at the median scene distance of its probes."""
    scene, s, res = S.case(CASE, 16, 8)
    t = S.tables_of(scene, res)
    dims = (3, 3, 3)
    plain = renderer.light_grid(t, s, dims, directions=64, mask_inside=None)
    dist = renderer.sdf_grid(t, s, plain.origin, plain.step, dims).reshape(-1).cpu().numpy()
    threshold = float(np.median(dist))
    masked = renderer.light_grid(t, s, dims, directions=64, mask_inside=threshold)
    return t, s, dims, plain, masked, dist, threshold


def test_light_grid_bakes_one_probes_call_and_masks_by_the_scene_distance(renderer, baked):
    t, s, dims, plain, masked, dist, threshold = baked
    lo, hi = mesh_bounds(t)
    assert (plain.origin == lo).all() and plain.dims == dims and (masked.origin == plain.origin).all() and (masked.step == plain.step).all()
    assert np.abs(plain.origin.astype(np.float64) + 2 * plain.step.astype(np.float64) - hi).max() <= 1e-6 * np.abs(hi).max()
    positions = light_grid_positions(plain.origin, plain.step, dims)
    sh, hits = renderer.light_probes(t, s, positions, directions=64)
    direct = np.concatenate([sh.cpu().numpy().reshape(27, 36), hits.cpu().numpy().view(f32)[:, None], np.zeros((27, 3), f32)], axis=1)
    h.assert_bit_equal(plain.probes.cpu().numpy(), direct, "the unmasked grid against a direct light_probes call")
    assert (hits.cpu().numpy() >= 0).all()
    inside = dist < f32(threshold)
    assert 0 < inside.sum() < 27
    want = direct.copy()
    want.view(np.int32)[inside, 36] = abi.RM_RAY_INVALID
    h.assert_bit_equal(masked.probes.cpu().numpy(), want, "the masked grid: hits = RM_RAY_INVALID exactly where sdf_grid is below the threshold")
    # the default masks the probes inside geometry
    default = renderer.light_grid(t, s, dims, directions=64)
    got = default.probes.cpu().numpy()[:, 36].view(np.int32)
    assert ((got == abi.RM_RAY_INVALID) == (dist < 0)).all()


def test_at_the_unmasked_probes_the_light_is_the_probes_own_convolution(renderer, baked):
    t, s, dims, plain, masked, dist, threshold = baked
    rec = np.frombuffer(masked.probes.cpu().numpy().tobytes(), G.PROBE, 27)
    keep = np.nonzero(rec["hits"] >= 0)[0]
    rng = np.random.default_rng(41)
    nrm = rng.normal(size=(len(keep), 4))
    nrm = (nrm / np.linalg.norm(nrm[:, 0:3], axis=1, keepdims=True)).astype(f32)
    pts = light_grid_positions(masked.origin, masked.step, dims)[keep]
    got = query_guarded(renderer, masked, *upload(renderer, pts, nrm), False)
    G.assert_records_equal(got, G.grid_light(rec, dims, masked.origin, masked.step, pts, nrm, False), "against the definition")
    E = G.convolve(rec["sh"][keep], G.lobe(nrm[:, 0:3]))
    assert (got["weight"] == 1).all() and (got["probes"] == 1).all()
    there = E != 0  # a zero of E_c may change its sign on the way through the tree: the other seven leaves are zeros too
    assert there.sum() >= 3 * len(keep) and (got["e"].view(np.uint32)[there] == E.view(np.uint32)[there]).all() and (got["e"][~there] == 0).all()


def test_light_gbuffer_is_irradiance_at_the_hit_points_and_zeros_on_misses(renderer, baked):
    t, s, dims, plain, masked, dist, threshold = baked
    W, H = 16, 8
    nd, ids, pos = renderer.render_gbuffer(t, s, W, H, position=True)
    for facing in (True, False):
        img = masked.light_gbuffer(nd, pos, facing=facing)
        assert tuple(img.shape) == (1, H, W, 4) and img.dtype == torch.float32
        e, weight, probes = masked.irradiance(pos.reshape(-1, 4), nd.reshape(-1, 4), facing=facing)
        h.assert_bit_equal(img.cpu().numpy().reshape(-1, 4), e.cpu().numpy(), f"light_gbuffer, facing {facing}")
        miss = (ids.reshape(-1) < 0).cpu().numpy()
        print(f"{(~miss).sum()} hits and {miss.sum()} misses of {W * H} pixels")
        assert (~miss).any() and (probes.cpu().numpy()[miss] == abi.RM_RAY_INVALID).all() and (probes.cpu().numpy()[~miss] >= 0).all()
        assert not img.cpu().numpy().reshape(-1, 4)[miss].view(np.uint32).any(), "a miss has a zero normal: an invalid point, zeros"
        # and the definition on the downloaded G-buffer
        rec = np.frombuffer(masked.probes.cpu().numpy().tobytes(), G.PROBE, 27)
        want = G.grid_light(rec, dims, masked.origin, masked.step, pos.reshape(-1, 4).cpu().numpy(), nd.reshape(-1, 4).cpu().numpy(), facing)
        h.assert_bit_equal(e.cpu().numpy(), want["e"], f"the G-buffer's points against the definition, facing {facing}")


def test_render_indirect_adds_the_grids_diffuse_light_on_hit_pixels(renderer, baked):
    t, s, dims, plain, masked, dist, threshold = baked
    W, H = 16, 8
    frames = renderer.render_batch(t, s, W, H, [t.camera]).cpu().numpy()
    nd, ids, pos = renderer.render_gbuffer(t, s, W, H, position=True)
    e = masked.light_gbuffer(nd, pos).cpu().numpy().astype(np.float64)
    ids = ids.cpu().numpy()
    albedo = np.array([list(t.objects[i].cDiffuse) for i in range(t.num_objects)], np.float64)
    strength = 0.75
    add = np.where((ids >= 0)[..., None], strength * t.globals_.kd * albedo[np.maximum(ids, 0)] * e[..., 0:3] / math.pi, 0.0)
    got = renderer.render_indirect(t, s, W, H, masked, strength=strength).cpu().numpy()
    assert got.shape == frames.shape == (1, H, W, 4)
    assert (got[..., 3] == frames[..., 3]).all() and (got[ids < 0] == frames[ids < 0]).all()
    want = frames[..., 0:3].astype(np.float64) + add
    # plain float32 array arithmetic, not bit-defined: three products and one sum, a few binary32 roundings of values of order 1
    assert np.abs(got[..., 0:3] - want).max() <= 8 * 2.0 ** -24 * max(1.0, np.abs(want).max())
    assert np.abs(add).max() > 1e-4, "the grid does light the scene"
    assert (renderer.render_indirect(t, s, W, H, masked, strength=0.0).cpu().numpy() == frames).all()


# ---------------------------------------------------------------- refusals that need the device
def test_host_pointers_and_misaligned_tensors_are_refused(renderer):
    name = "strides"
    dims, origin, step, _, _ = M.GRIDS[name]
    n = 8
    probes = torch.from_numpy(as_rows(M.records(name))).to(renderer.device)
    pts, nrm = upload(renderer, *M.points(name, 64))
    out, check = h.guarded((n, 8), device=renderer.device)  # refused calls touch nothing: the guards and the poison hold to the end
    host = np.zeros(4096, f32)
    hp = (host.ctypes.data + 15) & ~15
    d, o, st = (C.c_int * 3)(*dims), (C.c_float * 3)(*origin), (C.c_float * 3)(*step)

    def call(a, p, v, r):
        return lib().rm_light_grid_irradiance(C.c_void_p(a), d, o, st, C.c_void_p(p), C.c_void_p(v), n, 1, C.c_void_p(r), None)

    good = (probes.data_ptr(), pts.data_ptr(), nrm.data_ptr(), out.data_ptr())
    for k, word in enumerate(("d_probes", "d_points", "d_normals", "d_out")):
        args = list(good)
        args[k] = hp
        assert call(*args) == abi.RM_ERR_INVALID_ARGUMENT and word in lib().rm_last_error().decode(), word
        args[k] = good[k] + 4
        assert call(*args) == abi.RM_ERR_INVALID_ARGUMENT and "16-byte aligned" in lib().rm_last_error().decode(), word
    torch.cuda.synchronize()
    assert bool((out.view(torch.int32) == h._i32(h.FLOAT_POISON)).all()), "a refused call wrote into d_out"
    assert call(*good) == abi.RM_OK
    torch.cuda.synchronize()
    check()
