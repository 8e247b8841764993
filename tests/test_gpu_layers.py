"""rm_shade_rays_layers / rm_trace_rays_layers on the GPU: all eight words of every ray bit for bit against the specification
(tests/layers_spec/rm_layers_spec.c, pinned to rmo_render_res by tests/test_layers_spec.py; a NaN is a NaN, layers_helpers.assert_spec) — for env_scene and sea_scene under
every layer mask, on the cameras' own rays and on seeded rays around the cameras with invalid rays in every wave, at ray counts
around the wave and workgroup sizes, into poisoned, guarded buffers.  Then: a camera's rays give rm_render's frame; the trace
agrees with rm_render_gbuffer where no layer won; without a layer bit the old entry points' bits; a shuffled call gives the
shuffled results; calls back to back keep apart and leave the single-frame state alone; a landscape panorama; the refusals that
need the device."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import helpers as h
import layers_helpers as L
from raymarcher_amd import RaymarcherError, abi, camera_rays, lib, panorama_rays

pytestmark = pytest.mark.gpu

W0, H0 = 64, 36


def far_of(name):
    return L.case(name)[0][0].initialFar


@functools.lru_cache(maxsize=None)
def shade_spec(name, kind):
    """The specification's (colour | bright) rows, float32 (n, 8), of the case's camera rays (64×36) or seeded rays: computed once,
    shared, read-only."""
    scene, s, res = L.case(name)
    rays = L.primary_rays(name, W0, H0) if kind == "camera" else L.seeded_rays(name)
    want = np.concatenate(L.spec_shade_layers(scene, s, rays, far_of(name), W0, res), axis=1)
    want.setflags(write=False)
    return want


@functools.lru_cache(maxsize=None)
def trace_spec(name, kind, mode="closest"):
    scene, s, _ = L.case(name)
    rays = L.primary_rays(name, W0, H0) if kind == "camera" else L.seeded_rays(name)
    want = L.spec_trace_layers(scene[1], scene[2], scene[5], s, rays, W0, mode)
    want.setflags(write=False)
    return want


def shade_guarded(renderer, name, rays, s=None, image_width=W0, far=None, bright=True, W=W0, H=H0):
    """Renderer.shade_rays_layers into poisoned, guarded buffers, checked → numpy (n, 8) (colour | bright) or (n, 4)."""
    scene, s0, res = L.case(name, W, H)
    out, check = h.guarded((len(rays), 4), device=renderer.device)
    kw = {}
    if bright:
        kw["out_bright"], check_b = h.guarded((len(rays), 4), device=renderer.device)
    got = renderer.shade_rays_layers(L.tables_of(scene, res), s0 if s is None else s, np.array(rays), image_width,
                                     far=far_of(name) if far is None else far, out=out, **kw)
    assert lib().rm_debug_last_path() == L.PATH_SHADE_LAYERS == abi.RM_PATH_SHADE_RAYS_LAYERS and lib().rm_debug_last_split() == 0
    check()
    if not bright:
        assert got.data_ptr() == out.data_ptr()
        return out.cpu().numpy()
    check_b()
    return np.concatenate([out.cpu().numpy(), kw["out_bright"].cpu().numpy()], axis=1)


def trace_guarded(renderer, name, rays, s=None, image_width=W0, normals=True, W=W0, H=H0):
    """Renderer.trace_rays_layers into a poisoned, guarded buffer, checked → numpy (n, 8) RmRayHit rows."""
    scene, s0, res = L.case(name, W, H)
    out, check = h.guarded((len(rays), 8), device=renderer.device)
    renderer.trace_rays_layers(L.tables_of(scene), s0 if s is None else s, np.array(rays), image_width, normals=normals, out=out)
    assert lib().rm_debug_last_path() == L.PATH_TRACE_LAYERS == abi.RM_PATH_TRACE_RAYS_LAYERS and lib().rm_debug_last_split() == 0
    check()
    return out.cpu().numpy()


# ---------------------------------------------------------------- (h) both kernels equal their specification in all eight words
@pytest.mark.parametrize("name", L.NAMES)
def test_shade_kernel_equals_the_spec_in_every_bit(renderer, name):
    want = shade_spec(name, "camera")
    L.assert_spec(shade_guarded(renderer, name, L.primary_rays(name, W0, H0)), want, f"{name} camera rays")
    rays, want = L.seeded_rays(name), shade_spec(name, "seeded")
    invalid = want[:, 3] == 0.0
    assert invalid.sum() >= 100 and (L.bits(want[invalid]) == 0).all() and (want[~invalid, 3] >= 1.0).all()
    assert len(np.unique(want[:, 0:3], axis=0)) > 100, "the seeded rays should see many colours"
    for n in L.COUNTS:
        L.assert_spec(shade_guarded(renderer, name, rays[:n]), want[:n], f"{name} {n} seeded rays")


@pytest.mark.parametrize("name", L.NAMES)
def test_trace_kernel_equals_the_spec_in_every_bit(renderer, name):
    want = trace_spec(name, "camera")
    L.assert_spec(trace_guarded(renderer, name, L.primary_rays(name, W0, H0)), want, f"{name} camera rays", id_word=7)
    rays, want = L.seeded_rays(name), trace_spec(name, "seeded")
    ids = L.ids_of(want)
    assert (ids == abi.RM_RAY_INVALID).sum() >= 100
    if L.case(name)[1].features & (L.TERRAIN | L.SEA):
        assert ((ids == L.HIT_TERRAIN) | (ids == L.HIT_SEA)).sum() >= 100, "the seeded rays should reach the layers"
    for n in L.COUNTS:
        L.assert_spec(trace_guarded(renderer, name, rays[:n]), want[:n], f"{name} {n} seeded rays", id_word=7)
    lean = trace_spec(name, "seeded", "no_normal")
    L.assert_spec(trace_guarded(renderer, name, rays, normals=False), lean, f"{name} without normals", id_word=7)


# ---------------------------------------------------------------- (i) a camera's rays give rm_render's frame
@pytest.mark.parametrize("W,H", L.SIZES_WH)
@pytest.mark.parametrize("name", L.NAMES)
def test_camera_rays_shaded_equal_the_rendered_frame(renderer, name, W, H):
    scene, s, res = L.case(name, W, H)
    frame, frame_b = renderer.render(L.tables_of(scene, res), s, W, H, bright=True)
    want = np.concatenate([frame.cpu().numpy().reshape(-1, 4), frame_b.cpu().numpy().reshape(-1, 4)], axis=1)
    rays = camera_rays(scene[0], W, H)
    L.assert_bits(shade_guarded(renderer, name, rays, image_width=W, W=W, H=H), want, f"{name} {W}x{H}")
    alone = shade_guarded(renderer, name, rays, image_width=W, bright=False, W=W, H=H)
    L.assert_bits(alone, want[:, 0:4], f"{name} {W}x{H} with d_bright = NULL")


# ---------------------------------------------------------------- (j) the trace and the G-buffer
@pytest.mark.parametrize("name", L.NAMES)
def test_trace_agrees_with_the_gbuffer_where_no_layer_won(renderer, name):
    scene, s, _ = L.case(name)
    rays = camera_rays(scene[0], W0, H0)
    ids = L.ids_of(trace_guarded(renderer, name, rays))
    _, gb = renderer.render_gbuffer(L.tables_of(scene), L.without_layers(s), W0, H0)
    gb = gb.cpu().numpy().reshape(-1)
    spec_ids = L.ids_of(trace_spec(name, "camera"))
    stands = (gb >= 0) & (spec_ids >= 0)  # an object under the pixel, and no layer in front of it by the specification
    assert ((ids >= 0) == stands).all() and (ids[stands] == gb[stands]).all()
    assert (gb >= 0).sum() >= 15, "the object should be in the frame"


# ---------------------------------------------------------------- (k) without a layer bit: the old entry points' bits
@pytest.mark.parametrize("name", ["env_all", "sea_sky"])
def test_without_a_layer_bit_the_old_entry_points_bits(renderer, name):
    scene, s, res = L.case(name)
    s = L.without_layers(s)
    t = L.tables_of(scene, res)
    rays = torch.from_numpy(np.array(L.seeded_rays(name))).to(renderer.device)
    col, br = renderer.shade_rays(t, s, rays, far=100.0, bright=True)
    want = np.concatenate([col.cpu().numpy(), br.cpu().numpy()], axis=1)
    L.assert_bits(shade_guarded(renderer, name, L.seeded_rays(name), s=s, image_width=7, far=100.0), want, f"{name} shade")
    for normals in (True, False):
        old = torch.empty((len(rays), 8), device=renderer.device)
        renderer.trace_rays(t, s, rays, normals=normals, out=old)
        L.assert_bits(trace_guarded(renderer, name, L.seeded_rays(name), s=s, image_width=7, normals=normals), old.cpu().numpy(),
                      f"{name} trace normals={normals}")
    # occlusion has no Python method of its own here: through the symbol
    old = torch.empty((len(rays), 8), device=renderer.device)
    renderer.trace_rays(t, s, rays, mode="occlusion", out=old)
    new, check = h.guarded((len(rays), 8), device=renderer.device)
    st = lib().rm_trace_rays_layers(C.c_void_p(rays.data_ptr()), len(rays), 7, scene[1], scene[2], C.byref(scene[5]), C.byref(s),
                                    abi.RM_TRACE_OCCLUSION, C.c_void_p(new.data_ptr()), None)
    assert st == abi.RM_OK and lib().rm_debug_last_path() == L.PATH_TRACE_LAYERS
    check()
    L.assert_bits(new.cpu().numpy(), old.cpu().numpy(), f"{name} occlusion")


# ---------------------------------------------------------------- (l) a shuffled call gives the shuffled results
@pytest.mark.parametrize("name", ["env_all_sea", "sea_terrain"])
def test_a_shuffled_call_gives_the_shuffled_results(renderer, name):
    rays = L.seeded_rays(name)
    perm = np.random.default_rng(77).permutation(L.N)
    L.assert_spec(shade_guarded(renderer, name, rays[perm]), shade_spec(name, "seeded")[perm], f"{name} shade shuffled")
    L.assert_spec(trace_guarded(renderer, name, rays[perm]), trace_spec(name, "seeded")[perm], f"{name} trace shuffled", id_word=7)


# ---------------------------------------------------------------- (m) launch state
def test_four_calls_back_to_back_keep_apart(renderer):
    names = ["env_all", "sea_sky", "env_cloud_dark", "sea_terrain"]
    n = 257
    dev = [torch.from_numpy(np.array(L.seeded_rays(name)[:n])).to(renderer.device) for name in names]
    tabs = [L.tables_of(L.case(name)[0], L.case(name)[2]) for name in names]
    outs = [h.guarded((n, 4), device=renderer.device) for _ in names]
    hits = [h.guarded((n, 8), device=renderer.device) for _ in names]
    torch.cuda.synchronize()
    for name, t, (out, _), rays in zip(names, tabs, outs, dev):  # nothing waits between the four
        renderer.shade_rays_layers(t, L.case(name)[1], rays, W0, far=far_of(name), out=out)
    assert lib().rm_debug_last_path() == L.PATH_SHADE_LAYERS and lib().rm_debug_last_split() == 0
    for name, t, (out, _), rays in zip(names, tabs, hits, dev):
        renderer.trace_rays_layers(t, L.case(name)[1], rays, W0, out=out)
    assert lib().rm_debug_last_path() == L.PATH_TRACE_LAYERS and lib().rm_debug_last_split() == 0
    for name, (out, check), (hit, check_h) in zip(names, outs, hits):
        check()
        check_h()
        L.assert_spec(out.cpu().numpy(), shade_spec(name, "seeded")[:n, 0:4], f"{name} shade among four calls")
        L.assert_spec(hit.cpu().numpy(), trace_spec(name, "seeded")[:n], f"{name} trace among four calls", id_word=7)


def test_single_frames_before_and_after_are_the_same_bits(renderer):
    scene, s, res = L.case("env_all")
    t = L.tables_of(scene, res)
    before = renderer.render(t, s, W0, H0).cpu().numpy()
    path, split = lib().rm_debug_last_path(), lib().rm_debug_last_split()
    shade_guarded(renderer, "env_all_sea", L.seeded_rays("env_all_sea")[:257])
    trace_guarded(renderer, "sea_terrain", L.seeded_rays("sea_terrain")[:257])
    after = renderer.render(t, s, W0, H0).cpu().numpy()
    assert lib().rm_debug_last_path() == path and lib().rm_debug_last_split() == split
    L.assert_bits(after, before, "a single frame around the layer calls")


# ---------------------------------------------------------------- (n) a landscape panorama
# Fixed from the CPU specification first (64×32 from env_scene's camera position under SKY | TERRAIN | CLOUD | PERLIN_BUMP): the
# trace names PANO_TERRAIN_LOWER of the 1024 rays of the lower half terrain and PANO_TERRAIN_UPPER of the upper half (far ridges);
# 947 rays of the upper half end on nothing solid and 725 of them show the clear sky's colour, the others a cloud; 6 see the torus.
PANO_TERRAIN_LOWER, PANO_TERRAIN_UPPER = 1023, 71


def test_panorama_of_a_landscape(renderer):
    W, H = 64, 32
    name = "env_all"
    scene, s, res = L.case(name)
    pos = (0.0, 500.0, 5.0)
    img = renderer.render_panorama_layers(L.tables_of(scene, res), s, W, H, pos)
    assert lib().rm_debug_last_path() == L.PATH_SHADE_LAYERS
    assert tuple(img.shape) == (H, W, 4) and img.dtype == torch.float32
    got = img.cpu().numpy().reshape(-1, 4)
    rays = panorama_rays(pos, W, H)
    L.assert_spec(got, L.spec_shade_layers(scene, s, rays, far_of(name), W, res)[0], "panorama against the spec")
    rays[:, 3] = far_of(name)  # panorama_rays leaves tMax 0 (the shade does not read it): the trace goes as far as the shade
    ids = L.ids_of(L.spec_trace_layers(scene[1], scene[2], scene[5], s, rays, W))
    lower, upper = np.arange(W * H) < W * H // 2, np.arange(W * H) >= W * H // 2  # row 0 = bottom
    assert (ids[lower] == L.HIT_TERRAIN).sum() == PANO_TERRAIN_LOWER >= 512, "terrain in the lower half"
    assert (ids[upper] == L.HIT_TERRAIN).sum() == PANO_TERRAIN_UPPER <= 256 and (ids[upper] == -1).sum() >= 768, "sky or cloud above"
    L.assert_bits(L.ids_of(trace_guarded(renderer, name, rays, image_width=W)), ids, "the trace of the panorama's rays")
    # the upper half's sky pixels are the sky's colour or a cloud over it: never the terrain's dark browns
    sky = L.sky_of(rays)
    clear = (L.bits(got[:, 0:3]) == L.bits(sky)).all(axis=1)
    assert clear[upper].sum() >= 725 // 2 and not clear[ids == L.HIT_TERRAIN].any()


# ---------------------------------------------------------------- (o) refusals that need the device
def test_host_pointers_and_misaligned_arrays_are_refused(renderer):
    scene, s, res = L.case("env_all")
    _, objs, no, lights, nl, g = scene
    n = 64
    rays = torch.from_numpy(np.array(L.seeded_rays("env_all")[:n + 1])).to(renderer.device)
    out, check = h.guarded((n, 4), device=renderer.device)  # refused calls touch nothing: the guards hold to the end
    br, check_b = h.guarded((n, 4), device=renderer.device)
    hit, check_h = h.guarded((n, 8), device=renderer.device)
    host = np.zeros((n + 1) * 8 + 8, dtype=np.float32)
    hp = (host.ctypes.data + 15) & ~15

    def shade(r, o, b):
        return lib().rm_shade_rays_layers(C.c_void_p(r), n, 2000.0, W0, objs, no, lights, nl, C.byref(g), C.byref(s), None, C.c_void_p(o),
                                          C.c_void_p(b) if b else None, None)

    def trace(r, o):
        return lib().rm_trace_rays_layers(C.c_void_p(r), n, W0, objs, no, C.byref(g), C.byref(s), 0, C.c_void_p(o), None)

    assert shade(rays.data_ptr(), out.data_ptr(), br.data_ptr()) == abi.RM_OK and trace(rays.data_ptr(), hit.data_ptr()) == abi.RM_OK
    torch.cuda.synchronize()
    for args, word in (((hp, out.data_ptr(), br.data_ptr()), "d_rays"), ((rays.data_ptr(), hp, br.data_ptr()), "d_rgba"),
                       ((rays.data_ptr(), out.data_ptr(), hp), "d_bright")):
        assert shade(*args) == abi.RM_ERR_INVALID_ARGUMENT and word in lib().rm_last_error().decode(), word
    for args, word in (((hp, hit.data_ptr()), "d_rays"), ((rays.data_ptr(), hp), "d_hits")):
        assert trace(*args) == abi.RM_ERR_INVALID_ARGUMENT and word in lib().rm_last_error().decode(), word
    for args in ((rays.data_ptr() + 4, out.data_ptr(), br.data_ptr()), (rays.data_ptr(), out.data_ptr() + 8, br.data_ptr()),
                 (rays.data_ptr(), out.data_ptr(), br.data_ptr() + 12)):
        assert shade(*args) == abi.RM_ERR_INVALID_ARGUMENT and "16-byte aligned" in lib().rm_last_error().decode()
    for args in ((rays.data_ptr() + 4, hit.data_ptr()), (rays.data_ptr(), hit.data_ptr() + 8)):
        assert trace(*args) == abi.RM_ERR_INVALID_ARGUMENT and "16-byte aligned" in lib().rm_last_error().decode()
    torch.cuda.synchronize()
    check()
    check_b()
    check_h()
    # through Python: a misaligned view is refused by the library, and so are a bad imageWidth and occlusion's absence of a method
    flat = torch.zeros(n * 8 + 1, dtype=torch.float32, device=renderer.device)
    t = L.tables_of(scene, res)
    with pytest.raises(RaymarcherError):
        renderer.shade_rays_layers(t, s, flat[1:].view(n, 8), W0)
    with pytest.raises(RaymarcherError):
        renderer.trace_rays_layers(t, s, flat[1:].view(n, 8), W0)
    with pytest.raises(RaymarcherError):
        renderer.shade_rays_layers(t, s, rays[:n], 0)
    with pytest.raises(RaymarcherError):
        renderer.trace_rays_layers(t, s, rays[:n], 0)
