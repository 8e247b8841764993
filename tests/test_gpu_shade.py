"""rm_shade_rays / Renderer.shade_rays on the GPU: all eight words (colour and bright) of every ray bit for bit against the
specification (tests/shade_spec/rm_shade_spec.c: the oracle's shadePixel from the background colour on, restated with the oracle's
own functions and pinned to rmo_render_res by tests/test_shade_spec.py) — for each of the twelve kernel classes, on seeded rays
from inside, on and far outside the cull ball, scaled and unit directions, with invalid rays in every wave, at ray counts around
the wave and workgroup sizes, into poisoned, guarded buffers.  Then: a shuffled call gives the shuffled colours; a camera's own rays
give rm_render's frame; calls back to back keep their tables apart and leave the single-frame state alone; a panorama of a lone
sphere; the refusals that need the device."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import helpers as h
import shade_helpers as S
import trace_helpers as T
from raymarcher_amd import RaymarcherError, abi, camera_rays, lib, panorama_rays, tile_order
from raymarcher_amd.render import SceneTables

pytestmark = pytest.mark.gpu

N = 4099
SIZES = (1, 63, 64, 65, 257, N)
FAR = 100.0
NAMES = list(S.CASES)


@functools.lru_cache(maxsize=None)
def rays_of(name, unit=False):
    """The case's N seeded rays (read-only, shared): T.seeded_rays around the cull bounds of its table; unit: the same rays with
    their directions normalised in float32."""
    scene, _, _ = S.case(name)
    centre, radius = T.cull_bounds(scene[1], scene[2], scene[5])
    rays = T.seeded_rays(np.random.default_rng(2000 + NAMES.index(name)), N, centre, radius)
    if unit:
        rays = S.normalised(rays)
    rays.setflags(write=False)
    return rays


@functools.lru_cache(maxsize=None)
def spec_of(name, unit=False, far=FAR):
    """The specification's colour and bright of the case's rays → float32 (N, 8), computed once and shared (read-only)."""
    scene, s, res = S.case(name)
    want = np.concatenate(S.spec_shade(scene, s, rays_of(name, unit), far, res), axis=1)
    want.setflags(write=False)
    return want


def shade_guarded(renderer, scene, s, res, rays, far=FAR, bright=True):
    """Renderer.shade_rays into poisoned, guarded buffers, checked → numpy (n, 8) (colour | bright) or (n, 4)."""
    out, check = h.guarded((len(rays), 4), device=renderer.device)
    kw = {}
    if bright:
        kw["out_bright"], check_b = h.guarded((len(rays), 4), device=renderer.device)
    got = renderer.shade_rays(S.tables_of(scene, res), s, np.array(rays), far=far, out=out, **kw)  # a writable copy of the shared rays
    assert lib().rm_debug_last_path() == S.PATH_SHADE == abi.RM_PATH_SHADE_RAYS and lib().rm_debug_last_split() == 0
    check()
    if not bright:
        assert got.data_ptr() == out.data_ptr()
        return out.cpu().numpy()
    check_b()
    assert got[0].data_ptr() == out.data_ptr() and got[1].data_ptr() == kw["out_bright"].data_ptr()
    return np.concatenate([out.cpu().numpy(), kw["out_bright"].cpu().numpy()], axis=1)


# ---------------------------------------------------------------- (d) the kernel equals the specification in all eight words
@pytest.mark.parametrize("unit", [False, True], ids=["scaled", "unit"])
@pytest.mark.parametrize("name", NAMES)
def test_kernel_equals_the_spec_in_every_bit(renderer, name, unit):
    scene, s, res = S.case(name)
    assert S.class_of(scene, s) == S.CASES[name][0], "the case is not of the class it is listed under"
    rays, want = rays_of(name, unit), spec_of(name, unit)
    invalid = want[:, 3] == 0.0
    assert invalid.sum() >= 100 and (T.bits(want[invalid]) == 0).all() and (want[~invalid, 3] >= 1.0).all()
    if name != "empty":
        assert len(np.unique(want[:, 0:3], axis=0)) > 100, "the case should hold many colours"
    if S.CASES[name][0][3]:
        assert (want[:, 3] >= 2.0).sum() >= 20, "a class with secondary rays should show bounces"
    for n in SIZES:
        got = shade_guarded(renderer, scene, s, res, rays[:n])
        S.assert_bits(got, want[:n], f"{name} {'unit' if unit else 'scaled'} {n} rays")


def test_every_kernel_class_is_covered():
    assert S.CLASSES == sorted((b, e, t, c) for b, e, t in ((0, 0, 0), (1, 0, 0), (2, 0, 0), (0, 1, 0), (0, 0, 1), (0, 1, 1)) for c in (0, 1))


@pytest.mark.parametrize("name", ["generic_nosec", "plain_bulb_nosec", "generic_sec"])
@pytest.mark.parametrize("what", ["no_steps", "no_lights", "far_zero", "far_short"])
def test_degenerate_settings_equal_the_spec(renderer, name, what):
    scene, s, res = S.case(name)
    s = abi.RmSettings.from_buffer_copy(bytes(s))
    far = FAR
    rays = rays_of(name, True)[:257]
    if what == "no_steps":
        s.maxSteps = 0
    elif what == "no_lights":
        scene = scene[:3] + (None, 0) + scene[5:]
    elif what == "far_zero":
        far = 0.0
    else:  # the march ends a radius short of the cull ball for the rays that start three radii out
        _, radius = T.cull_bounds(scene[1], scene[2], scene[5])
        far = float(radius)
    want = np.concatenate(S.spec_shade(scene, s, rays, far, res), axis=1)
    S.assert_bits(shade_guarded(renderer, scene, s, res, rays, far=far), want, f"{name} {what}")
    if what == "no_steps":  # no march finds anything; far = 0 still takes the reference's first full step, and a hit there counts
        assert (want[want[:, 3] != 0.0, 3] == 1.0).all()


def test_rays_may_be_a_device_tensor_and_bright_is_optional(renderer):
    name = "generic_sec"
    scene, s, res = S.case(name)
    t = S.tables_of(scene, res)
    want = spec_of(name, True)[:257]
    rays = torch.from_numpy(np.array(rays_of(name, True)[:257])).to(renderer.device)
    col = renderer.shade_rays(t, s, rays, far=FAR)
    assert col.shape == (257, 4) and col.dtype == torch.float32
    S.assert_bits(col.cpu().numpy(), want[:, 0:4], "colour alone (d_bright = NULL)")
    col2, br2 = renderer.shade_rays(t, s, rays, far=FAR, bright=True)
    S.assert_bits(np.concatenate([col2.cpu().numpy(), br2.cpu().numpy()], axis=1), want, "colour and bright")
    # far=None is the scene camera's initialFar
    S.assert_bits(renderer.shade_rays(t, s, rays).cpu().numpy(), S.spec_shade(scene, s, rays.cpu().numpy(), scene[0].initialFar, res)[0],
                  "far=None")
    with pytest.raises(ValueError):
        renderer.shade_rays(t, s, rays[:, :7])
    with pytest.raises(ValueError):
        renderer.shade_rays(t, s, rays, out=torch.empty((257, 3), device=renderer.device))


# ---------------------------------------------------------------- (e) grouping: a shuffled call gives the shuffled colours
@pytest.mark.parametrize("name", ["plain_bulb_nosec", "moved_bulb_sec", "generic_nosec", "generic_sec"])
def test_a_shuffled_call_gives_the_shuffled_colours(renderer, name):
    """The pooled bulb class (hard shadows, directional lights only) marches a ray's shadow rays on whichever lane of the wave is
    idle, and the table walk switches wave-uniform paths on what the lanes of a wave agree on: another set of neighbours must not
    change a bit of any ray's colour."""
    scene, s, res = S.case(name)
    if name.startswith("plain_bulb"):
        assert s.enableSoftShadow == 0 and all(scene[3][i].type == abi.RM_LIGHT_DIRECTIONAL for i in range(scene[4]))
    if name == "generic_nosec":
        assert s.enableSoftShadow == 1
    rays = rays_of(name, True)
    perm = np.random.default_rng(77).permutation(N)
    straight = shade_guarded(renderer, scene, s, res, rays)
    shuffled = shade_guarded(renderer, scene, s, res, rays[perm])
    S.assert_bits(shuffled, straight[perm], f"{name} shuffled")
    S.assert_bits(straight, spec_of(name, True), name)


# ---------------------------------------------------------------- (f) a camera's rays give rm_render's frame
@pytest.mark.parametrize("W,H", [(64, 36), (37, 23)])
@pytest.mark.parametrize("name", NAMES)
def test_camera_rays_shaded_equal_the_rendered_frame(renderer, name, W, H):
    scene, s, res = S.case(name, W, H)
    t = S.tables_of(scene, res)
    frame, frame_b = renderer.render(t, s, W, H, bright=True)
    want = np.concatenate([frame.cpu().numpy().reshape(-1, 4), frame_b.cpu().numpy().reshape(-1, 4)], axis=1)
    rays = camera_rays(scene[0], W, H)
    got = shade_guarded(renderer, scene, s, res, rays, far=scene[0].initialFar)
    S.assert_bits(got, want, f"{name} {W}x{H}")
    alone = shade_guarded(renderer, scene, s, res, rays, far=scene[0].initialFar, bright=False)
    S.assert_bits(alone, want[:, 0:4], f"{name} {W}x{H} with d_bright = NULL")


# ---------------------------------------------------------------- (g) launch state
def test_four_calls_back_to_back_keep_their_tables_apart(renderer):
    names = ["generic_sec", "plain_bulb_nosec", "menger_sec", "tex_sec"]
    n = 257
    outs = [h.guarded((n, 4), device=renderer.device) for _ in names]
    dev = [torch.from_numpy(np.array(rays_of(name, True)[:n])).to(renderer.device) for name in names]
    tabs = [S.tables_of(S.case(name)[0], S.case(name)[2]) for name in names]
    torch.cuda.synchronize()
    for name, t, (out, _), rays in zip(names, tabs, outs, dev):  # nothing waits between the four
        renderer.shade_rays(t, S.case(name)[1], rays, far=FAR, out=out)
    assert lib().rm_debug_last_path() == S.PATH_SHADE
    for name, (out, check) in zip(names, outs):
        check()
        S.assert_bits(out.cpu().numpy(), spec_of(name, True)[:n, 0:4], f"{name} among four calls")


def test_single_frames_before_and_after_are_the_same_bits(renderer):
    W, H = 64, 36
    scene, s, res = S.case("generic_nosec", W, H)
    t = S.tables_of(scene, res)
    before = renderer.render(t, s, W, H).cpu().numpy()
    path, split = lib().rm_debug_last_path(), lib().rm_debug_last_split()
    for name in ("generic_sec", "plain_bulb_nosec"):
        sc, ss, rr = S.case(name)
        shade_guarded(renderer, sc, ss, rr, rays_of(name, True)[:257])
    after = renderer.render(t, s, W, H).cpu().numpy()
    assert lib().rm_debug_last_path() == path and lib().rm_debug_last_split() == split
    S.assert_bits(after, before, "a single frame around rm_shade_rays")


# ---------------------------------------------------------------- (h) a panorama of a lone sphere
def test_panorama_of_a_lone_sphere(renderer):
    W, H, R = 64, 32, 1.2
    centre, pos = np.array([0.4, -0.2, -3.0]), (0.1, 0.3, 0.5)
    objs, no = T.sphere_table(2 * R, tuple(centre))
    for k in range(3):
        objs[0].cAmbient[k], objs[0].cDiffuse[k] = 0.4, 0.8
    lights = (abi.RmLight * 1)(h.make_light(abi.RM_LIGHT_DIRECTIONAL, (1, 1, 1), (-0.3, -1, -0.5)))
    scene = (h.make_camera(pos, (0, 0, -1), (0, 1, 0), 40.0, W, H), objs, no, lights, 1, h.make_globals())
    s = abi.default_settings(features=abi.RM_FEAT_DARK_BACKGROUND)
    img = renderer.render_panorama(SceneTables(*scene), s, W, H, pos, far=FAR)
    assert lib().rm_debug_last_path() == S.PATH_SHADE
    assert tuple(img.shape) == (H, W, 4) and img.dtype == torch.float32
    got = img.cpu().numpy().reshape(-1, 4)
    rays = panorama_rays(pos, W, H)
    S.assert_bits(got, S.spec_shade(scene, s, rays, FAR)[0], "panorama against the spec")
    # the distance of each ray's line from the centre, in float64 (test_trace_spec's margins: 0.9 R inside, 1.1 R outside)
    d = rays[:, 4:7].astype(np.float64)
    v = centre - np.asarray(pos, dtype=np.float64)
    along = d @ v
    miss = np.linalg.norm(v - along[:, None] * d, axis=1)
    inside, outside = (along > 0) & (miss <= 0.9 * R), (along <= 0) | (miss >= 1.1 * R)
    assert inside.sum() >= 10 and outside.sum() >= 1000
    background = (T.bits(got[:, 0:3]) == 0).all(axis=1)
    assert not background[inside].any(), "every ray through the sphere is lit (ambient > 0)"
    assert background[outside].all() and (got[outside, 3] == 1.0).all()
    # tile order is a reordering of the same call
    order = tile_order(W, H)
    tiled = renderer.shade_rays(SceneTables(*scene), s, rays[order], far=FAR).cpu().numpy()
    S.assert_bits(tiled, got[order], "tile order")


# ---------------------------------------------------------------- (i) refusals that need the device
def test_host_pointers_and_misaligned_tensors_are_refused(renderer):
    scene, s, res = S.case("generic_nosec")
    _, objs, no, lights, nl, g = scene
    n = 64
    rays = torch.from_numpy(np.array(rays_of("generic_nosec", True)[:n + 1])).to(renderer.device)
    out, check = h.guarded((n, 4), device=renderer.device)  # refused calls touch nothing: the guards hold to the end
    br, check_b = h.guarded((n, 4), device=renderer.device)
    host = np.zeros((n + 1) * 8 + 8, dtype=np.float32)
    hp = (host.ctypes.data + 15) & ~15

    def call(r, o, b):
        return lib().rm_shade_rays(C.c_void_p(r), n, FAR, objs, no, lights, nl, C.byref(g), C.byref(s), None, C.c_void_p(o),
                                   C.c_void_p(b) if b else None, None)

    assert call(rays.data_ptr(), out.data_ptr(), br.data_ptr()) == abi.RM_OK
    torch.cuda.synchronize()
    for args, word in (((hp, out.data_ptr(), br.data_ptr()), "d_rays"), ((rays.data_ptr(), hp, br.data_ptr()), "d_rgba"),
                       ((rays.data_ptr(), out.data_ptr(), hp), "d_bright")):
        assert call(*args) == abi.RM_ERR_INVALID_ARGUMENT and word in lib().rm_last_error().decode(), word
    for args in ((rays.data_ptr() + 4, out.data_ptr(), br.data_ptr()), (rays.data_ptr(), out.data_ptr() + 8, br.data_ptr()),
                 (rays.data_ptr(), out.data_ptr(), br.data_ptr() + 4), (rays.data_ptr(), out.data_ptr(), br.data_ptr() + 12)):
        assert call(*args) == abi.RM_ERR_INVALID_ARGUMENT and "16-byte aligned" in lib().rm_last_error().decode()
    torch.cuda.synchronize()
    check()
    check_b()
    # through Python: a misaligned view is not contiguous-from-its-base as a (n, 8) tensor must be, and the library refuses the rest
    flat = torch.zeros(n * 8 + 1, dtype=torch.float32, device=renderer.device)
    with pytest.raises(RaymarcherError):
        renderer.shade_rays(S.tables_of(scene), s, flat[1:].view(n, 8), far=FAR)
    with pytest.raises(RaymarcherError):
        renderer.shade_rays(S.tables_of(scene), s, rays[:n], far=float("nan"))
