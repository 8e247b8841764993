"""rm_render_adaptive / Renderer.render_adaptive on the GPU.  An adaptive pixel is defined by things the contract already has: the
1-sample frame F of rm_render_batch, the supersampled frame R of rm_render_supersampled and the contrast test M over F —
`adaptive` of test_adaptive_abi.py is that definition in NumPy.  Every class the dispatcher has is compared on the uint32 view, no
tolerance and no excluded pixel, with the oracle's composite (F and R both from the CPU oracle) and with the library's own two
entry points; then the limits of the threshold, write coverage in guarded buffers, chunking under a workspace limit, frames with a
handful of flagged pixels, the schedule (path 8, tuners untouched, wider workgroups, one stream), the device-side errors, and
render_sequence(..., adaptive=t) against the oracle's whole export chain."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as h
import scene_builders as SB
from helpers import assert_bit_equal, tables_of, with_globals
from scene_builders import orbit
from test_adaptive_abi import adaptive
from test_gpu_supersample import CLASSES, ODD, SCENES, class_tables, oracle_resolved
from raymarcher_amd import abi, lib
from raymarcher_amd._lib import RaymarcherError

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


def run(renderer, t, s, W, H, cams, ss, thr, globs=None):
    """One adaptive launch with every output → NumPy (out, bright, mask as bool, counts), path and split asserted."""
    out, br, m, cnt = renderer.render_adaptive(t, s, W, H, cams, ss, thr, globals_=globs, bright=True, mask=True, counts=True)
    assert lib().rm_debug_last_path() == 8 and lib().rm_debug_last_split() == 0
    n = len(cams)
    assert tuple(out.shape) == (n, H, W, 4) and tuple(br.shape) == (n, H, W, 4) and tuple(m.shape) == (n, H, W) and tuple(cnt.shape) == (n,)
    m = m.cpu().numpy()
    assert ((m == 0) | (m == 1)).all()
    return out.cpu().numpy(), br.cpu().numpy(), m.astype(bool), cnt.cpu().numpy().astype(np.int64)


# ---------------------------------------------------------------- 1. bit for bit against the oracle, every class of the dispatcher
def adaptive_vs_oracle(renderer, scene, s, cams_of, globs, sizes=ODD, textures=None, what="", **resources):
    """cams_of(W, H) → the cameras; globs: one RmGlobals or one per camera.  Every frame: fragColor, BrightColor, mask and count
    against the definition applied to the oracle's frames, at threshold 0.1 — under these orbit cameras every frame of every case
    stays inside the band of refined pixels asserted below at that threshold (the closest: sea + sky at 97×61, 7.7 %), so no case
    needs a lower one."""
    th = 0.1
    for ss, W, H in sizes:
        cams = cams_of(W, H)
        t = tables_of(scene, **resources)
        if textures:
            t.textures = textures
        out, br, mask, cnt = run(renderer, t, s, W, H, cams, ss, th, globs)
        for f, cam in enumerate(cams):
            g = globs[f] if isinstance(globs, (list, tuple)) else globs
            F, Fb = h.oracle_render((cam,) + tuple(scene[1:5]) + (g,), s, W, H, bright=True, threads=16, textures=textures, **resources)
            assert np.isfinite(F).all() and np.isfinite(Fb).all(), "the oracle's 1-sample frame is not finite: choose another camera"
            R, Rb = oracle_resolved(scene, cam, g, s, W, H, ss, textures=textures, **resources)
            exp, exp_b, exp_m = adaptive(F, Fb, R, Rb, th)
            share = exp_m.mean()
            print(f"{what} ss {ss} {W}x{H} threshold {th} frame {f}: the oracle refines {100 * share:.1f} %")
            # a condition on the case, not a measurement: both branches of the composite are exercised in every frame
            assert 0.05 < share < 0.95, f"{what} ss {ss} {W}x{H} frame {f}: the oracle's composite refines {100 * share:.1f} % of the pixels"
            assert (mask[f] == exp_m).all(), f"{what} ss {ss} {W}x{H} frame {f}: {(mask[f] != exp_m).sum()} mask bytes differ"
            assert cnt[f] == exp_m.sum(), (what, ss, f, cnt[f], exp_m.sum())
            assert_bit_equal(out[f], exp, f"{what} ss {ss} {W}x{H} frame {f}")
            assert_bit_equal(br[f], exp_b, f"{what} ss {ss} {W}x{H} frame {f} bright")


def test_bulb_plain_form(renderer):
    scene = h.scene_mandelbulb(64, 36)
    globs = [with_globals(scene[5], iTime=0.5 * f) for f in range(4)]
    assert all(lib().rm_debug_bulb_plain(scene[1], 1, C.byref(g)) == 1 for g in globs)
    adaptive_vs_oracle(renderer, scene, abi.default_settings(fractalIters=12),
                       lambda W, H: orbit((0, 0, 4.5), (0, 0, -1), 30.0, W, H, 4, deg=7.0), globs, what="plain bulb")


def test_bulb_general_form_mixed_with_plain(renderer):
    scene = h.scene_mandelbulb(64, 36)
    globs = [with_globals(scene[5], power=(8.0 if f % 2 == 0 else 7.5), iTime=0.3 * f) for f in range(4)]
    assert [lib().rm_debug_bulb_plain(scene[1], 1, C.byref(g)) for g in globs] == [1, 0, 1, 0]
    adaptive_vs_oracle(renderer, scene, abi.default_settings(), lambda W, H: orbit((0, 0, 4.5), (0, 0, -1), 30.0, W, H, 4, deg=5.0), globs,
                       what="power 8 / 7.5 bulb")


def test_primitives_two_lights_soft_shadows_ao(renderer):
    scene = SB.reflect_refract_scene(64, 36)  # reflection / refraction off below: the plain table walk
    globs = [with_globals(scene[5], iTime=0.25 * f) for f in range(3)]
    adaptive_vs_oracle(renderer, scene, abi.default_settings(enableSoftShadow=1, enableAmbientOcclusion=1),
                       lambda W, H: orbit((0, 1.2, 5), (0, -0.2, -1), 40.0, W, H, 3, deg=6.0), globs, what="primitives soft+AO")


def test_reflection_and_refraction_two_bounces(renderer):
    scene = SB.reflect_refract_scene(64, 36)
    s = abi.default_settings(enableReflection=1, enableRefraction=1, numReflection=2)
    adaptive_vs_oracle(renderer, scene, s, lambda W, H: orbit((0, 1.2, 5), (0, -0.2, -1), 40.0, W, H, 3, deg=8.0), scene[5],
                       what="reflection+refraction")


def test_menger_sponge_with_reflection_never_takes_the_wavefront_pipeline(renderer):
    L = lib()
    scene = SB.menger_scene(64, 36)
    globs = [with_globals(scene[5], iTime=3.7 * f) for f in range(3)]
    s = abi.default_settings(mengerLevels=4, enableReflection=1, numReflection=1)
    cams_of = lambda W, H: orbit((2.6, 2.2, 3.0), (-2.6, -2.2, -3.0), 30.0, W, H, 3, deg=5.0)  # noqa: E731
    adaptive_vs_oracle(renderer, scene, s, cams_of, globs, what="menger")
    try:
        assert L.rm_set_kernel_path(5) == 0  # run() asserts path 8 all the same, with the same bits
        adaptive_vs_oracle(renderer, scene, s, cams_of, globs, sizes=ODD[:1], what="menger, path 5 requested")
    finally:
        L.rm_set_kernel_path(0)


def test_textures_sky_box_and_area_light(renderer):
    scene = SB.textured_scene(64, 36)
    s = abi.default_settings(features=abi.RM_FEAT_WHITE_BACKGROUND, enableSoftShadow=1, enableSkyBox=1)
    adaptive_vs_oracle(renderer, scene, s, lambda W, H: orbit((0.4, 2.2, 5.5), (-0.05, -0.35, -1), 42.0, W, H, 3, deg=6.0), scene[5],
                       textures=SB.synthetic_textures(), what="textured + sky box", skybox=SB.synthetic_skybox())
    scene, s, res = SB.resource_case("area_light", 64, 36)
    s.enableSkyBox = 1
    adaptive_vs_oracle(renderer, scene, s, lambda W, H: orbit((0, 1.6, 5.5), (0, -0.2, -1), 45.0, W, H, 3, deg=7.0), scene[5],
                       what="area light + sky box", skybox=SB.synthetic_skybox(), **res)


def test_terrain_and_clouds_with_advancing_time(renderer):
    scene = SB.env_scene(64, 36)
    globs = [with_globals(scene[5], iTime=4.0 * f) for f in range(3)]
    adaptive_vs_oracle(renderer, scene, abi.default_settings(features=SB.ENV_ALL, enableReflection=1),
                       lambda W, H: orbit((0, 500, 5), (0.3, 0.12, -1), 70.0, W, H, 3, deg=3.0, far=2000.0), globs,
                       what="terrain+cloud")


def test_sea_and_night_sky_with_the_noise_texture(renderer):
    scene, s, res = SB.resource_case("sea_sky", 64, 36)
    globs = [with_globals(scene[5], iTime=0.7 + 0.9 * f) for f in range(3)]
    adaptive_vs_oracle(renderer, scene, s, lambda W, H: orbit((0, 3.5, 6), (0, -0.35, -1), 50.0, W, H, 3, deg=5.0), globs,
                       what="sea + sky", **res)
    scene, s, res = SB.resource_case("night_sky", 64, 36)
    adaptive_vs_oracle(renderer, scene, s, lambda W, H: orbit((1.6, 0.4, -5), (-0.42, 0.36, 1), 60.0, W, H, 3, deg=4.0), scene[5],
                       what="night sky", **res)


# ---------------------------------------------------------------- 2. against the library itself
def library_composite(renderer, t, s, W, H, cams, ss, thr, globs=None):
    """(out, bright, mask) of the definition from the library's own rm_render_batch and rm_render_supersampled."""
    F, Fb = renderer.render_batch(t, s, W, H, cams, globals_=globs, bright=True)
    R, Rb = renderer.render_supersampled(t, s, W, H, cams, ss, globals_=globs, bright=True)
    F, Fb, R, Rb = (a.cpu().numpy() for a in (F, Fb, R, Rb))
    parts = [adaptive(F[f], Fb[f], R[f], Rb[f], thr) for f in range(len(cams))]
    return tuple(np.stack([p[i] for p in parts]) for i in range(3)) + (F, Fb, R, Rb)


def assert_is_composite(renderer, t, s, W, H, cams, ss, thr, globs=None, what=""):
    exp, exp_b, exp_m, F, Fb, R, Rb = library_composite(renderer, t, s, W, H, cams, ss, thr, globs)
    out, br, mask, cnt = run(renderer, t, s, W, H, cams, ss, thr, globs)
    assert (mask == exp_m).all(), f"{what}: {(mask != exp_m).sum()} mask bytes differ from the rule applied to render_batch's frame"
    assert (cnt == exp_m.reshape(len(cams), -1).sum(axis=1)).all(), (what, cnt.tolist())
    u = lambda a: np.ascontiguousarray(a).view(np.uint32)  # noqa: E731
    assert (u(out)[mask] == u(R)[mask]).all() and (u(out)[~mask] == u(F)[~mask]).all(), what
    assert (u(br)[mask] == u(Rb)[mask]).all() and (u(br)[~mask] == u(Fb)[~mask]).all(), what + " bright"
    return out, br, mask, cnt


@pytest.mark.parametrize("name", CLASSES)
def test_flagged_pixels_are_supersampled_the_rest_is_render_batch(renderer, name):
    for ss, W, H in ((2, 131, 75), (4, 67, 45)):
        scene, t, s = class_tables(name, W, H)
        assert_is_composite(renderer, t, s, W, H, [scene[0]], ss, 0.1, what=f"{name} ss {ss}")


# ---------------------------------------------------------------- 3. limits
def _three(W, H):
    scene = SB.reflect_refract_scene(W, H)
    s = abi.default_settings(enableReflection=1)
    cams = orbit((0, 1.2, 5), (0, -0.2, -1), 40.0, W, H, 3, deg=8.0)
    globs = [with_globals(scene[5], iTime=0.25 * f) for f in range(3)]
    return scene, tables_of(scene), s, cams, globs


@pytest.mark.parametrize("ss", [1, 2, 4])
def test_threshold_inf_is_render_batch(renderer, ss):
    W, H = 77, 45
    scene, t, s, cams, globs = _three(W, H)
    out, br, mask, cnt = run(renderer, t, s, W, H, cams, ss, INF, globs)
    b, bb = renderer.render_batch(t, s, W, H, cams, globals_=globs, bright=True)
    assert np.isfinite(b.cpu().numpy()).all()
    assert_bit_equal(out, b.cpu().numpy(), "threshold +inf")
    assert_bit_equal(br, bb.cpu().numpy(), "threshold +inf, bright")
    assert not mask.any() and (cnt == 0).all()


@pytest.mark.parametrize("ss", [2, 4])
def test_negative_threshold_is_render_supersampled(renderer, ss):
    W, H = 77, 45
    scene, t, s, cams, globs = _three(W, H)
    out, br, mask, cnt = run(renderer, t, s, W, H, cams, ss, -1.0, globs)
    r, rb = renderer.render_supersampled(t, s, W, H, cams, ss, globals_=globs, bright=True)
    assert_bit_equal(out, r.cpu().numpy(), "threshold -1")
    assert_bit_equal(br, rb.cpu().numpy(), "threshold -1, bright")
    assert mask.all() and (cnt == W * H).all()


def test_ss_1_is_render_batch_with_the_mask_still_computed(renderer):
    W, H = 77, 45
    scene, t, s, cams, globs = _three(W, H)
    out, br, mask, cnt = assert_is_composite(renderer, t, s, W, H, cams, 1, 0.1, globs, what="ss 1")
    b, bb = renderer.render_batch(t, s, W, H, cams, globals_=globs, bright=True)
    assert_bit_equal(out, b.cpu().numpy(), "ss 1")
    assert_bit_equal(br, bb.cpu().numpy(), "ss 1, bright")
    assert mask.any() and not mask.all() and (cnt > 0).all()


@pytest.mark.parametrize("ss", [1, 2, 4])
def test_a_1x1_frame_is_never_flagged(renderer, ss):
    scene, t, s = class_tables("table_sec", 1, 1)
    cams = [scene[0]] * 3
    for thr in (0.1, 0.0, -1.0, -INF):
        out, br, mask, cnt = run(renderer, t, s, 1, 1, cams, ss, thr)
        b, bb = renderer.render_batch(t, s, 1, 1, cams, bright=True)
        assert not mask.any() and (cnt == 0).all()
        assert_bit_equal(out, b.cpu().numpy(), "1x1")
        assert_bit_equal(br, bb.cpu().numpy(), "1x1 bright")


@pytest.mark.parametrize("ss", [2, 4])
def test_pure_background_flags_nothing_at_threshold_0(renderer, ss):
    W, H = 45, 27
    for scene in (h.scene_mandelbulb(W, H), SB.reflect_refract_scene(W, H)):
        away = h.make_camera((0, 0, 4.5), (0, 0, 1), (0, 1, 0), 30.0, W, H)  # every object is behind the camera
        s = abi.default_settings(features=abi.RM_FEAT_WHITE_BACKGROUND)
        t = tables_of((away,) + tuple(scene[1:]))
        one, one_b = renderer.render(t, s, W, H, bright=True)
        assert float(one[..., :3].min()) == 1.0  # nothing but the white background
        out, br, mask, cnt = run(renderer, t, s, W, H, [away], ss, 0.0)
        assert not mask.any() and cnt[0] == 0
        assert_bit_equal(out[0], one.cpu().numpy(), "white background")
        assert_bit_equal(br[0], one_b.cpu().numpy(), "white background, bright")


# ---------------------------------------------------------------- 4. write coverage
@pytest.mark.parametrize("ss,W,H", ODD + [(2, 1, 1), (4, 1, 1), (4, 3, 70), (2, 65, 9)])
@pytest.mark.parametrize("n", [1, 3])
def test_every_word_is_written_and_nothing_else(renderer, ss, W, H, n):
    torch = renderer.torch
    for name in ("bulb_plain", "table_sec"):
        scene, t, s = class_tables(name, W, H)
        cams = [scene[0]] * n
        out, c1 = h.guarded((n, H, W, 4), device=renderer.device)
        br, c2 = h.guarded((n, H, W, 4), device=renderer.device)
        cnt, c3 = h.guarded((n,), torch.int32, device=renderer.device)

        def produce(m):
            renderer.render_adaptive(t, s, W, H, cams, ss, 0.1, out=out, out_bright=br, mask=m, counts=cnt)

        mask = h.guarded_u8((n, H, W), produce, device=renderer.device)  # twice, under two poisons: every mask byte is written
        c1()
        c2()
        c3()
        exp, exp_b, exp_m = library_composite(renderer, t, s, W, H, cams, ss, 0.1)[:3]
        assert (mask.cpu().numpy().astype(bool) == exp_m).all() and (cnt.cpu().numpy() == exp_m.reshape(n, -1).sum(axis=1)).all()
        assert_bit_equal(out.cpu().numpy(), exp, f"{name} guarded")
        assert_bit_equal(br.cpu().numpy(), exp_b, f"{name} guarded bright")
        # d_bright, d_mask, d_refined = NULL in turn: the same frames, and a neighbouring poisoned allocation is left alone
        for kw in (dict(mask=True, counts=True), dict(bright=True, counts=True), dict(bright=True, mask=True), dict()):
            out2, c4 = h.guarded((n, H, W, 4), device=renderer.device)
            spare = h.Guarded((n, H, W, 4), torch.float32, h.FLOAT_POISON, renderer.device)
            got = renderer.render_adaptive(t, s, W, H, cams, ss, 0.1, out=out2, **kw)
            c4()
            assert SB.ieq(out2, out), kw
            assert bool(spare._unwritten(spare.buf).all()), f"a launch with {kw} wrote outside its outputs"
            if "mask" in kw:
                assert bool((got[-2 if "counts" in kw else -1] == mask).all())
        for f in range(1, n):
            assert SB.ieq(out[f], out[0]) and SB.ieq(br[f], br[0]) and bool((mask[f] == mask[0]).all())


# ---------------------------------------------------------------- 5. chunking under a workspace limit
def test_chunks_under_a_workspace_limit_render_the_same_frames(renderer):
    L = lib()
    ss, W, H, n = 2, 61, 37, 5
    scene = h.scene_mandelbulb(W, H)
    s = abi.default_settings(fractalIters=12)
    t = tables_of(scene)
    cams = orbit((0, 0, 4.5), (0, 0, -1), 30.0, W, H, n, deg=9.0)
    globs = [with_globals(scene[5], iTime=0.5 * f) for f in range(n)]
    whole = run(renderer, t, s, W, H, cams, ss, 0.1, globs)
    assert whole[2].any() and not whole[2].all()
    try:
        assert L.rm_release_workspaces(None) == 0
        assert L.rm_set_workspace_limit(2 * 4 * W * H + 4 * W * H - 4) == 0  # two frames' lists fit, three do not: chunks of 2, 2, 1
        chunked = run(renderer, t, s, W, H, cams, ss, 0.1, globs)
        for a, b, what in zip(whole, chunked, ("out", "bright", "mask", "counts")):
            assert (np.ascontiguousarray(a).view(np.uint8) == np.ascontiguousarray(b).view(np.uint8)).all(), what
        assert L.rm_release_workspaces(None) == 0
        assert L.rm_set_workspace_limit(4 * W * H - 4) == 0  # below one frame's list
        with pytest.raises(RaymarcherError) as e:
            renderer.render_adaptive(t, s, W, H, cams, ss, 0.1, globals_=globs)
        assert e.value.status == abi.RM_ERR_DEVICE and "limit" in str(e.value)
        assert renderer.torch.cuda.is_available()
        renderer.torch.cuda.synchronize(renderer.device)  # HIP's error state is clean
        assert L.rm_set_workspace_limit(0) == 0
        again = run(renderer, t, s, W, H, cams, ss, 0.1, globs)  # and the next render succeeds
        assert_bit_equal(again[0], whole[0], "after the refusal")
    finally:
        L.rm_set_workspace_limit(0)


# ---------------------------------------------------------------- 6. frames that flag a handful of pixels each
SMALL_R = 0.18  # about three pixels across at this distance and size


@pytest.mark.parametrize("ss", [2, 4])
def test_frames_with_a_handful_of_flagged_pixels_each(renderer, ss):
    """A small sphere far away on a white background: a few flagged pixels per frame, fewer than one refine wave holds (16 at
    ss = 2), in every frame of a batch whose cameras differ."""
    W, H, n = 64, 40, 6
    sphere = h.make_object(abi.RM_SPHERE, model=h.scale(SMALL_R, SMALL_R, SMALL_R), scale_factor=SMALL_R, diffuse=(0.2, 0.4, 0.9))
    objs = (abi.RmObject * 1)(sphere)
    lights = (abi.RmLight * 1)(h.make_light(abi.RM_LIGHT_DIRECTIONAL, direction=(-0.3, -1, -0.5)))
    cams = [h.make_camera((0.4 * f - 1.0, 0.2 * f, 9.0), (0, 0, -1), (0, 1, 0), 30.0, W, H) for f in range(n)]
    scene = (cams[0], objs, 1, lights, 1, h.make_globals())
    s = abi.default_settings(features=abi.RM_FEAT_WHITE_BACKGROUND)
    t = tables_of(scene)
    out, br, mask, cnt = assert_is_composite(renderer, t, s, W, H, cams, ss, 0.1, what="small sphere")
    assert (cnt > 0).all() and (cnt < 16).all(), cnt.tolist()
    assert len({m.tobytes() for m in mask}) > 1  # the frames flag different pixels


# ---------------------------------------------------------------- 7. schedule and state
def _c2(W, H):
    from raymarcher_amd import Scene
    return Scene(path=os.path.join(SCENES, "lighting", "directional_light_2.json")).tables(W, H)


def test_timing_counts_one_launch_all_stage_1(renderer):
    L = lib()
    W, H = 64, 40
    scene = SB.menger_scene(W, H)
    s = abi.default_settings(mengerLevels=3)
    cams = orbit((2.6, 2.2, 3.0), (-2.6, -2.2, -3.0), 30.0, W, H, 3)
    try:
        assert L.rm_set_timing(1) == 0
        renderer.render_adaptive(tables_of(scene), s, W, H, cams, 2, 0.1, mask=True, counts=True)
        renderer.torch.cuda.synchronize(renderer.device)
        total, stages, n = C.c_double(), (C.c_double * 4)(), C.c_int()
        assert L.rm_get_stage_timing(C.byref(total), stages, C.byref(n)) == 0
        assert n.value == 1 and total.value > 0.0
        assert stages[0] == 0.0 and stages[1] == total.value and stages[2] == 0.0 and stages[3] == 0.0
    finally:
        L.rm_set_timing(0)


def test_adaptive_launch_leaves_the_single_frame_tuners_alone(renderer):
    L = lib()
    W, H = 512, 320
    t = _c2(W, H)
    s = abi.default_settings(enableSoftShadow=1, enableAmbientOcclusion=1)
    other = tables_of((orbit((0, 1, 8), (0, -0.1, -1), 40.0, W, H, 1)[0], t.objects, t.num_objects, t.lights, t.num_lights, t.globals_))
    cams = [other.camera, t.camera, other.camera]

    def sequence(adaptive_after=None):
        renderer.render(other, s, W, H)  # another picture of the same size: the picture below starts afresh
        splits, frames = [], []
        for k in range(12):
            if k == adaptive_after:
                renderer.render_adaptive(t, s, W, H, cams, 2, 0.1)  # the picture's own frame among them
                assert L.rm_debug_last_path() == 8 and L.rm_debug_last_split() == 0
            frames.append(renderer.render(t, s, W, H).clone())
            assert L.rm_debug_last_path() == 1
            splits.append(L.rm_debug_last_split())
        return splits, frames

    try:
        assert L.rm_debug_set_tile_shape(3) == 0  # no timed shape tuning: the sequence depends on the tile-order state alone
        assert L.rm_debug_set_light_split(32) == 0  # split a settled picture without measuring
        plain, frames = sequence()
        assert sequence()[0] == plain, "the sequence is not deterministic without an adaptive launch"
        assert plain[0] == 0 and plain[-1] > 0, plain  # it settles, then splits
        again, frames2 = sequence(adaptive_after=plain.index(plain[-1]) + 1)
        assert again == plain
        assert all(SB.ieq(a, frames[0]) for a in frames + frames2)
    finally:
        L.rm_debug_set_tile_shape(-1)
        L.rm_debug_set_light_split(-1)


_CHILD = r'''
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_adaptive as t
from raymarcher_amd import Renderer
r = Renderer(0)
for name in ("bulb_plain", "table_sec", "textures"):
    t.test_flagged_pixels_are_supersampled_the_rest_is_render_batch(r, name)
for ss, W, H in t.ODD:
    t.test_every_word_is_written_and_nothing_else(r, ss, W, H, 3)
for ss in (2, 4):
    t.test_frames_with_a_handful_of_flagged_pixels_each(r, ss)
print("ok")
'''


@pytest.mark.parametrize("wpb", [2, 4])
def test_wider_workgroups_render_the_same_frames(renderer, wpb):
    """RM_WAVES_PER_BLOCK (read once per process): the three steps with 2 and 4 waves per workgroup, in a fresh child process."""
    env = dict(os.environ, RM_WAVES_PER_BLOCK=str(wpb))
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]


def test_back_to_back_launches_on_one_stream(renderer):
    import torch
    W = H = 16
    ss = 2
    scene = h.scene_mandelbulb(W, H)
    s = abi.default_settings()
    cams_a = orbit((0, 0, 4.5), (0, 0, -1), 30.0, W, H, 300, deg=1.2)
    cams_b = orbit((0, 0.5, 4.2), (0, -0.1, -1), 35.0, W, H, 40, deg=9.0)
    globs_a = [with_globals(scene[5], iTime=0.01 * f) for f in range(300)]
    t = tables_of(scene)
    stream = torch.cuda.Stream(device=renderer.device)
    torch.cuda.synchronize(renderer.device)
    with torch.cuda.stream(stream):
        a = renderer.render_adaptive(t, s, W, H, cams_a, ss, 0.1, globals_=globs_a, mask=True, counts=True)
        b = renderer.render_adaptive(t, s, W, H, cams_b, ss, 0.1, mask=True, counts=True)
    stream.synchronize()
    for got, cams, globs, what in ((a, cams_a, globs_a, "first launch"), (b, cams_b, None, "second launch")):
        exp, _exp_b, exp_m = library_composite(renderer, t, s, W, H, cams, ss, 0.1, globs)[:3]
        assert_bit_equal(got[0].cpu().numpy(), exp, what)
        assert (got[1].cpu().numpy().astype(bool) == exp_m).all(), what
        assert (got[2].cpu().numpy() == exp_m.reshape(len(cams), -1).sum(axis=1)).all(), what
        assert exp_m.any() and not exp_m.all()


# ---------------------------------------------------------------- 8. errors on the device
def test_host_output_pointers_are_refused_and_hip_stays_clean(renderer):
    L = lib()
    torch = renderer.torch
    W, H = 16, 8
    scene = h.scene_mandelbulb(W, H)
    cams = (abi.RmCamera * 2)(scene[0], scene[0])
    host = np.zeros((2, H, W, 4), dtype=np.float32)
    hp = C.c_void_p(host.ctypes.data)
    dev = [torch.empty((2, H, W, 4), dtype=torch.float32, device=renderer.device) for _ in range(2)]
    dm = torch.empty((2, H, W), dtype=torch.uint8, device=renderer.device)
    dc = torch.empty((2,), dtype=torch.int32, device=renderer.device)
    good = [C.c_void_p(a.data_ptr()) for a in (dev[0], dev[1], dm, dc)]
    for ss in (1, 2, 4):
        for bad in range(4):
            ptrs = [hp if k == bad else good[k] for k in range(4)]
            st = L.rm_render_adaptive(cams, C.byref(scene[5]), 1, 2, scene[1], 1, scene[3], scene[4], C.byref(abi.default_settings()),
                                      None, W, H, ss, 0.1, ptrs[0], ptrs[1], ptrs[2], ptrs[3], None)
            assert st == abi.RM_ERR_INVALID_ARGUMENT, (ss, bad)
            assert "not device-accessible" in L.rm_last_error().decode()
    out = renderer.render_adaptive(tables_of(scene), abi.default_settings(), W, H, [scene[0]], 2, 0.1)  # a following render succeeds
    torch.cuda.synchronize(renderer.device)
    assert bool(torch.isfinite(out).all())


def test_a_missing_sampler_is_unsupported(renderer):
    W, H = 16, 16
    for name in ("night_sky", "sea_sky", "skybox_reflect", "area_light"):
        scene, s, _res = SB.resource_case(name, W, H)
        with pytest.raises(RaymarcherError) as e:
            renderer.render_adaptive(tables_of(scene), s, W, H, [scene[0]], 2, 0.1)
        assert e.value.status == abi.RM_ERR_UNSUPPORTED, name
    scene = h.scene_mandelbulb(W, H)
    t = tables_of(scene)
    assert_is_composite(renderer, t, abi.default_settings(), W, H, [scene[0]], 2, 0.1, what="the render after the refusals")


# ---------------------------------------------------------------- 9. render_sequence(..., supersample=2, adaptive=0.1)
def test_render_sequence_adaptive_equals_the_oracle_chain(renderer):
    W, H, N, ss, thr = 75, 45, 3, 2, 0.1
    scene = SB.reflect_refract_scene(W, H)
    for li in scene[3]:
        li.color[0] *= 2.5; li.color[1] *= 2.5; li.color[2] *= 2.5  # over-exposed: BrightColor is populated
    s = abi.default_settings(enableReflection=1)
    cams = orbit((0, 1.2, 5), (0, -0.2, -1), 40.0, W, H, N)
    globs = [with_globals(scene[5], iTime=0.25 * f) for f in range(N)]
    post = abi.RmPostSettings(**{"exposure": 1.0, **SB.POST_CASES["bloom_hdr_fxaa"]})
    assert post.enableBloom and post.enableHDR and post.enableFXAA
    imgs = renderer.render_sequence(tables_of(scene), s, W, H, cams, globals_=globs, post=post, supersample=ss, adaptive=thr)
    assert lib().rm_debug_last_path() == 8
    assert tuple(imgs.shape) == (N, H, W, 4) and imgs.dtype == renderer.torch.uint8
    imgs = imgs.cpu().numpy()
    for f in range(N):
        F, Fb = h.oracle_render((cams[f],) + tuple(scene[1:5]) + (globs[f],), s, W, H, bright=True, threads=16)
        assert np.isfinite(F).all() and np.isfinite(Fb).all()
        R, Rb = oracle_resolved(scene, cams[f], globs[f], s, W, H, ss)
        frag, bright, m = adaptive(F, Fb, R, Rb, thr)
        assert 0.05 < m.mean() < 0.95
        if f == 0:
            assert bright[..., :3].max() > 1.0
        ref = h.oracle_post(frag, bright, post)
        exp = (np.clip(ref[::-1], 0, 1) * np.float32(255.0) + np.float32(0.5)).astype(np.uint8)
        assert (imgs[f] == exp).all(), f"frame {f}: {(imgs[f] != exp).sum()} bytes differ"
    # without the keyword the call is what it was: supersample alone, and nothing at all
    full = renderer.render_sequence(tables_of(scene), s, W, H, cams, globals_=globs, post=post, supersample=ss)
    assert lib().rm_debug_last_path() == 7
    assert (full.cpu().numpy() != imgs).any()
    one = renderer.render_sequence(tables_of(scene), s, W, H, cams, globals_=globs, post=post)
    assert lib().rm_debug_last_path() == 6
    assert bool((one == renderer.render_sequence(tables_of(scene), s, W, H, cams, globals_=globs, post=post, supersample=1)).all())
