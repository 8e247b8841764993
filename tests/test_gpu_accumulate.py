"""rm_render_accumulated / Renderer.render_accumulated on the GPU.  An accumulated pixel is defined by things the contract already
has: the oracle's frames S_0 … S_{n−1} of the sub-frames' cameras and globals, added in index order in float32 and multiplied by
float32(1) / float32(n) — `accumulate` below is that definition in NumPy.  Every class the dispatcher has is compared with it on the
uint32 view, no tolerance and no excluded pixel, and a second time with the library's own render_batch frames reduced the same way,
so that a mismatch says which side moved.  Then n = 1 against render_batch, write coverage in guarded buffers, the schedule (path 9,
one timed launch, tuners untouched), a full-size frame, and render_sequence(..., accumulate=n) against the oracle's export chain."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import helpers as h
import scene_builders as SB
from helpers import assert_bit_equal, tables_of, with_globals
from raymarcher_amd import abi, lib
from raymarcher_amd.render import lens_cameras, shutter_globals

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(ROOT, "tests", "golden", "scenes")
SUBFRAMES = [1, 2, 3, 5, 8, 16]


def accumulate(S):
    """The definition: the n sub-frames (n, H, W, 4) float32 → (H, W, 4)."""
    S = np.ascontiguousarray(S, dtype=np.float32)
    n = S.shape[0]
    acc = S[0].copy()
    for j in range(1, n):
        acc = acc + S[j]
    out = acc * (np.float32(1) / np.float32(n))
    assert out.dtype == np.float32
    return out


def test_accumulate_is_the_sum_of_the_header():
    """The NumPy definition against the same sum written out per value with explicit binary32 roundings, denormals and −0 included."""
    rng = np.random.default_rng(9)
    f = np.float32
    for n in SUBFRAMES + [64]:
        S = (rng.standard_normal((n, 2, 3, 4)) * 10.0 ** rng.integers(-3, 4, (n, 2, 3, 4))).astype(f)
        S[:, 0, 0, 0] = f(1e-41) * rng.integers(-5, 6, n).astype(f)  # denormals stay denormals
        S[:, 0, 0, 1] = f(-0.0)                                     # the sum of −0 is −0
        got = accumulate(S)
        for idx in np.ndindex(2, 3, 4):
            acc = S[(0,) + idx]
            for j in range(1, n):
                acc = f(acc + S[(j,) + idx])
            exp = f(acc * f(f(1) / f(n)))
            assert got[idx].view(np.uint32) == exp.view(np.uint32), (n, idx)
        assert got[0, 0, 1].view(np.uint32) == f(-0.0).view(np.uint32)
        if n == 1:
            assert (got.view(np.uint32) == S[0].view(np.uint32)).all()  # n = 1: the frame itself


def camera_data(pos, look, up=(0, 1, 0), angle_deg=30.0):
    cd = abi.RmCameraData()
    for i in range(3):
        cd.pos[i], cd.look[i], cd.up[i] = pos[i], look[i], up[i]
    cd.pos[3], cd.look[3], cd.up[3] = 1.0, 0.0, 0.0
    cd.heightAngle = math.radians(angle_deg)
    return cd


def lens_frames(cd, W, H, radius, focus, n, frames, far=100.0, step=0.15):
    """frames·n cameras: frame f is the lens of `cd` moved by f·step along x (so the frames of a call differ)."""
    cams = []
    for f in range(frames):
        c = camera_data((cd.pos[0] + step * f, cd.pos[1], cd.pos[2]), tuple(cd.look[:3]), tuple(cd.up[:3]), math.degrees(cd.heightAngle))
        cams += lens_cameras(c, W, H, radius, focus, n, far=far)
    return cams


def oracle_accumulated(scene, cams, globs, s, W, H, n, rows=None, textures=None, **resources):
    """(fragColor, BrightColor) of every output frame by the definition: the oracle per sub-frame (its own camera and globals),
    asserted finite (NaN payloads could differ between NumPy and the GPU), then `accumulate`.  rows: (r0, r1) or the whole frame."""
    r0, r1 = rows if rows else (0, H)
    outs, brs = [], []
    for f in range(len(cams) // n):
        S, Sb = [], []
        for j in range(n):
            k = f * n + j
            g = globs[k] if isinstance(globs, (list, tuple)) else globs
            a, b = h.oracle_render((cams[k],) + tuple(scene[1:5]) + (g,), s, W, H, r0, r1, bright=True, threads=16, textures=textures, **resources)
            assert np.isfinite(a).all() and np.isfinite(b).all(), "the oracle's sub-frame is not finite: choose another camera"
            S.append(a)
            Sb.append(b)
        outs.append(accumulate(np.stack(S)))
        brs.append(accumulate(np.stack(Sb)))
    return outs, brs


def acc_vs_oracle(renderer, scene, s, W, H, cams, globs, n, bright=True, textures=None, what="", **resources):
    """One call against the definition twice: from the oracle's sub-frames, and from render_batch's."""
    t = tables_of(scene, **resources)
    if textures:
        t.textures = textures
    frames = len(cams) // n
    got = renderer.render_accumulated(t, s, W, H, cams, n, globals_=globs, bright=bright)
    assert lib().rm_debug_last_path() == 9 and lib().rm_debug_last_split() == 0
    out, br = (got if bright else (got, None))
    assert tuple(out.shape) == (frames, H, W, 4)
    out = out.cpu().numpy()
    br = br.cpu().numpy() if bright else None
    ref, ref_b = oracle_accumulated(scene, cams, globs, s, W, H, n, textures=textures, **resources)
    sub, sub_b = renderer.render_batch(t, s, W, H, cams, globals_=globs, bright=True)
    sub, sub_b = sub.cpu().numpy(), sub_b.cpu().numpy()
    for f in range(frames):
        tag = f"{what} n {n} {W}x{H} frame {f}"
        assert_bit_equal(out[f], ref[f], tag + " against the oracle")
        assert_bit_equal(out[f], accumulate(sub[f * n:(f + 1) * n]), tag + " against render_batch reduced")
        if bright:
            assert_bit_equal(br[f], ref_b[f], tag + " bright against the oracle")
            assert_bit_equal(br[f], accumulate(sub_b[f * n:(f + 1) * n]), tag + " bright against render_batch reduced")
    return out


# ---------------------------------------------------------------- 1. bit for bit against the oracle, every class of the dispatcher
@pytest.mark.parametrize("n", SUBFRAMES)
def test_plain_bulb_through_a_lens(renderer, n):
    """unit_mandelbulb, 12 iterations, lens samples; every n, 3 frames and 1, with and without d_bright, both frame sizes."""
    W, H = (97, 53) if n != 16 else (256, 256)
    scene = h.scene_mandelbulb(W, H)
    s = abi.default_settings(fractalIters=12)
    assert lib().rm_debug_bulb_plain(scene[1], 1, C.byref(scene[5])) == 1
    cd = camera_data((0, 0, 4.5), (0, 0, -4.5))
    frames = 3 if n <= 5 else 1
    out = acc_vs_oracle(renderer, scene, s, W, H, lens_frames(cd, W, H, 0.12, 3.6, n, frames), scene[5], n, bright=(n % 2 == 1),
                        what="plain bulb")
    if n > 1:  # the lens blurs: the picture is not the pinhole's
        pin = renderer.render_batch(tables_of(scene), s, W, H, lens_cameras(cd, W, H, 0.12, 3.6, 1)).cpu().numpy()
        assert np.abs(out[0] - pin[0]).max() > 0.02


@pytest.mark.parametrize("n", [2, 5])
def test_general_bulb_where_some_sub_frames_are_not_plain(renderer, n):
    W, H = 97, 53
    scene = h.scene_mandelbulb(W, H)
    cams = lens_frames(camera_data((0, 0, 4.5), (0, 0, -4.5)), W, H, 0.08, 3.6, n, 3)
    globs = [with_globals(scene[5], power=(8.0 if k % 2 == 0 else 7.5), iTime=0.3 * k) for k in range(3 * n)]  # one per sub-frame
    assert sorted({lib().rm_debug_bulb_plain(scene[1], 1, C.byref(g)) for g in globs}) == [0, 1]
    acc_vs_oracle(renderer, scene, abi.default_settings(), W, H, cams, globs, n, what="power 8 / 7.5 bulb")


def test_general_bulb_in_one_sub_frame_only(renderer):
    """The plain form needs every sub-frame of the CALL: one Julia seed in the last sub-frame of the last frame switches all."""
    W, H, n = 64, 40, 3
    scene = h.scene_mandelbulb(W, H)
    cams = lens_frames(camera_data((0, 0, 4.5), (0, 0, -4.5)), W, H, 0.08, 3.6, n, 2)
    globs = [with_globals(scene[5]) for _ in range(2 * n)]
    globs[-1] = with_globals(scene[5], julia=(0.3, -0.2))
    acc_vs_oracle(renderer, scene, abi.default_settings(fractalIters=10), W, H, cams, globs, n, what="one Julia sub-frame")


@pytest.mark.parametrize("n,frames", [(3, 3), (16, 1)])
def test_depth_of_field_scenefile_with_its_own_lens(renderer, n, frames):
    """scenefiles/lighting/depth_of_field.json through the loader: ten textured cubes in two rows receding from the camera, the
    file's aperture and focalLength as the lens.  The table walk with object textures; with reflection on, its secondary rays."""
    from raymarcher_amd import Scene
    W, H = 97, 53
    sc = Scene(path=os.path.join(SCENES, "lighting", "depth_of_field.json"))
    t = sc.tables(W, H)
    radius, focus = sc.lens()
    assert (np.float32(radius), np.float32(focus)) == (np.float32(0.008), np.float32(3.0))
    scene = SB.scene_tuple(t)
    cams = lens_frames(sc.camera_data(), W, H, radius, focus, n, frames, step=0.4)
    for s in (abi.default_settings(), abi.default_settings(enableReflection=1, enableSoftShadow=1)):
        acc_vs_oracle(renderer, scene, s, W, H, cams, t.globals_, n, textures=t.textures, what="depth_of_field.json")


@pytest.mark.parametrize("n", [2, 8])
def test_primitive_table_walk_and_its_secondary_rays(renderer, n):
    """The plain table walk (soft shadows + AO), then the same table with reflection and refraction, two bounces (SEC)."""
    W, H = 97, 53
    scene = SB.reflect_refract_scene(W, H)
    cd = camera_data((0, 1.2, 5), (0, -0.2, -1), angle_deg=40.0)
    frames = 3 if n == 2 else 1
    cams = lens_frames(cd, W, H, 0.1, 5.0, n, frames)
    acc_vs_oracle(renderer, scene, abi.default_settings(enableSoftShadow=1, enableAmbientOcclusion=1), W, H, cams, scene[5], n,
                  what="primitives soft+AO")
    globs = [with_globals(scene[5], iTime=0.25 * k) for k in range(frames * n)]
    acc_vs_oracle(renderer, scene, abi.default_settings(enableReflection=1, enableRefraction=1, numReflection=2), W, H, cams, globs, n,
                  bright=False, what="reflection+refraction")


def test_textures_sky_box_and_area_light(renderer):
    W, H, n = 97, 53, 3
    scene = SB.textured_scene(W, H)
    s = abi.default_settings(features=abi.RM_FEAT_WHITE_BACKGROUND, enableSoftShadow=1, enableSkyBox=1)
    cams = lens_frames(camera_data((0.4, 2.2, 5.5), (-0.05, -0.35, -1), angle_deg=42.0), W, H, 0.15, 5.5, n, 2)
    acc_vs_oracle(renderer, scene, s, W, H, cams, scene[5], n, textures=SB.synthetic_textures(), what="textured + sky box",
                  skybox=SB.synthetic_skybox())
    scene, s, res = SB.resource_case("area_light", W, H)
    cams = lens_frames(camera_data((0, 1.6, 5.5), (0, -0.2, -1), angle_deg=45.0), W, H, 0.1, 5.0, 5, 1)
    acc_vs_oracle(renderer, scene, s, W, H, cams, scene[5], 5, what="area light", **res)


@pytest.mark.parametrize("n", [3, 8])
def test_terrain_and_clouds_through_a_shutter(renderer, n):
    """ENV: the layers move with iTime; one camera, the shutter open for 2 s per frame, frames 4 s apart."""
    W, H = 97, 53
    scene = SB.env_scene(W, H)
    frames = 2
    cam = h.make_camera((0, 500, 5), (0.3, 0.12, -1), (0, 1, 0), 70.0, W, H, far=2000.0)
    cams = [cam] * (frames * n)
    globs = [g for f in range(frames) for g in shutter_globals(scene[5], 4.0 * f, 4.0 * f + 2.0, n)]
    assert len({g.iTime for g in globs}) == frames * n
    out = acc_vs_oracle(renderer, scene, abi.default_settings(features=SB.ENV_ALL, enableReflection=1), W, H, cams, globs, n,
                        what="terrain+cloud shutter")
    assert np.abs(out[0] - out[1]).max() > 1e-3  # time moves the picture


def test_sea_and_night_sky_through_a_shutter(renderer):
    W, H, n = 64, 40, 5
    scene, s, res = SB.resource_case("sea_sky", W, H)
    cams = [h.make_camera((0, 3.5, 6), (0, -0.35, -1), (0, 1, 0), 50.0, W, H)] * n
    acc_vs_oracle(renderer, scene, s, W, H, cams, shutter_globals(scene[5], 0.7, 1.6, n), n, what="sea + sky shutter", **res)


@pytest.mark.parametrize("n", [2, 5])
def test_menger_sponge_motion_blur(renderer, n):
    """The sponge's animation advances with iTime (its uniforms are computed on the device per scene block): motion blur.  A path-5
    request does not reach this entry point."""
    L = lib()
    W, H = 97, 53
    scene = SB.menger_scene(W, H)
    frames = 3 if n == 2 else 1
    cams = [h.make_camera((2.6, 2.2, 3.0), (-2.6, -2.2, -3.0), (0, 1, 0), 30.0, W, H)] * (frames * n)
    # the sponge opens while −cos(iTime / 2) crosses ±0.2 (frag:1052): iTime from 2.74 to 3.54
    globs = [g for f in range(frames) for g in shutter_globals(scene[5], 2.7 + 0.2 * f, 3.4 + 0.2 * f, n)]
    s = abi.default_settings(mengerLevels=4, enableReflection=1, numReflection=1)
    plain = acc_vs_oracle(renderer, scene, s, W, H, cams, globs, n, what="menger shutter")
    sharp = renderer.render_batch(tables_of(scene), s, W, H, cams[:1], globals_=globs[:1]).cpu().numpy()
    assert np.abs(plain[0] - sharp[0]).max() > 1e-3
    try:
        assert L.rm_set_kernel_path(5) == 0
        forced = renderer.render_accumulated(tables_of(scene), s, W, H, cams, n, globals_=globs)
        assert L.rm_debug_last_path() == 9
        assert_bit_equal(forced.cpu().numpy(), plain, "menger with and without the path request")
    finally:
        L.rm_set_kernel_path(0)


# ---------------------------------------------------------------- 2. globals: one for all, or one per sub-frame
def test_one_globals_equals_the_same_globals_per_sub_frame(renderer):
    W, H, n, frames = 64, 40, 3, 3
    scene = SB.reflect_refract_scene(W, H)
    s = abi.default_settings(enableReflection=1)
    cams = lens_frames(camera_data((0, 1.2, 5), (0, -0.2, -1), angle_deg=40.0), W, H, 0.1, 5.0, n, frames)
    one = renderer.render_accumulated(tables_of(scene), s, W, H, cams, n, globals_=scene[5])
    per = renderer.render_accumulated(tables_of(scene), s, W, H, cams, n, globals_=[with_globals(scene[5]) for _ in cams])
    assert SB.ieq(one, per)
    none = renderer.render_accumulated(tables_of(scene), s, W, H, cams, n)  # tables.globals_
    assert SB.ieq(one, none)


# ---------------------------------------------------------------- 3. n = 1 is render_batch
def test_one_sub_frame_is_render_batch(renderer):
    W, H = 77, 45
    for scene, s in ((SB.reflect_refract_scene(W, H), abi.default_settings(enableReflection=1)),
                     (h.scene_mandelbulb(W, H), abi.default_settings(fractalIters=12))):
        cams = lens_frames(camera_data((0, 1.2, 5), (0, -0.2, -1), angle_deg=40.0), W, H, 0.0, 5.0, 1, 3, step=0.3)
        globs = [with_globals(scene[5], iTime=0.25 * f) for f in range(3)]
        a, ab = renderer.render_accumulated(tables_of(scene), s, W, H, cams, 1, globals_=globs, bright=True)
        assert lib().rm_debug_last_path() == 9
        b, bb = renderer.render_batch(tables_of(scene), s, W, H, cams, globals_=globs, bright=True)
        assert SB.ieq(a, b) and SB.ieq(ab, bb)


def test_two_equal_sub_frames_are_the_frame(renderer):
    """Twice the same camera: v + v and · 0.5 are both exact, so the mean of two equal frames is the frame, bit for bit."""
    W, H = 45, 27
    scene = h.scene_mandelbulb(W, H)
    s = abi.default_settings(fractalIters=12)
    one, one_b = renderer.render(tables_of(scene), s, W, H, bright=True)
    out, br = renderer.render_accumulated(tables_of(scene), s, W, H, [scene[0]] * 6, 2, bright=True)
    for f in range(3):
        assert SB.ieq(out[f], one) and SB.ieq(br[f], one_b), f


# ---------------------------------------------------------------- 4. write coverage
@pytest.mark.parametrize("W,H", [(97, 53), (1, 1), (3, 70), (65, 9), (256, 256)])
@pytest.mark.parametrize("frames", [1, 3])
def test_every_word_is_written_and_nothing_else(renderer, W, H, frames):
    n = 3
    for scene, s in ((h.scene_mandelbulb(W, H), abi.default_settings(fractalIters=12)),
                     (SB.reflect_refract_scene(W, H), abi.default_settings(enableReflection=1, enableRefraction=1, numReflection=2))):
        t = tables_of(scene)
        cams = [scene[0]] * (frames * n)
        out, c1 = h.guarded((frames, H, W, 4), device=renderer.device)
        br, c2 = h.guarded((frames, H, W, 4), device=renderer.device)
        renderer.render_accumulated(t, s, W, H, cams, n, out=out, out_bright=br)
        c1()
        c2()
        # d_bright = NULL: the same frames, and a neighbouring poisoned allocation is left alone
        out2, c3 = h.guarded((frames, H, W, 4), device=renderer.device)
        spare = h.Guarded((frames, H, W, 4), renderer.torch.float32, h.FLOAT_POISON, renderer.device)
        renderer.render_accumulated(t, s, W, H, cams, n, out=out2)
        c3()
        assert SB.ieq(out2, out)
        assert bool(spare._unwritten(spare.buf).all()), "a launch without d_bright wrote outside d_rgba"
        for f in range(1, frames):
            assert SB.ieq(out[f], out[0]) and SB.ieq(br[f], br[0])


# ---------------------------------------------------------------- 5. schedule and state
def test_timing_counts_one_launch_all_stage_1(renderer):
    L = lib()
    W, H, n = 64, 40, 4
    scene = SB.menger_scene(W, H)
    s = abi.default_settings(mengerLevels=3)
    cams = [scene[0]] * (3 * n)
    try:
        assert L.rm_set_timing(1) == 0
        renderer.render_accumulated(tables_of(scene), s, W, H, cams, n, globals_=shutter_globals(scene[5], 0.0, 1.0, 3 * n))
        renderer.torch.cuda.synchronize(renderer.device)
        total, stages, k = C.c_double(), (C.c_double * 4)(), C.c_int()
        assert L.rm_get_stage_timing(C.byref(total), stages, C.byref(k)) == 0
        assert k.value == 1 and total.value > 0.0
        assert stages[0] == 0.0 and stages[1] == total.value and stages[2] == 0.0 and stages[3] == 0.0
    finally:
        L.rm_set_timing(0)


def test_accumulated_launch_leaves_the_single_frame_tuners_alone(renderer):
    """The sequence of test_gpu_supersample, with an accumulated launch of the same picture in the middle."""
    from raymarcher_amd import Scene
    L = lib()
    W, H = 512, 320
    t = Scene(path=os.path.join(SCENES, "lighting", "directional_light_2.json")).tables(W, H)
    s = abi.default_settings(enableSoftShadow=1, enableAmbientOcclusion=1)
    other = tables_of((h.make_camera((0, 1, 8), (0, -0.1, -1), (0, 1, 0), 40.0, W, H), t.objects, t.num_objects, t.lights, t.num_lights,
                       t.globals_))

    def sequence(acc_after=None):
        renderer.render(other, s, W, H)  # another picture of the same size: the picture below starts afresh
        splits, frames = [], []
        for k in range(12):
            if k == acc_after:
                renderer.render_accumulated(t, s, W, H, [other.camera, t.camera, t.camera, other.camera], 2)
                assert L.rm_debug_last_path() == 9 and L.rm_debug_last_split() == 0
            frames.append(renderer.render(t, s, W, H).clone())
            assert L.rm_debug_last_path() == 1
            splits.append(L.rm_debug_last_split())
        return splits, frames

    try:
        assert L.rm_debug_set_tile_shape(3) == 0  # no timed shape tuning: the sequence depends on the tile-order state alone
        assert L.rm_debug_set_light_split(32) == 0  # split a settled picture without measuring
        plain, frames = sequence()
        assert plain[0] == 0 and plain[-1] > 0, plain  # it settles, then splits
        again, frames2 = sequence(acc_after=plain.index(plain[-1]) + 1)
        assert again == plain
        assert all(SB.ieq(a, frames[0]) for a in frames + frames2)
    finally:
        L.rm_debug_set_tile_shape(-1)
        L.rm_debug_set_light_split(-1)


def test_back_to_back_launches_on_one_stream(renderer):
    """Two calls in flight on one stream, the first filling the ring's cap of scene blocks: staging of the second does not disturb it."""
    import torch
    W = H = 16
    n = 4
    scene = h.scene_mandelbulb(W, H)
    s = abi.default_settings()
    cd = camera_data((0, 0, 4.5), (0, 0, -4.5))
    cams_a = lens_frames(cd, W, H, 0.1, 3.6, n, abi.RM_MAX_BATCH_FRAMES // n, step=0.002)
    cams_b = lens_frames(cd, W, H, 0.3, 3.0, n, 10, step=0.05)
    globs_a = [with_globals(scene[5], iTime=0.01 * k) for k in range(len(cams_a))]
    t = tables_of(scene)
    stream = torch.cuda.Stream(device=renderer.device)
    torch.cuda.synchronize(renderer.device)
    with torch.cuda.stream(stream):
        a = renderer.render_accumulated(t, s, W, H, cams_a, n, globals_=globs_a)
        b = renderer.render_accumulated(t, s, W, H, cams_b, n)
    stream.synchronize()
    Sa = renderer.render_batch(t, s, W, H, cams_a, globals_=globs_a).cpu().numpy()
    Sb = renderer.render_batch(t, s, W, H, cams_b).cpu().numpy()
    assert np.isfinite(Sa).all() and np.isfinite(Sb).all()
    a, b = a.cpu().numpy(), b.cpu().numpy()
    for f in range(a.shape[0]):
        assert_bit_equal(a[f], accumulate(Sa[f * n:(f + 1) * n]), f"first launch, frame {f}")
    for f in range(b.shape[0]):
        assert_bit_equal(b[f], accumulate(Sb[f * n:(f + 1) * n]), f"second launch, frame {f}")
    assert np.abs(a[0] - a[-1]).max() > 0.02


def test_host_output_pointer_is_refused_and_hip_stays_clean(renderer):
    L = lib()
    W, H = 16, 8
    scene = h.scene_mandelbulb(W, H)
    cams = (abi.RmCamera * 4)(*[scene[0]] * 4)
    host = np.zeros((2, H, W, 4), dtype=np.float32)
    st = L.rm_render_accumulated(cams, C.byref(scene[5]), 1, 2, 2, scene[1], 1, scene[3], scene[4], C.byref(abi.default_settings()),
                                 None, W, H, C.c_void_p(host.ctypes.data), None, None)
    assert st == abi.RM_ERR_INVALID_ARGUMENT and "not device-accessible" in L.rm_last_error().decode()
    out = renderer.render_accumulated(tables_of(scene), abi.default_settings(), W, H, [scene[0]] * 4, 2)  # a following render succeeds
    renderer.torch.cuda.synchronize(renderer.device)
    assert bool(renderer.torch.isfinite(out).all())


# ---------------------------------------------------------------- 6. full size
def test_full_size_1080p_depth_of_field_16_lens_samples(renderer):
    """1920×1080, depth_of_field.json, n = 16, lens three times the file's so that the blur spans pixels: seeded bands of rows against
    the oracle's sub-frames (the CPU time stays bounded), the whole frame against render_batch reduced."""
    from raymarcher_amd import Scene
    W, H, n = 1920, 1080, 16
    sc = Scene(path=os.path.join(SCENES, "lighting", "depth_of_field.json"))
    t = sc.tables(W, H)
    radius, focus = sc.lens()
    cams = lens_cameras(sc.camera_data(), W, H, 3.0 * radius, focus, n)
    s = abi.default_settings(enableReflection=1)
    out, br = renderer.render_accumulated(t, s, W, H, cams, n, bright=True)
    assert lib().rm_debug_last_path() == 9
    out, br = out.cpu().numpy(), br.cpu().numpy()
    sub, sub_b = renderer.render_batch(t, s, W, H, cams, bright=True)
    assert_bit_equal(out[0], accumulate(sub.cpu().numpy()), "1080p depth of field against render_batch reduced")
    assert_bit_equal(br[0], accumulate(sub_b.cpu().numpy()), "1080p depth of field bright against render_batch reduced")
    rng = np.random.default_rng(20261017)
    for r0 in sorted(int(r) for r in rng.integers(0, H - 4, 3)):
        ref, ref_b = oracle_accumulated(SB.scene_tuple(t), cams, t.globals_, s, W, H, n, rows=(r0, r0 + 4), textures=t.textures)
        assert_bit_equal(out[0][r0:r0 + 4], ref[0], f"1080p depth of field rows {r0}..{r0 + 4}")
        assert_bit_equal(br[0][r0:r0 + 4], ref_b[0], f"1080p depth of field bright rows {r0}..{r0 + 4}")
    pin = sub[0].cpu().numpy()
    assert (np.abs(out[0] - pin).max(-1) > 1e-3).mean() > 0.01  # the lens blurs what is out of focus


# ---------------------------------------------------------------- 7. render_sequence(..., accumulate=n)
def test_render_sequence_accumulated_equals_the_oracle_chain(renderer):
    W, H, N, n = 75, 45, 2, 3
    scene = SB.reflect_refract_scene(W, H)
    for li in scene[3]:
        li.color[0] *= 2.5; li.color[1] *= 2.5; li.color[2] *= 2.5  # over-exposed: BrightColor is populated
    s = abi.default_settings(enableReflection=1)
    cams = lens_frames(camera_data((0, 1.2, 5), (0, -0.2, -1), angle_deg=40.0), W, H, 0.1, 5.0, n, N)
    globs = [g for f in range(N) for g in shutter_globals(scene[5], 0.25 * f, 0.25 * f + 0.1, n)]
    post = abi.RmPostSettings(**{"exposure": 1.0, **SB.POST_CASES["bloom_hdr_fxaa"]})
    imgs = renderer.render_sequence(tables_of(scene), s, W, H, cams, globals_=globs, post=post, accumulate=n)
    assert lib().rm_debug_last_path() == 9
    assert tuple(imgs.shape) == (N, H, W, 4) and imgs.dtype == renderer.torch.uint8
    imgs = imgs.cpu().numpy()
    frag, bright = oracle_accumulated(scene, cams, globs, s, W, H, n)
    assert bright[0][..., :3].max() > 1.0
    for f in range(N):
        ref = h.oracle_post(frag[f], bright[f], post)
        exp = (np.clip(ref[::-1], 0, 1) * np.float32(255.0) + np.float32(0.5)).astype(np.uint8)
        assert (imgs[f] == exp).all(), f"frame {f}: {(imgs[f] != exp).sum()} bytes differ"
    # without the keyword the call is what it was: one image per camera
    bare = renderer.render_sequence(tables_of(scene), s, W, H, cams, globals_=globs, post=post)
    assert lib().rm_debug_last_path() == 6 and tuple(bare.shape) == (N * n, H, W, 4)
