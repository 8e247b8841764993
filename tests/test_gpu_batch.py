"""rm_render_batch / Renderer.render_batch on the GPU: every frame of a batch — its own camera on a short orbit, its own globals —
bit for bit against the oracle and against rm_render of the same camera and globals, for every kernel class the batch dispatches;
the one-launch schedule (rm_debug_last_path 6) and the per-frame fallback of wavefront frames (5); back-to-back batches on one
stream (staging memory still in flight); the single-frame tuners undisturbed by a batch; device-pointer errors."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import helpers as h
import scene_builders as SB
from helpers import assert_bit_equal, tables_of, with_globals
from scene_builders import orbit
from raymarcher_amd import abi, lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(ROOT, "tests", "golden", "scenes")


def batch_vs_oracle(renderer, scene, s, W, H, cams, globs, textures=None, what="", **resources):
    t = tables_of(scene, **resources)
    if textures:
        t.textures = textures
    out, br = renderer.render_batch(t, s, W, H, cams, globals_=globs, bright=True)
    assert tuple(out.shape) == (len(cams), H, W, 4)
    assert lib().rm_debug_last_path() == 6
    out, br = out.cpu().numpy(), br.cpu().numpy()
    for f, cam in enumerate(cams):
        g = globs[f] if isinstance(globs, (list, tuple)) else globs
        ref, ref_b = h.oracle_render((cam,) + tuple(scene[1:5]) + (g,), s, W, H, bright=True, textures=textures, **resources)
        assert_bit_equal(out[f], ref, f"{what} frame {f}")
        assert_bit_equal(br[f], ref_b, f"{what} frame {f} bright")
    return out


# ---------------------------------------------------------------- 1. against the oracle, every class the batch dispatches
def test_bulb_plain_form(renderer):
    W, H = 96, 64
    scene = h.scene_mandelbulb(W, H)
    cams = orbit((0, 0, 4.5), (0, 0, -1), 30.0, W, H, 4, deg=7.0)
    globs = [with_globals(scene[5], iTime=0.5 * f) for f in range(4)]
    assert all(lib().rm_debug_bulb_plain(scene[1], 1, C.byref(g)) == 1 for g in globs)
    out = batch_vs_oracle(renderer, scene, abi.default_settings(fractalIters=12), W, H, cams, globs, what="plain bulb")
    assert np.abs(out[0] - out[3]).max() > 0.05  # the frames differ


def test_bulb_frames_that_disagree_on_the_plain_form(renderer):
    W, H = 80, 64
    scene = h.scene_mandelbulb(W, H)
    cams = orbit((0, 0, 4.5), (0, 0, -1), 30.0, W, H, 4, deg=5.0)
    globs = [with_globals(scene[5], power=(8.0 if f % 2 == 0 else 7.5), iTime=0.3 * f) for f in range(4)]
    assert [lib().rm_debug_bulb_plain(scene[1], 1, C.byref(g)) for g in globs] == [1, 0, 1, 0]
    batch_vs_oracle(renderer, scene, abi.default_settings(), W, H, cams, globs, what="power 8 / 7.5 bulb")


def test_primitives_two_lights_soft_shadows_ao(renderer):
    W, H = 128, 80
    scene = SB.reflect_refract_scene(W, H)  # reflection / refraction off below: the plain table walk, c2's class
    cams = orbit((0, 1.2, 5), (0, -0.2, -1), 40.0, W, H, 5, deg=6.0)
    globs = [with_globals(scene[5], iTime=0.25 * f) for f in range(5)]
    batch_vs_oracle(renderer, scene, abi.default_settings(enableSoftShadow=1, enableAmbientOcclusion=1), W, H, cams, globs,
                    what="primitives soft+AO")


def test_reflection_and_refraction(renderer):
    W, H = 112, 72
    scene = SB.reflect_refract_scene(W, H)
    cams = orbit((0, 1.2, 5), (0, -0.2, -1), 40.0, W, H, 3, deg=8.0)
    s = abi.default_settings(enableReflection=1, enableRefraction=1, numReflection=2)
    batch_vs_oracle(renderer, scene, s, W, H, cams, scene[5], what="reflection+refraction")


def test_textures_and_sky_box(renderer):
    W, H = 112, 72
    scene = SB.textured_scene(W, H)
    cams = orbit((0.4, 2.2, 5.5), (-0.05, -0.35, -1), 42.0, W, H, 3, deg=6.0)
    batch_vs_oracle(renderer, scene, abi.default_settings(enableSoftShadow=1), W, H, cams, scene[5], textures=SB.synthetic_textures(),
                    what="textured")
    scene = SB.reflect_refract_scene(W, H)
    s = abi.default_settings(features=abi.RM_FEAT_WHITE_BACKGROUND, enableSkyBox=1, enableReflection=1, enableRefraction=1)
    batch_vs_oracle(renderer, scene, s, W, H, orbit((0, 1.2, 5), (0, -0.2, -1), 40.0, W, H, 3, deg=9.0), scene[5],
                    what="sky box", skybox=SB.synthetic_skybox())


def test_terrain_and_clouds_with_advancing_time(renderer):
    W, H = 96, 54
    scene = SB.env_scene(W, H)
    cams = orbit((0, 500, 5), (0.3, 0.12, -1), 70.0, W, H, 4, deg=3.0, far=2000.0)
    globs = [with_globals(scene[5], iTime=4.0 * f) for f in range(4)]
    out = batch_vs_oracle(renderer, scene, abi.default_settings(features=SB.ENV_ALL, enableReflection=1), W, H, cams, globs,
                          what="terrain+cloud")
    # sky + textures together (the ENV × TEX kernel)
    scene = SB.reflect_refract_scene(W, H)
    s = abi.default_settings(features=SB.ENV_ALL, enableSkyBox=1)
    batch_vs_oracle(renderer, scene, s, W, H, orbit((0, 1.2, 5), (0, -0.2, -1), 40.0, W, H, 3, deg=9.0), globs[:3],
                    what="env+skybox", skybox=SB.synthetic_skybox())
    assert np.isfinite(out).all()


def test_menger_sponge_with_advancing_time(renderer):
    W, H = 96, 72
    scene = SB.menger_scene(W, H)
    cams = orbit((2.6, 2.2, 3.0), (-2.6, -2.2, -3.0), 30.0, W, H, 4, deg=5.0)
    globs = [with_globals(scene[5], iTime=3.7 * f) for f in range(4)]  # ani / off of sdMengerSponge move with iTime
    s = abi.default_settings(mengerLevels=4, enableReflection=1, numReflection=1)
    out = batch_vs_oracle(renderer, scene, s, W, H, cams, globs, what="menger")
    same_cam = [cams[0]] * 2
    two = renderer.render_batch(tables_of(scene), s, W, H, same_cam, globals_=globs[:2]).cpu().numpy()
    assert_bit_equal(two[0], out[0], "menger frame 0 again")
    assert np.abs(two[1] - two[0]).max() > 1e-3  # the time alone changes the sponge


def test_two_d_frames_mixed_with_three_d_frames(renderer):
    W, H = 96, 64
    scene = h.scene_mandelbulb(W, H)
    cams = orbit((0, 0, 4.5), (0, 0, -1), 30.0, W, H, 4, deg=6.0)
    globs = [with_globals(scene[5], isTwoD=f % 2, iTime=1.5 * f) for f in range(4)]
    out = batch_vs_oracle(renderer, scene, abi.default_settings(), W, H, cams, globs, what="2-D / 3-D")
    assert np.abs(out[0] - out[1]).max() > 0.05


# ---------------------------------------------------------------- 2. against rm_render, with the single-frame schedules engaged
def _c2(W, H):
    from raymarcher_amd import Scene
    return Scene(path=os.path.join(SCENES, "lighting", "directional_light_2.json")).tables(W, H)


def test_each_frame_equals_rm_render_including_bright(renderer):
    W, H = 512, 320  # 2560 8×8 tiles: single frames take the tile-order and tile-shape paths
    t = _c2(W, H)
    s = abi.default_settings(enableSoftShadow=1, enableAmbientOcclusion=1)
    from raymarcher_amd import Scene
    data = Scene(path=os.path.join(SCENES, "lighting", "directional_light_2.json")).camera_data()
    pos, look = tuple(data.pos[:3]), tuple(data.look[:3])
    cams = orbit(pos, look, math.degrees(data.heightAngle), W, H, 4, deg=2.0)  # the scenefile's own view, turned
    globs = [with_globals(t.globals_, iTime=0.5 * f) for f in range(4)]
    out, br = renderer.render_batch(t, s, W, H, cams, globals_=globs, bright=True)
    out, br = out.clone(), br.clone()
    assert lib().rm_debug_last_path() == 6
    for f in range(4):
        tf = tables_of((cams[f], t.objects, t.num_objects, t.lights, t.num_lights, globs[f]))
        for _ in range(3):  # a new picture, then repeats of it (cost-ordered tiles)
            o1, b1 = h.render_guarded(renderer, tf, s, W, H, bright=True)
            assert SB.ieq(o1, out[f]) and SB.ieq(b1, br[f]), f"frame {f}"
    # numGlobals = 1 equals N identical explicit entries
    one = renderer.render_batch(t, s, W, H, cams, globals_=globs[0]).clone()
    many = renderer.render_batch(t, s, W, H, cams, globals_=[globs[0]] * 4)
    assert SB.ieq(one, many)
    assert SB.ieq(one[0], out[0])


# ---------------------------------------------------------------- 3. launch and fallback
def test_wavefront_frames_are_rendered_one_by_one(renderer):
    W = H = 2048  # 2^22 pixels with two reflection bounces: the single-frame launcher takes the wavefront pipeline
    scene = SB.menger_scene(W, H)
    s = abi.default_settings(mengerLevels=4, enableReflection=1, numReflection=2)
    cams = orbit((2.6, 2.2, 3.0), (-2.6, -2.2, -3.0), 30.0, W, H, 2, deg=10.0)
    globs = [with_globals(scene[5], iTime=2.0 * f) for f in range(2)]
    out = renderer.render_batch(tables_of(scene), s, W, H, cams, globals_=globs).clone()
    assert lib().rm_debug_last_path() == 5
    for f in range(2):
        single = renderer.render(tables_of((cams[f],) + tuple(scene[1:5]) + (globs[f],)), s, W, H)
        assert lib().rm_debug_last_path() == 5
        assert SB.ieq(single, out[f]), f"frame {f}"
    small = renderer.render_batch(tables_of(scene), s, 64, 48, orbit((2.6, 2.2, 3.0), (-2.6, -2.2, -3.0), 30.0, 64, 48, 2), scene[5])
    assert lib().rm_debug_last_path() == 6 and small.shape[0] == 2


# ---------------------------------------------------------------- 4. staging: back-to-back batches on one stream
def test_back_to_back_batches_on_one_stream(renderer):
    import torch
    W = H = 32
    scene = h.scene_mandelbulb(W, H)
    s = abi.default_settings()
    cams_a = orbit((0, 0, 4.5), (0, 0, -1), 30.0, W, H, 300, deg=1.2)
    cams_b = orbit((0, 0.5, 4.2), (0, -0.1, -1), 35.0, W, H, 40, deg=9.0)
    globs_a = [with_globals(scene[5], iTime=0.01 * f) for f in range(300)]
    t = tables_of(scene)
    stream = torch.cuda.Stream(device=renderer.device)
    torch.cuda.synchronize(renderer.device)
    with torch.cuda.stream(stream):
        a = renderer.render_batch(t, s, W, H, cams_a, globals_=globs_a)
        b = renderer.render_batch(t, s, W, H, cams_b)
    stream.synchronize()
    for f in range(300):
        tf = tables_of((cams_a[f],) + tuple(scene[1:5]) + (globs_a[f],))
        assert SB.ieq(renderer.render(tf, s, W, H), a[f]), f"first batch, frame {f}"
    for f in range(40):
        assert SB.ieq(renderer.render(tables_of((cams_b[f],) + tuple(scene[1:])), s, W, H), b[f]), f"second batch, frame {f}"


# ---------------------------------------------------------------- 5. the single-frame tuners are not disturbed
def test_batch_leaves_the_single_frame_tuners_alone(renderer):
    L = lib()
    W, H = 512, 320
    t = _c2(W, H)
    s = abi.default_settings(enableSoftShadow=1, enableAmbientOcclusion=1)
    other = tables_of((orbit((0, 1, 8), (0, -0.1, -1), 40.0, W, H, 1)[0], t.objects, t.num_objects, t.lights, t.num_lights, t.globals_))
    cams = [other.camera, t.camera, other.camera]

    def sequence(batch_after=None):
        renderer.render(other, s, W, H)  # another picture of the same size: the picture below starts afresh
        splits = []
        for k in range(12):
            if k == batch_after:
                renderer.render_batch(t, s, W, H, cams)
                assert L.rm_debug_last_path() == 6
            renderer.render(t, s, W, H)
            splits.append(L.rm_debug_last_split())
        return splits

    try:
        assert L.rm_debug_set_tile_shape(3) == 0  # no timed shape tuning: the sequence depends on the tile-order state alone
        assert L.rm_debug_set_light_split(32) == 0  # split a settled picture without measuring
        plain = sequence()
        assert sequence() == plain, "the sequence is not deterministic without a batch"
        assert plain[0] == 0 and plain[-1] > 0, plain  # it settles, then splits
        assert sequence(batch_after=plain.index(plain[-1]) + 1) == plain
    finally:
        L.rm_debug_set_tile_shape(-1)
        L.rm_debug_set_light_split(-1)


# ---------------------------------------------------------------- 6. device-pointer errors
def test_host_output_pointer_is_refused(renderer):
    L = lib()
    W, H = 16, 8
    scene = h.scene_mandelbulb(W, H)
    cams = (abi.RmCamera * 2)(scene[0], scene[0])
    host = np.zeros((2, H, W, 4), dtype=np.float32)
    st = L.rm_render_batch(cams, C.byref(scene[5]), 1, 2, scene[1], 1, scene[3], scene[4], C.byref(abi.default_settings()), None,
                           W, H, C.c_void_p(host.ctypes.data), None, None)
    assert st == abi.RM_ERR_INVALID_ARGUMENT
    assert "not device-accessible" in L.rm_last_error().decode()
    ref = h.scene_mandelbulb(W, H)
    assert L.rm_render(C.byref(ref[0]), ref[1], 1, ref[3], ref[4], C.byref(ref[5]), C.byref(abi.default_settings()), W, H, 0, H,
                       C.c_void_p(host.ctypes.data), None, None) == abi.RM_ERR_INVALID_ARGUMENT
