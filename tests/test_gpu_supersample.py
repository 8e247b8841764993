"""rm_render_supersampled / Renderer.render_supersampled on the GPU.  A supersampled pixel is defined by things the contract already
has: the oracle's frame S at ss·W × ss·H of the same camera, reduced by the fixed float32 tree of include/raymarcher_amd.h (x pairs,
then y pairs, once for ss = 2 and twice for ss = 4, then · 1 / ss²) — `resolve` below is that definition in NumPy.  Every class the
dispatcher has is compared with it on the uint32 view, no tolerance and no excluded pixel; then the launch is compared with the
library's own rm_render_res reduced on the host, with frames of pure background (averaging equal values is exact), for what it does
to silhouettes, for write coverage in guarded buffers, for its schedule (path 7, no wavefront pipeline, tuners untouched, staging
in flight), for its device-side errors, and through render_sequence(..., supersample=2) against the oracle's whole export chain."""
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
from raymarcher_amd import abi, lib
from raymarcher_amd._lib import RaymarcherError

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(ROOT, "tests", "golden", "scenes")
# (ss, W, H) of the oracle comparisons: ss·W and ss·H are multiples of 8 in neither (edge tiles partial in both axes)
ODD = [(2, 45, 27), (4, 97, 61)]


def resolve(S, ss):
    """The definition: (ss·H, ss·W, 4) float32, rows bottom-up → (H, W, 4)."""
    S = np.ascontiguousarray(S, dtype=np.float32)
    assert S.dtype == np.float32 and S.shape[0] % ss == 0 and S.shape[1] % ss == 0
    level = 1
    while level < ss:
        a = S[:, 0::2] + S[:, 1::2]
        S = a[0::2] + a[1::2]
        level *= 2
    out = S * np.float32(1 / ss ** 2)
    assert out.dtype == np.float32
    return out


def test_resolve_is_the_tree_of_the_header():
    """The NumPy definition against the same tree written out per pixel with explicit binary32 roundings."""
    rng = np.random.default_rng(3)
    f = np.float32
    for ss in (2, 4):
        S = (rng.standard_normal((2 * ss, 3 * ss, 4)) * 10.0 ** rng.integers(-3, 4, (2 * ss, 3 * ss, 4))).astype(f)
        got = resolve(S, ss)
        for Y in range(2):
            for X in range(3):
                blk = S[ss * Y:ss * Y + ss, ss * X:ss * X + ss]  # [j][i]
                lvl = blk
                while lvl.shape[0] > 1:
                    a = np.stack([[f(lvl[j, 2 * i] + lvl[j, 2 * i + 1]) for i in range(lvl.shape[1] // 2)] for j in range(lvl.shape[0])])
                    lvl = np.stack([[f(a[2 * j, i] + a[2 * j + 1, i]) for i in range(a.shape[1])] for j in range(a.shape[0] // 2)])
                exp = f(lvl[0, 0] * f(0.25 if ss == 2 else 0.0625))
                assert (got[Y, X].view(np.uint32) == exp.view(np.uint32)).all()


def oracle_resolved(scene, cam, g, s, W, H, ss, textures=None, **resources):
    """(fragColor, BrightColor) of the definition: the oracle at ss·W × ss·H, asserted finite everywhere (NaN payloads could
    differ between NumPy and the GPU), reduced."""
    S, Sb = h.oracle_render((cam,) + tuple(scene[1:5]) + (g,), s, ss * W, ss * H, bright=True, threads=16, textures=textures, **resources)
    assert np.isfinite(S).all() and np.isfinite(Sb).all(), "the oracle's sample frame is not finite: choose another camera"
    return resolve(S, ss), resolve(Sb, ss)


def ss_vs_oracle(renderer, scene, s, cams_of, globs, sizes=ODD, textures=None, what="", **resources):
    """cams_of(W, H) → the cameras; globs: one RmGlobals or one per camera.  Every frame, fragColor and BrightColor, both ss."""
    outs = {}
    for ss, W, H in sizes:
        cams = cams_of(W, H)
        t = tables_of(scene, **resources)
        if textures:
            t.textures = textures
        out, br = renderer.render_supersampled(t, s, W, H, cams, ss, globals_=globs, bright=True)
        assert tuple(out.shape) == (len(cams), H, W, 4) and tuple(br.shape) == (len(cams), H, W, 4)
        assert lib().rm_debug_last_path() == 7 and lib().rm_debug_last_split() == 0
        out, br = out.cpu().numpy(), br.cpu().numpy()
        for f, cam in enumerate(cams):
            g = globs[f] if isinstance(globs, (list, tuple)) else globs
            ref, ref_b = oracle_resolved(scene, cam, g, s, W, H, ss, textures=textures, **resources)
            assert_bit_equal(out[f], ref, f"{what} ss {ss} {W}x{H} frame {f}")
            assert_bit_equal(br[f], ref_b, f"{what} ss {ss} {W}x{H} frame {f} bright")
        outs[ss] = out
    return outs


# ---------------------------------------------------------------- 1. bit for bit against the oracle, every class of the dispatcher
def test_bulb_plain_form(renderer):
    scene = h.scene_mandelbulb(64, 36)
    globs = [with_globals(scene[5], iTime=0.5 * f) for f in range(4)]
    assert all(lib().rm_debug_bulb_plain(scene[1], 1, C.byref(g)) == 1 for g in globs)
    outs = ss_vs_oracle(renderer, scene, abi.default_settings(fractalIters=12),
                        lambda W, H: orbit((0, 0, 4.5), (0, 0, -1), 30.0, W, H, 4, deg=7.0), globs, what="plain bulb")
    assert np.abs(outs[4][0] - outs[4][3]).max() > 0.05  # the frames differ


def test_bulb_general_form_mixed_with_plain(renderer):
    scene = h.scene_mandelbulb(64, 36)
    globs = [with_globals(scene[5], power=(8.0 if f % 2 == 0 else 7.5), iTime=0.3 * f) for f in range(4)]
    assert [lib().rm_debug_bulb_plain(scene[1], 1, C.byref(g)) for g in globs] == [1, 0, 1, 0]
    ss_vs_oracle(renderer, scene, abi.default_settings(), lambda W, H: orbit((0, 0, 4.5), (0, 0, -1), 30.0, W, H, 4, deg=5.0), globs,
                 what="power 8 / 7.5 bulb")


def test_primitives_two_lights_soft_shadows_ao(renderer):
    scene = SB.reflect_refract_scene(64, 36)  # reflection / refraction off below: the plain table walk
    globs = [with_globals(scene[5], iTime=0.25 * f) for f in range(3)]
    ss_vs_oracle(renderer, scene, abi.default_settings(enableSoftShadow=1, enableAmbientOcclusion=1),
                 lambda W, H: orbit((0, 1.2, 5), (0, -0.2, -1), 40.0, W, H, 3, deg=6.0), globs, what="primitives soft+AO")


def test_reflection_and_refraction_two_bounces(renderer):
    scene = SB.reflect_refract_scene(64, 36)
    s = abi.default_settings(enableReflection=1, enableRefraction=1, numReflection=2)
    ss_vs_oracle(renderer, scene, s, lambda W, H: orbit((0, 1.2, 5), (0, -0.2, -1), 40.0, W, H, 3, deg=8.0), scene[5],
                 what="reflection+refraction")


def test_menger_sponge_with_reflection_never_takes_the_wavefront_pipeline(renderer):
    L = lib()
    scene = SB.menger_scene(64, 36)
    globs = [with_globals(scene[5], iTime=3.7 * f) for f in range(3)]
    s = abi.default_settings(mengerLevels=4, enableReflection=1, numReflection=1)
    cams_of = lambda W, H: orbit((2.6, 2.2, 3.0), (-2.6, -2.2, -3.0), 30.0, W, H, 3, deg=5.0)  # noqa: E731
    plain = ss_vs_oracle(renderer, scene, s, cams_of, globs, what="menger")
    try:
        assert L.rm_set_kernel_path(5) == 0
        # the single-frame launcher sends this very frame to the wavefront pipeline …
        ss, W, H = ODD[0]
        renderer.render(tables_of((cams_of(ss * W, ss * H)[0],) + tuple(scene[1:5]) + (globs[0],)), s, ss * W, ss * H)
        assert L.rm_debug_last_path() == 5
        # … the supersampled launch does not (ss_vs_oracle asserts path 7), with the same bits
        forced = ss_vs_oracle(renderer, scene, s, cams_of, globs, sizes=ODD[:1], what="menger, path 5 requested")
        assert_bit_equal(forced[ss], plain[ss], "menger with and without the path request")
    finally:
        L.rm_set_kernel_path(0)


def test_textures_sky_box_and_area_light(renderer):
    scene = SB.textured_scene(64, 36)
    s = abi.default_settings(features=abi.RM_FEAT_WHITE_BACKGROUND, enableSoftShadow=1, enableSkyBox=1)
    ss_vs_oracle(renderer, scene, s, lambda W, H: orbit((0.4, 2.2, 5.5), (-0.05, -0.35, -1), 42.0, W, H, 3, deg=6.0), scene[5],
                 textures=SB.synthetic_textures(), what="textured + sky box", skybox=SB.synthetic_skybox())
    scene, s, res = SB.resource_case("area_light", 64, 36)
    s.enableSkyBox = 1
    ss_vs_oracle(renderer, scene, s, lambda W, H: orbit((0, 1.6, 5.5), (0, -0.2, -1), 45.0, W, H, 3, deg=7.0), scene[5],
                 what="area light + sky box", skybox=SB.synthetic_skybox(), **res)


def test_terrain_and_clouds_with_advancing_time(renderer):
    scene = SB.env_scene(64, 36)
    globs = [with_globals(scene[5], iTime=4.0 * f) for f in range(3)]
    ss_vs_oracle(renderer, scene, abi.default_settings(features=SB.ENV_ALL, enableReflection=1),
                 lambda W, H: orbit((0, 500, 5), (0.3, 0.12, -1), 70.0, W, H, 3, deg=3.0, far=2000.0), globs,
                 what="terrain+cloud")


def test_sea_and_night_sky_with_the_noise_texture(renderer):
    scene, s, res = SB.resource_case("sea_sky", 64, 36)
    globs = [with_globals(scene[5], iTime=0.7 + 0.9 * f) for f in range(3)]
    ss_vs_oracle(renderer, scene, s, lambda W, H: orbit((0, 3.5, 6), (0, -0.35, -1), 50.0, W, H, 3, deg=5.0), globs,
                 what="sea + sky", **res)
    scene, s, res = SB.resource_case("night_sky", 64, 36)
    ss_vs_oracle(renderer, scene, s, lambda W, H: orbit((1.6, 0.4, -5), (-0.42, 0.36, 1), 60.0, W, H, 3, deg=4.0), scene[5],
                 what="night sky", **res)


# ---------------------------------------------------------------- 2. against the library itself
def class_case(name, W, H):
    """name → (scene, settings, resources, textures) of one kernel class."""
    if name == "bulb_plain":
        return h.scene_mandelbulb(W, H), abi.default_settings(fractalIters=12), {}, None
    if name == "bulb_general":
        sc = h.scene_mandelbulb(W, H)
        return sc[:5] + (with_globals(sc[5], power=7.5),), abi.default_settings(), {}, None
    if name == "table":
        return SB.reflect_refract_scene(W, H), abi.default_settings(enableSoftShadow=1, enableAmbientOcclusion=1), {}, None
    if name == "table_sec":
        return SB.reflect_refract_scene(W, H), abi.default_settings(enableReflection=1, enableRefraction=1, numReflection=2), {}, None
    if name == "menger":
        return SB.menger_scene(W, H), abi.default_settings(mengerLevels=4, enableReflection=1, numReflection=1), {}, None
    if name == "textures":
        return SB.textured_scene(W, H), abi.default_settings(enableSoftShadow=1), {}, SB.synthetic_textures()
    if name == "layers":
        return SB.env_scene(W, H), abi.default_settings(features=SB.ENV_ALL, enableReflection=1), {}, None
    if name == "layers_textures":
        return SB.reflect_refract_scene(W, H), abi.default_settings(features=SB.ENV_ALL, enableSkyBox=1), {"skybox": SB.synthetic_skybox()}, None
    if name in ("sea_sky", "night_sky", "skybox_reflect", "area_light"):
        return SB.resource_case(name, W, H) + (None,)
    raise KeyError(name)


CLASSES = ["bulb_plain", "bulb_general", "table", "table_sec", "menger", "textures", "layers", "layers_textures", "sea_sky", "night_sky",
           "skybox_reflect", "area_light"]


def class_tables(name, W, H):
    scene, s, res, textures = class_case(name, W, H)
    t = tables_of(scene, **res)
    if textures:
        t.textures = textures
    return scene, t, s


@pytest.mark.parametrize("name", CLASSES)
def test_equals_rm_render_res_reduced_on_the_host(renderer, name):
    for ss, W, H in ((2, 131, 75), (4, 67, 45)):
        scene, t, s = class_tables(name, W, H)
        S, Sb = renderer.render(t, s, ss * W, ss * H, bright=True)
        S, Sb = S.cpu().numpy(), Sb.cpu().numpy()
        out, br = renderer.render_supersampled(t, s, W, H, [scene[0]], ss, bright=True)
        assert lib().rm_debug_last_path() == 7
        assert np.isfinite(S).all() and np.isfinite(Sb).all()  # the bits of a NaN would be NumPy's own affair
        assert_bit_equal(out[0].cpu().numpy(), resolve(S, ss), f"{name} ss {ss}")
        assert_bit_equal(br[0].cpu().numpy(), resolve(Sb, ss), f"{name} ss {ss} bright")


def test_ss_1_is_render_batch(renderer):
    W, H = 77, 45
    scene = SB.reflect_refract_scene(W, H)
    s = abi.default_settings(enableReflection=1)
    cams = orbit((0, 1.2, 5), (0, -0.2, -1), 40.0, W, H, 3, deg=8.0)
    globs = [with_globals(scene[5], iTime=0.25 * f) for f in range(3)]
    a, ab = renderer.render_supersampled(tables_of(scene), s, W, H, cams, 1, globals_=globs, bright=True)
    assert lib().rm_debug_last_path() == 6  # rm_render_batch's own launch
    b, bb = renderer.render_batch(tables_of(scene), s, W, H, cams, globals_=globs, bright=True)
    assert SB.ieq(a, b) and SB.ieq(ab, bb)


# ---------------------------------------------------------------- 3. a frame of pure background
@pytest.mark.parametrize("ss", [2, 4])
def test_pure_background_is_the_1x_frame(renderer, ss):
    W, H = 45, 27
    for scene in (h.scene_mandelbulb(W, H), SB.reflect_refract_scene(W, H)):
        away = h.make_camera((0, 0, 4.5), (0, 0, 1), (0, 1, 0), 30.0, W, H)  # every object is behind the camera
        s = abi.default_settings(features=abi.RM_FEAT_WHITE_BACKGROUND)
        t = tables_of((away,) + tuple(scene[1:]))
        one, one_b = renderer.render(t, s, W, H, bright=True)
        assert float(one[..., :3].min()) == 1.0  # nothing but the white background
        out, br = renderer.render_supersampled(t, s, W, H, [away], ss, bright=True)
        assert SB.ieq(out[0], one) and SB.ieq(br[0], one_b)


# ---------------------------------------------------------------- 4. it anti-aliases
def test_silhouettes_converge_with_the_sample_count(renderer):
    W, H = 128, 80
    scene = h.scene_mandelbulb(W, H)
    s = abi.default_settings(fractalIters=12)
    t = tables_of(scene)
    img = {ss: renderer.render_supersampled(t, s, W, H, [scene[0]], ss)[0].cpu().numpy() for ss in (1, 2, 4)}
    bg = img[1][0, 0]
    hit = (img[1] != bg).any(axis=-1)
    edge = np.zeros_like(hit)  # silhouette pixels of the 1× image: a 4-neighbour across the hit / background boundary
    edge[:, 1:] |= hit[:, 1:] != hit[:, :-1]
    edge[:, :-1] |= hit[:, 1:] != hit[:, :-1]
    edge[1:] |= hit[1:] != hit[:-1]
    edge[:-1] |= hit[1:] != hit[:-1]
    assert edge.sum() > 100
    differs = (img[2] != img[1]).any(axis=-1)
    assert differs[edge].mean() > 0.5, "supersampling left most silhouette pixels as the centre ray found them"
    assert not differs[(img[4] == bg).all(axis=-1) & ~edge].any()  # background stays background
    d1, d2 = np.abs(img[1] - img[4]).mean(), np.abs(img[2] - img[4]).mean()
    assert d2 < d1, (d1, d2)


# ---------------------------------------------------------------- 5. write coverage
@pytest.mark.parametrize("ss,W,H", ODD + [(2, 1, 1), (4, 1, 1), (4, 3, 70), (2, 65, 9)])
@pytest.mark.parametrize("n", [1, 3])
def test_every_word_is_written_and_nothing_else(renderer, ss, W, H, n):
    for name in ("bulb_plain", "table_sec"):
        scene, t, s = class_tables(name, W, H)
        cams = [scene[0]] * n
        out, c1 = h.guarded((n, H, W, 4), device=renderer.device)
        br, c2 = h.guarded((n, H, W, 4), device=renderer.device)
        renderer.render_supersampled(t, s, W, H, cams, ss, out=out, out_bright=br)
        c1()
        c2()
        # d_bright = NULL: the same frames, and a neighbouring poisoned allocation is left alone
        out2, c3 = h.guarded((n, H, W, 4), device=renderer.device)
        spare = h.Guarded((n, H, W, 4), renderer.torch.float32, h.FLOAT_POISON, renderer.device)
        renderer.render_supersampled(t, s, W, H, cams, ss, out=out2)
        c3()
        assert SB.ieq(out2, out)
        assert bool(spare._unwritten(spare.buf).all()), "a launch without d_bright wrote outside d_rgba"
        for f in range(1, n):
            assert SB.ieq(out[f], out[0]) and SB.ieq(br[f], br[0])


_CHILD = r'''
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_supersample as t
from raymarcher_amd import Renderer
r = Renderer(0)
for name in ("bulb_plain", "table_sec", "textures"):
    t.test_equals_rm_render_res_reduced_on_the_host(r, name)
for ss, W, H in t.ODD:
    t.test_every_word_is_written_and_nothing_else(r, ss, W, H, 3)
print("ok")
'''


@pytest.mark.parametrize("wpb", [2, 4])
def test_wider_workgroups_render_the_same_frames(renderer, wpb):
    """RM_WAVES_PER_BLOCK (read once per process): the supersampling kernel with 2 and 4 waves per workgroup, in a child."""
    env = dict(os.environ, RM_WAVES_PER_BLOCK=str(wpb))
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]


# ---------------------------------------------------------------- 6. schedule and state
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
        renderer.render_supersampled(tables_of(scene), s, W, H, cams, 2)
        renderer.torch.cuda.synchronize(renderer.device)
        total, stages, n = C.c_double(), (C.c_double * 4)(), C.c_int()
        assert L.rm_get_stage_timing(C.byref(total), stages, C.byref(n)) == 0
        assert n.value == 1 and total.value > 0.0
        assert stages[0] == 0.0 and stages[1] == total.value and stages[2] == 0.0 and stages[3] == 0.0
    finally:
        L.rm_set_timing(0)


def test_supersampled_launch_leaves_the_single_frame_tuners_alone(renderer):
    L = lib()
    W, H = 512, 320
    t = _c2(W, H)
    s = abi.default_settings(enableSoftShadow=1, enableAmbientOcclusion=1)
    other = tables_of((orbit((0, 1, 8), (0, -0.1, -1), 40.0, W, H, 1)[0], t.objects, t.num_objects, t.lights, t.num_lights, t.globals_))
    cams = [other.camera, t.camera, other.camera]

    def sequence(ss_after=None):
        renderer.render(other, s, W, H)  # another picture of the same size: the picture below starts afresh
        splits, frames = [], []
        for k in range(12):
            if k == ss_after:
                renderer.render_supersampled(t, s, W // 2, H // 2, cams, 2)  # the same sample frame as the picture's
                assert L.rm_debug_last_path() == 7 and L.rm_debug_last_split() == 0
            frames.append(renderer.render(t, s, W, H).clone())
            assert L.rm_debug_last_path() == 1
            splits.append(L.rm_debug_last_split())
        return splits, frames

    try:
        assert L.rm_debug_set_tile_shape(3) == 0  # no timed shape tuning: the sequence depends on the tile-order state alone
        assert L.rm_debug_set_light_split(32) == 0  # split a settled picture without measuring
        plain, frames = sequence()
        assert sequence()[0] == plain, "the sequence is not deterministic without a supersampled launch"
        assert plain[0] == 0 and plain[-1] > 0, plain  # it settles, then splits
        again, frames2 = sequence(ss_after=plain.index(plain[-1]) + 1)
        assert again == plain
        assert all(SB.ieq(a, frames[0]) for a in frames + frames2)
    finally:
        L.rm_debug_set_tile_shape(-1)
        L.rm_debug_set_light_split(-1)


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
        a = renderer.render_supersampled(t, s, W, H, cams_a, ss, globals_=globs_a)
        b = renderer.render_supersampled(t, s, W, H, cams_b, ss)
    stream.synchronize()
    Sa = renderer.render_batch(t, s, ss * W, ss * H, cams_a, globals_=globs_a).cpu().numpy()
    Sb = renderer.render_batch(t, s, ss * W, ss * H, cams_b).cpu().numpy()
    assert np.isfinite(Sa).all() and np.isfinite(Sb).all()
    a, b = a.cpu().numpy(), b.cpu().numpy()
    for f in range(300):
        assert_bit_equal(a[f], resolve(Sa[f], ss), f"first launch, frame {f}")
    for f in range(40):
        assert_bit_equal(b[f], resolve(Sb[f], ss), f"second launch, frame {f}")
    assert np.abs(a[0] - a[299]).max() > 0.05


# ---------------------------------------------------------------- 7. errors on the device
def test_host_output_pointer_is_refused_and_hip_stays_clean(renderer):
    L = lib()
    W, H = 16, 8
    scene = h.scene_mandelbulb(W, H)
    cams = (abi.RmCamera * 2)(scene[0], scene[0])
    host = np.zeros((2, H, W, 4), dtype=np.float32)
    for ss in (2, 4):
        st = L.rm_render_supersampled(cams, C.byref(scene[5]), 1, 2, scene[1], 1, scene[3], scene[4], C.byref(abi.default_settings()),
                                      None, W, H, ss, C.c_void_p(host.ctypes.data), None, None)
        assert st == abi.RM_ERR_INVALID_ARGUMENT
        assert "not device-accessible" in L.rm_last_error().decode()
    dev = renderer.torch.empty((2, H, W, 4), dtype=renderer.torch.float32, device=renderer.device)
    st = L.rm_render_supersampled(cams, C.byref(scene[5]), 1, 2, scene[1], 1, scene[3], scene[4], C.byref(abi.default_settings()),
                                  None, W, H, 2, C.c_void_p(dev.data_ptr()), C.c_void_p(host.ctypes.data), None)
    assert st == abi.RM_ERR_INVALID_ARGUMENT
    out = renderer.render_supersampled(tables_of(scene), abi.default_settings(), W, H, [scene[0]], 2)  # a following render succeeds
    renderer.torch.cuda.synchronize(renderer.device)
    assert bool(renderer.torch.isfinite(out).all())


def test_a_missing_sampler_is_unsupported(renderer):
    W, H = 16, 16
    for name in ("night_sky", "sea_sky", "skybox_reflect", "area_light"):
        scene, s, _res = SB.resource_case(name, W, H)
        with pytest.raises(RaymarcherError) as e:
            renderer.render_supersampled(tables_of(scene), s, W, H, [scene[0]], 2)
        assert e.value.status == abi.RM_ERR_UNSUPPORTED, name
    scene = h.scene_mandelbulb(W, H)
    ref = renderer.render(tables_of(scene), abi.default_settings(), 2 * W, 2 * H).cpu().numpy()
    out = renderer.render_supersampled(tables_of(scene), abi.default_settings(), W, H, [scene[0]], 2)
    assert_bit_equal(out[0].cpu().numpy(), resolve(ref, 2), "the render after the refusals")


# ---------------------------------------------------------------- 8. render_sequence(..., supersample=2)
def test_render_sequence_supersampled_equals_the_oracle_chain(renderer):
    W, H, N, ss = 75, 45, 3, 2
    scene = SB.reflect_refract_scene(W, H)
    for li in scene[3]:
        li.color[0] *= 2.5; li.color[1] *= 2.5; li.color[2] *= 2.5  # over-exposed: BrightColor is populated
    s = abi.default_settings(enableReflection=1)
    cams = orbit((0, 1.2, 5), (0, -0.2, -1), 40.0, W, H, N)
    globs = [with_globals(scene[5], iTime=0.25 * f) for f in range(N)]
    post = abi.RmPostSettings(**{"exposure": 1.0, **SB.POST_CASES["bloom_hdr_fxaa"]})
    assert post.enableBloom and post.enableHDR and post.enableFXAA
    imgs = renderer.render_sequence(tables_of(scene), s, W, H, cams, globals_=globs, post=post, supersample=ss)
    assert lib().rm_debug_last_path() == 7
    assert tuple(imgs.shape) == (N, H, W, 4) and imgs.dtype == renderer.torch.uint8
    imgs = imgs.cpu().numpy()
    for f in range(N):
        frag, bright = oracle_resolved(scene, cams[f], globs[f], s, W, H, ss)
        if f == 0:
            assert bright[..., :3].max() > 1.0
        ref = h.oracle_post(frag, bright, post)
        exp = (np.clip(ref[::-1], 0, 1) * np.float32(255.0) + np.float32(0.5)).astype(np.uint8)
        assert (imgs[f] == exp).all(), f"frame {f}: {(imgs[f] != exp).sum()} bytes differ"
    # supersample=1 is the call without the keyword, byte for byte
    one = renderer.render_sequence(tables_of(scene), s, W, H, cams, globals_=globs, post=post, supersample=1)
    assert lib().rm_debug_last_path() == 6
    bare = renderer.render_sequence(tables_of(scene), s, W, H, cams, globals_=globs, post=post)
    assert bool((one == bare).all())
    assert (one.cpu().numpy() != imgs).any()  # and supersampling changes the picture
