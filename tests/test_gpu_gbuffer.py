"""rm_render_gbuffer / Renderer.render_gbuffer on the GPU: normal + depth, object index and position of every pixel's primary hit, bit
for bit against the specification (tests/gbuffer_spec/rm_gbuffer_spec.c: the oracle's own raymarch, getNormal and bumpNormal) for
the three march classes, the sponge prologue, a fractal in a table walk and an emissive rectangle; batches with partial tiles; the
optional position output; the schedule (rm_debug_last_path 11) and the single-frame state left alone.  Every output goes into
poisoned, guarded buffers: an element the launch never wrote, or a write outside them, fails."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import gbuffer_helpers as G
import helpers as h
import test_gpu_parity as P
from raymarcher_amd import abi, lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(ROOT, "tests", "golden", "scenes")
INT_POISON = 0x5AA5A55A  # no object index and not −1


def tables_of(scene):
    from raymarcher_amd.render import SceneTables
    return SceneTables(*scene)


def with_globals(g, **over):
    g2 = abi.RmGlobals()
    C.memmove(C.byref(g2), C.byref(g), C.sizeof(g))
    for k, v in over.items():
        setattr(g2, k, v)
    return g2


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_bits(got, want, what):
    bad = bits(got) != bits(want)
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} words differ; first at {np.argwhere(bad)[:5].tolist()}"


def gbuffer_guarded(renderer, t, s, W, H, cameras=None, globals_=None, position=True):
    """Renderer.render_gbuffer into poisoned, guarded buffers, checked → numpy (normal_depth, object_id, position or None)."""
    n = 1 if cameras is None else len(cameras)
    nd, c1 = h.guarded((n, H, W, 4), device=renderer.device)
    ids, c2 = h.guarded((n, H, W), torch.int32, INT_POISON, device=renderer.device)
    pos, c3 = h.guarded((n, H, W, 4), device=renderer.device) if position else (None, None)
    got = renderer.render_gbuffer(t, s, W, H, cameras=cameras, globals_=globals_, out_normal_depth=nd, out_object_id=ids, out_position=pos)
    assert len(got) == (3 if position else 2) and got[0] is nd and got[1] is ids
    assert lib().rm_debug_last_path() == 11 and lib().rm_debug_last_split() == 0
    c1()
    c2()
    if position:
        c3()
    return nd.cpu().numpy(), ids.cpu().numpy(), pos.cpu().numpy() if position else None


def check_against_spec(renderer, scene, s, W, H, what, cameras=None, globals_=None):
    """Every frame of the call against the spec of its own camera and globals; returns the GPU outputs and the specs' ids."""
    t = tables_of(scene)
    nd, ids, pos = gbuffer_guarded(renderer, t, s, W, H, cameras, globals_)
    cams = [scene[0]] if cameras is None else cameras
    spec_ids = []
    for f, cam in enumerate(cams):
        g = scene[5] if globals_ is None else (globals_[f] if isinstance(globals_, (list, tuple)) else globals_)
        snd, sids, spos = G.spec_gbuffer(cam, scene[1], scene[2], g, s, W, H)
        assert_bits(nd[f], snd, f"{what} frame {f} normalDepth")
        assert (ids[f] == sids).all(), f"{what} frame {f} objectId: {(ids[f] != sids).sum()} differ"
        assert_bits(pos[f], spos, f"{what} frame {f} position")
        spec_ids.append(sids)
    return nd, ids, pos, spec_ids


def moved_bulb_scene(W, H):
    scene = h.scene_mandelbulb(W, H)
    model = h.translate(0.15, -0.1, 0.2) @ h.rotation((0.3, 1.0, -0.2), 0.7)
    objs = (abi.RmObject * 1)(h.make_object(abi.RM_MANDELBULB, model=model))
    return (scene[0], objs, 1) + tuple(scene[3:])


def directional_light_2(W, H):
    from raymarcher_amd import Scene
    t = Scene(path=os.path.join(SCENES, "lighting", "directional_light_2.json")).tables(W, H)
    return t.camera, t.objects, t.num_objects, t.lights, t.num_lights, t.globals_


# ---------------------------------------------------------------- the march classes, bit for bit
@pytest.mark.parametrize("bump", [True, False])
def test_plain_bulb(renderer, bump):
    W, H = 64, 36
    scene = h.scene_mandelbulb(W, H)
    assert lib().rm_debug_bulb_plain(scene[1], 1, C.byref(scene[5])) == 1
    s = abi.default_settings(features=abi.RM_FEAT_WHITE_BACKGROUND | (abi.RM_FEAT_PERLIN_BUMP if bump else 0))
    nd, ids, _, _ = check_against_spec(renderer, scene, s, W, H, "plain bulb")
    assert 0.2 < (ids >= 0).mean() < 0.5 and set(np.unique(ids)) == {-1, 0}
    assert np.isfinite(nd).all()


def test_general_bulb(renderer):
    W, H = 64, 36
    scene = moved_bulb_scene(W, H)
    assert lib().rm_debug_bulb_plain(scene[1], 1, C.byref(scene[5])) == 0
    _, ids, _, _ = check_against_spec(renderer, scene, abi.default_settings(), W, H, "general bulb")
    assert 0.1 < (ids >= 0).mean() < 0.6
    # a plain table under globals that are not plain takes the general class too
    scene = h.scene_mandelbulb(W, H)
    g = with_globals(scene[5], power=7.0)
    assert lib().rm_debug_bulb_plain(scene[1], 1, C.byref(g)) == 0
    check_against_spec(renderer, scene[:5] + (g,), abi.default_settings(), W, H, "power 7 bulb")


def test_table_walk(renderer):
    W, H = 64, 36
    scene = directional_light_2(W, H)
    _, ids, _, _ = check_against_spec(renderer, scene, abi.default_settings(), W, H, "directional_light_2")
    seen = set(np.unique(ids).tolist())
    assert -1 in seen and len(seen - {-1}) >= 3, seen
    # soft shadows, AO, reflection, a sky box without faces: none of them is read
    s = abi.default_settings(enableSoftShadow=1, enableAmbientOcclusion=1, enableReflection=1, enableSkyBox=1)
    nd2, ids2, _ = gbuffer_guarded(renderer, tables_of(scene), s, W, H)
    nd1, ids1, _ = gbuffer_guarded(renderer, tables_of(scene), abi.default_settings(), W, H)
    assert_bits(nd2, nd1, "shading settings")
    assert (ids2 == ids1).all()


def test_menger_sponge_with_the_prologue(renderer):
    W, H = 48, 27
    scene = P.menger_scene(W, H)
    scene[5].iTime = 7.5
    _, ids, _, _ = check_against_spec(renderer, scene, abi.default_settings(mengerLevels=3), W, H, "menger depth 3")
    assert 0.05 < (ids >= 0).mean() < 0.95


def test_fractal_behind_a_primitive_runs_the_table_walk(renderer):
    W, H = 64, 36
    scene = h.scene_mandelbulb(W, H)
    objs = (abi.RmObject * 2)(h.make_object(abi.RM_MANDELBULB),
                              h.make_object(abi.RM_SPHERE, model=h.translate(0.5, 0.2, 1.6) @ h.scale(0.8, 0.8, 0.8), scale_factor=0.8))
    scene = (scene[0], objs, 2) + tuple(scene[3:])
    _, ids, _, _ = check_against_spec(renderer, scene, abi.default_settings(), W, H, "bulb behind a sphere")
    assert {0, 1, -1} <= set(np.unique(ids).tolist())


def test_emissive_rectangle_reports_its_own_index(renderer):
    W, H = 64, 36
    scene = P.area_light_scene(W, H)
    assert scene[1][3].isEmissive == 1
    _, ids, _, _ = check_against_spec(renderer, scene, abi.default_settings(), W, H, "area light")
    assert (ids == 3).sum() > 10 and -1 in ids


# ---------------------------------------------------------------- batches
@pytest.mark.parametrize("shared_globals", [False, True])
def test_batch_of_five_with_partial_tiles(renderer, shared_globals):
    W, H = 37, 19  # partial tiles on both axes
    scene = moved_bulb_scene(W, H)
    cams = [h.make_camera(P_pos, tuple(-v for v in P_pos), (0, 1, 0), 30.0, W, H)
            for P_pos in ((0, 0, 4.5), (1.0, 0.3, 4.3), (-1.2, 0.8, 4.0), (0.4, -1.5, 4.1), (2.5, 1.0, 3.5))]
    globs = scene[5] if shared_globals else [with_globals(scene[5], iTime=0.4 * f, power=8.0 - 0.5 * f) for f in range(5)]
    s = abi.default_settings(fractalIters=10)
    nd, ids, pos, _ = check_against_spec(renderer, scene, s, W, H, "batch", cameras=cams, globals_=globs)
    assert len({ids[f].tobytes() for f in range(5)}) == 5  # the frames differ
    t = tables_of(scene)
    for f in range(5):
        g = globs if shared_globals else globs[f]
        nd1, ids1, pos1 = gbuffer_guarded(renderer, t, s, W, H, cameras=[cams[f]], globals_=g)
        assert_bits(nd[f], nd1[0], f"frame {f} against a one-frame call")
        assert (ids[f] == ids1[0]).all()
        assert_bits(pos[f], pos1[0], f"frame {f} position against a one-frame call")


def test_batch_where_one_frame_is_not_plain_takes_the_general_class_for_all(renderer):
    W, H = 40, 27
    scene = h.scene_mandelbulb(W, H)
    cams = [scene[0]] * 3
    globs = [with_globals(scene[5], power=p) for p in (8.0, 6.5, 8.0)]
    assert [lib().rm_debug_bulb_plain(scene[1], 1, C.byref(g)) for g in globs] == [1, 0, 1]
    check_against_spec(renderer, scene, abi.default_settings(), W, H, "mixed plain", cameras=cams, globals_=globs)


# ---------------------------------------------------------------- the optional output, the schedule, the state
def test_without_position_the_required_outputs_are_the_same_bits(renderer):
    W, H = 64, 36
    for scene in (directional_light_2(W, H), h.scene_mandelbulb(W, H)):
        t = tables_of(scene)
        s = abi.default_settings()
        nd, ids, pos = gbuffer_guarded(renderer, t, s, W, H, position=True)
        nd0, ids0, none = gbuffer_guarded(renderer, t, s, W, H, position=False)
        assert none is None
        assert_bits(nd0, nd, "normalDepth without position")
        assert (ids0 == ids).all()
        # fresh outputs of the wrapper: shapes and types
        a, b = renderer.render_gbuffer(t, s, W, H)
        assert tuple(a.shape) == (1, H, W, 4) and a.dtype == torch.float32 and tuple(b.shape) == (1, H, W) and b.dtype == torch.int32
        assert_bits(a.cpu().numpy(), nd, "fresh outputs")


def test_path_and_device_pointer_errors(renderer):
    L = lib()
    W, H = 32, 24
    scene = h.scene_mandelbulb(W, H)
    renderer.render(tables_of(scene), abi.default_settings(), W, H)
    assert L.rm_debug_last_path() == 1
    renderer.render_gbuffer(tables_of(scene), abi.default_settings(), W, H)
    assert L.rm_debug_last_path() == 11 and L.rm_debug_last_split() == 0
    dev = torch.empty((H, W, 4), dtype=torch.float32, device=renderer.device)
    host = np.zeros((H, W, 4), dtype=np.float32)
    s = abi.default_settings()
    dp, hp = C.c_void_p(dev.data_ptr()), C.c_void_p(host.ctypes.data)
    for nd, ids, pos, name in ((hp, dp, None, "d_normalDepth"), (dp, hp, None, "d_objectId"), (dp, dp, hp, "d_position")):
        st = L.rm_render_gbuffer(C.byref(scene[0]), C.byref(scene[5]), 1, 1, scene[1], 1, C.byref(s), W, H, nd, ids, pos, None)
        assert st == abi.RM_ERR_INVALID_ARGUMENT and f"{name} is not device-accessible" in L.rm_last_error().decode()


def test_single_frame_renders_are_the_same_bits_before_and_after(renderer):
    from raymarcher_amd import Scene
    W = H = 256
    t = Scene(path=os.path.join(SCENES, "simple", "unit_sphere.json")).tables(W, H)
    s = abi.default_settings(maxSteps=64)
    before = [renderer.render(t, s, W, H).clone() for _ in range(2)]
    renderer.render_gbuffer(t, s, W, H, position=True)
    assert lib().rm_debug_last_path() == 11
    after = [renderer.render(t, s, W, H).clone() for _ in range(2)]
    assert lib().rm_debug_last_path() == 1
    for a in before + after:
        assert P._ieq(a, before[0])
