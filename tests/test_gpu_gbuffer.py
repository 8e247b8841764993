"""rm_render_gbuffer / Renderer.render_gbuffer on the GPU: normal + depth, object index and position of every pixel's primary hit, bit
for bit against the specification (tests/gbuffer_spec/rm_gbuffer_spec.c: the oracle's own raymarch, getNormal and bumpNormal) for
the three march classes, the sponge prologue, a fractal in a table walk and an emissive rectangle; batches with partial tiles; the
optional position output; the schedule (rm_debug_last_path 11) and the single-frame state left alone.  Every output goes into
poisoned, guarded buffers: an element the launch never wrote, or a write outside them, fails.
Further down: the wide random tables of scene_builders (nested, coincident, sheared and strongly scaled objects: what the skip-test
seeds handed to getNormal must survive), the edges of the definition, ragged frames with 1, 2 and 4 waves per workgroup, four
launches back to back on one stream, the hit count of the colour path and the timing record."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import arbiter_numpy as an
import gbuffer_helpers as G
import helpers as h
import scene_builders as SB
from helpers import assert_bit_equal as assert_bits, bits, tables_of, with_globals
from raymarcher_amd import abi, lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(ROOT, "tests", "golden", "scenes")
INT_POISON = 0x5AA5A55A  # no object index and not −1


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


def check_against_spec(renderer, scene, s, W, H, what, cameras=None, globals_=None, position=True):
    """Every frame of the call against the spec of its own camera and globals; returns the GPU outputs and the specs' ids."""
    t = tables_of(scene)
    nd, ids, pos = gbuffer_guarded(renderer, t, s, W, H, cameras, globals_, position)
    cams = [scene[0]] if cameras is None else cameras
    spec_ids = []
    for f, cam in enumerate(cams):
        g = scene[5] if globals_ is None else (globals_[f] if isinstance(globals_, (list, tuple)) else globals_)
        snd, sids, spos = G.spec_gbuffer(cam, scene[1], scene[2], g, s, W, H)
        assert_bits(nd[f], snd, f"{what} frame {f} normalDepth")
        assert (ids[f] == sids).all(), f"{what} frame {f} objectId: {(ids[f] != sids).sum()} differ"
        if position:
            assert_bits(pos[f], spos, f"{what} frame {f} position")
        spec_ids.append(sids)
    return nd, ids, pos, spec_ids


moved_bulb_scene, directional_light_2 = SB.moved_bulb_scene, SB.directional_light_2


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
    scene = SB.menger_scene(W, H)
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
    scene = SB.area_light_scene(W, H)
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
        assert SB.ieq(a, before[0])


# ---------------------------------------------------------------- random wide tables
def _fuzz(default_cases, default_seed):
    return int(os.environ.get("RM_FUZZ_CASES", str(default_cases))), int(os.environ.get("RM_FUZZ_SEED", str(default_seed)))


def _eye_inside_an_object(scene):
    objs = [(scene[1][i].type, np.array(list(scene[1][i].invModel), np.float64).reshape(4, 4).T, scene[1][i].scaleFactor) for i in range(scene[2])]
    eye = np.array([list(scene[0].eyePosition)[:3]], np.float64)
    return bool(an.Table(objs)(eye)[0][0] < 0.0)


@pytest.mark.parametrize("kind", ["tablewalk", "primitive"])
def test_random_tables_bit_exact(renderer, kind):
    """scene_builders' random tables — up to 30 objects, nested, coincident, sheared, anisotropic, scaleFactors that are not the
    smallest scale, cameras inside objects and on their bounding balls — with each case's own maxSteps and bump bit: the three
    outputs equal the spec in every bit.  The normal's taps may pass over an object only where render's skip-test seeds allow it."""
    cases, seed = _fuzz(48 if kind == "tablewalk" else 16, 20261018 if kind == "tablewalk" else 20261019)
    gen = SB.random_tablewalk_case if kind == "tablewalk" else SB.random_primitive_case
    rng = np.random.default_rng(seed)
    W, H = 56, 40
    seen = {"max_objects": 0, "inside": 0, "bump": 0, "plain": 0, "hits": 0}
    for i in range(cases):
        scene, s = gen(rng, W, H)
        _, ids, _, _ = check_against_spec(renderer, scene, s, W, H, f"seed {seed} {kind} case {i} ({scene[2]} objects)")
        seen["max_objects"] = max(seen["max_objects"], scene[2])
        seen["inside"] += _eye_inside_an_object(scene)
        seen["bump" if s.features & abi.RM_FEAT_PERLIN_BUMP else "plain"] += 1
        seen["hits"] += int((ids >= 0).any())
    print(f"GBUFFER_FUZZ kind={kind} seed={seed} cases={cases} mismatched_words=0 {seen}")
    if cases < 16:
        print(f"GBUFFER_FUZZ kind={kind}: {cases} cases are too few to assert what the run saw; coverage NOT asserted")
    else:
        assert seen["bump"] and seen["plain"] and seen["hits"] >= cases // 2, seen
        if kind == "tablewalk":
            assert seen["max_objects"] >= 20 and seen["inside"] >= 1, seen


def test_random_bulbs_bit_exact(renderer):
    """scene_builders' random single-Mandelbulb scenes (tiny and anisotropic models, Julia seeds, powers, maxSteps 1…256,
    fractalIters 1…20, the algebraic power-8 form, bump on and off, cameras inside the ball).  The generator never draws the plain
    class (its model is never the identity), so every fourth case keeps its camera and settings and takes the identity model,
    power 8 and no Julia seed."""
    cases, seed = _fuzz(16, 20261020)
    rng = np.random.default_rng(seed)
    W, H = 48, 40
    seen = {"plain": 0, "general": 0, "algebraic": 0, "bump": 0, "no_bump": 0, "hits": 0}
    for i in range(cases):
        scene, s = SB.random_bulb_case(rng, W, H)
        if i % 4 == 3:
            g = with_globals(scene[5], power=8.0)
            g.juliaSeed[0] = g.juliaSeed[1] = 0.0
            scene = (scene[0], (abi.RmObject * 1)(h.make_object(abi.RM_MANDELBULB)), 1, scene[3], scene[4], g)
        plain = lib().rm_debug_bulb_plain(scene[1], 1, C.byref(scene[5]))
        assert plain in (0, 1)
        _, ids, _, _ = check_against_spec(renderer, scene, s, W, H, f"seed {seed} bulb case {i} ({'plain' if plain else 'general'})")
        seen["plain" if plain else "general"] += 1
        seen["algebraic"] += bool(s.features & abi.RM_FEAT_BULB_POWER8_ALGEBRAIC)
        seen["bump" if s.features & abi.RM_FEAT_PERLIN_BUMP else "no_bump"] += 1
        seen["hits"] += int((ids >= 0).any())
    print(f"GBUFFER_FUZZ kind=bulb seed={seed} cases={cases} mismatched_words=0 {seen}")
    if cases < 16:
        print(f"GBUFFER_FUZZ kind=bulb: {cases} cases are too few to assert what the run saw; coverage NOT asserted")
    else:
        assert seen["plain"] and seen["general"] and seen["bump"] and seen["no_bump"] and seen["hits"] >= cases // 2, seen


# ---------------------------------------------------------------- edges of the definition
EW, EH = 40, 27


def cull_bounds(objs, n, g):
    out = (C.c_float * 14)()
    assert lib().rm_debug_cull_bounds(objs, n, C.byref(g), out) == 0
    return [float(v) for v in out]  # ok, centre xyz, R², soft R², box ok, lo xyz, hi xyz, lip


def test_empty_table_with_null_objects(renderer):
    cam = h.make_camera((0, 0, 5), (0, 0, -1), (0, 1, 0), 40.0, EW, EH, far=37.5)
    scene = (cam, None, 0, None, 0, h.make_globals())
    nd, ids, pos, _ = check_against_spec(renderer, scene, abi.default_settings(), EW, EH, "empty table")
    assert (ids == -1).all() and (bits(nd[..., 3]) == np.float32(37.5).view(np.uint32)).all()
    assert (bits(nd[..., :3]) == 0).all() and (bits(pos) == 0).all()


def full_table_scene(W, H):
    """RM_MAX_OBJECTS objects, every type 0…12 at least twice, on a 6×5 grid."""
    objs = []
    for k in range(abi.RM_MAX_OBJECTS):
        ty = k % 13
        sc = 0.55 if ty in (abi.RM_MANDELBULB, abi.RM_MENGERSPONGE, abi.RM_SIERPINSKI, abi.RM_MANDELBROT) else 1.0 + 0.03 * k
        M = h.translate(-3.75 + 1.5 * (k % 6), -2.4 + 1.2 * (k // 6), -0.1 * (k % 4)) @ h.rotation((1, 0.3 * k, 0.5), 0.37 * k) @ h.scale(sc, sc * 0.9, sc)
        objs.append(h.make_object(ty, model=M, scale_factor=0.9 * sc))
    cam = h.make_camera((0.2, 0.1, 9.0), (0, 0, -1), (0, 1, 0), 50.0, W, H)
    return cam, (abi.RmObject * len(objs))(*objs), len(objs), None, 0, h.make_globals(itime=2.0)


def test_table_of_rm_max_objects_with_every_type(renderer):
    scene = full_table_scene(EW, EH)
    assert scene[2] == abi.RM_MAX_OBJECTS and {scene[1][i].type for i in range(scene[2])} == set(range(13))
    s = abi.default_settings(maxSteps=96, fractalIters=6, mengerLevels=2)
    _, ids, _, _ = check_against_spec(renderer, scene, s, EW, EH, "30 objects")
    assert len(set(np.unique(ids).tolist()) - {-1}) >= 12 and ids.max() >= 24


@pytest.mark.parametrize("over", [{"maxSteps": 0}, {"maxSteps": 1}, {"fractalIters": 0}, {"mengerLevels": 0}], ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_degenerate_loop_bounds(renderer, over):
    for name, scene in (("table", directional_light_2(EW, EH)), ("bulb", h.scene_mandelbulb(EW, EH)), ("general bulb", moved_bulb_scene(EW, EH)),
                        ("sponge", SB.menger_scene(EW, EH)), ("full table", full_table_scene(EW, EH))):
        s = abi.default_settings(**{"maxSteps": 64, "fractalIters": 6, "mengerLevels": 2, **over})
        _, ids, _, _ = check_against_spec(renderer, scene, s, EW, EH, f"{name} {over}")
        if over.get("maxSteps") == 0:
            assert (ids == -1).all()  # no evaluation: closest stays at 1000000


def test_far_plane_through_an_object(renderer):
    """initialFar smaller than the object's far side: the rays near the silhouette pass far before they come within SURFACE_DIST."""
    for name, obj in (("sphere", h.make_object(abi.RM_SPHERE, model=h.scale(2, 2, 2), scale_factor=2.0)), ("bulb", h.make_object(abi.RM_MANDELBULB))):
        for far in (100.0, 3.8):
            cam = h.make_camera((0, 0, 4.5), (0, 0, -1), (0, 1, 0), 35.0, EW, EH, far=far)
            scene = (cam, (abi.RmObject * 1)(obj), 1, None, 0, h.make_globals())
            _, ids, _, _ = check_against_spec(renderer, scene, abi.default_settings(), EW, EH, f"{name} far {far}")
            hits = int((ids >= 0).sum())
            if far == 100.0:
                full = hits
        assert 0 < hits < full, (name, hits, full)  # the far plane took hits away


def test_camera_on_the_bounding_ball_and_a_staged_box(renderer):
    objs = (abi.RmObject * 5)(
        h.make_object(abi.RM_CUBE, model=h.translate(0, -1, 0) @ h.scale(14, 0.2, 6), scale_factor=0.2),
        h.make_object(abi.RM_SPHERE, model=h.translate(-4, -0.4, 0)),
        h.make_object(abi.RM_CONE, model=h.translate(-1.5, -0.4, 0.5) @ SB.rot_x(0.3)),
        h.make_object(abi.RM_CYLINDER, model=h.translate(1.5, -0.4, -0.5)),
        h.make_object(abi.RM_TORUS, model=h.translate(4.5, -0.3, 0.2) @ SB.rot_x(1.2) @ h.scale(1.5, 1.5, 1.5), scale_factor=1.5))
    g = h.make_globals()
    b = cull_bounds(objs, 5, g)
    assert b[0] == 1 and b[6] == 1, "the table must have its ball and its staged box"
    c, R = np.array(b[1:4]), np.sqrt(b[4])
    lo, hi = np.array(b[7:10]), np.array(b[10:13])
    cams = {"on the ball, along it": h.make_camera(tuple(c + R * np.array([0, 0.6, 0.8])), (1, -0.05, 0.0), (0, 1, 0), 60.0, EW, EH),
            "on the ball, into it": h.make_camera(tuple(c + R * np.array([0.6, 0, 0.8])), (-0.6, -0.1, -0.8), (0, 1, 0), 60.0, EW, EH),
            "on the box's top plane": h.make_camera((0.5, float(hi[1]), 3), (0, -0.2, -1), (0, 1, 0), 50.0, EW, EH),
            "inside the box": h.make_camera((0.2, 0.0, 1.5), (0.3, -0.2, -1), (0, 1, 0), 60.0, EW, EH),
            "far plane inside the box": h.make_camera((0, 0.3, 9), (0, 0, -1), (0, 1, 0), 40.0, EW, EH, far=8.0)}
    assert (lo < hi).all()
    hits = 0
    for name, cam in cams.items():
        _, ids, _, _ = check_against_spec(renderer, (cam, objs, 5, None, 0, g), abi.default_settings(), EW, EH, name)
        hits += int((ids >= 0).sum())
    assert hits > 0


@pytest.mark.parametrize("bump", [True, False])
def test_sierpinski_in_a_table_has_no_lipschitz_bound(renderer, bump):
    objs = (abi.RmObject * 3)(h.make_object(abi.RM_SIERPINSKI, model=h.scale(0.8, 0.8, 0.8), scale_factor=0.8),
                              h.make_object(abi.RM_SPHERE, model=h.translate(1.5, 0, 0)),
                              h.make_object(abi.RM_CUBE, model=h.translate(-1.4, 0.2, 0.3) @ h.rotation((1, 1, 0), 0.6)))
    g = h.make_globals()
    assert cull_bounds(objs, 3, g)[13] == float("inf")
    cam = h.make_camera((0.3, 0.6, 5.0), (-0.05, -0.12, -1), (0, 1, 0), 40.0, EW, EH)
    s = abi.default_settings(features=abi.RM_FEAT_WHITE_BACKGROUND | (abi.RM_FEAT_PERLIN_BUMP if bump else 0))
    _, ids, _, _ = check_against_spec(renderer, (cam, objs, 3, None, 0, g), s, EW, EH, f"sierpinski table bump {bump}")
    assert {0, 1, 2, -1} <= set(np.unique(ids).tolist())


@pytest.mark.parametrize("bump", [True, False])
def test_table_walk_with_and_without_bump(renderer, bump):
    scene = directional_light_2(EW, EH)
    assert np.isfinite(cull_bounds(scene[1], scene[2], scene[5])[13])
    s = abi.default_settings(features=abi.RM_FEAT_WHITE_BACKGROUND | (abi.RM_FEAT_PERLIN_BUMP if bump else 0))
    nd, ids, _, _ = check_against_spec(renderer, scene, s, EW, EH, f"table walk bump {bump}")
    other = gbuffer_guarded(renderer, tables_of(scene), abi.default_settings(features=0 if bump else abi.RM_FEAT_PERLIN_BUMP), EW, EH)
    assert (other[1] == ids).all() and (bits(other[0][..., 3]) == bits(nd[..., 3])).all()  # the bit moves no hit and no depth …
    assert (bits(other[0][..., :3]) != bits(nd[..., :3])).any()                              # … and does move normals


# ---------------------------------------------------------------- ragged frames, wider workgroups
RAGGED = [(1, 1), (3, 70), (65, 9), (97, 53)]


def ragged_case(kind, W, H, frames):
    """(scene, settings, cameras, globals) of the table-walk or the general-bulb frames at W×H."""
    if kind == "table":
        scene = directional_light_2(W, H)
        cams = [scene[0]] + [h.make_camera(p, l, (0, 1, 0), 45.0, W, H) for p, l in (((3, 4, 9), (-0.3, -0.35, -1)), ((-4, 2, 8), (0.4, -0.2, -1)))]
        return scene, abi.default_settings(), cams[:frames], scene[5]
    scene = moved_bulb_scene(W, H)
    cams = [h.make_camera(p, tuple(-v for v in p), (0, 1, 0), 30.0, W, H) for p in ((0, 0, 4.5), (1.0, 0.3, 4.3), (-1.2, 0.8, 4.0))]
    globs = [with_globals(scene[5], iTime=0.4 * f, power=8.0 - 0.5 * f) for f in range(frames)]
    return scene, abi.default_settings(fractalIters=8), cams[:frames], globs


@pytest.mark.parametrize("position", [True, False], ids=["position", "no-position"])
@pytest.mark.parametrize("frames", [1, 3])
@pytest.mark.parametrize("W,H", RAGGED)
@pytest.mark.parametrize("kind", ["table", "bulb"])
def test_ragged_frames(renderer, kind, W, H, frames, position):
    scene, s, cams, globs = ragged_case(kind, W, H, frames)
    check_against_spec(renderer, scene, s, W, H, f"{kind} {W}x{H}x{frames}", cameras=cams, globals_=globs, position=position)


_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import test_gpu_gbuffer as t
from raymarcher_amd import Renderer
r = Renderer(0)
out = {}
for W, H in ((65, 9), (97, 53)):
    for frames in (1, 3):
        scene, s, cams, globs = t.ragged_case("table", W, H, frames)
        nd, ids, pos, _ = t.check_against_spec(r, scene, s, W, H, f"child {W}x{H}x{frames}", cameras=cams, globals_=globs)
        out[f"nd_{W}_{H}_{frames}"], out[f"ids_{W}_{H}_{frames}"], out[f"pos_{W}_{H}_{frames}"] = nd, ids, pos
np.savez(sys.argv[2], **out)
print("ok")
"""


@pytest.mark.parametrize("wpb", [2, 4])
def test_waves_per_block(renderer, tmp_path, wpb):
    """Two and four waves side by side per workgroup (RM_WAVES_PER_BLOCK is read once per process: a fresh child process with a
    timeout of its own): the child's outputs equal the spec there and this process's outputs here, in every bit."""
    path = str(tmp_path / "child.npz")
    env = dict(os.environ, RM_WAVES_PER_BLOCK=str(wpb))
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, path], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), (p.returncode, p.stdout[-1000:], p.stderr[-3000:])
    child = np.load(path)
    for W, H in ((65, 9), (97, 53)):
        for frames in (1, 3):
            scene, s, cams, globs = ragged_case("table", W, H, frames)
            nd, ids, pos = gbuffer_guarded(renderer, tables_of(scene), s, W, H, cams, globs)
            key = f"{W}_{H}_{frames}"
            assert_bits(child["nd_" + key], nd, f"RM_WAVES_PER_BLOCK={wpb} {key} normalDepth")
            assert (child["ids_" + key] == ids).all()
            assert_bits(child["pos_" + key], pos, f"RM_WAVES_PER_BLOCK={wpb} {key} position")


# ---------------------------------------------------------------- back to back, the colour path, timing
def test_four_launches_back_to_back_on_one_stream(renderer):
    """A bulb table, a 28-object table, a sponge and the bulb again, launched without a synchronisation between them: every launch
    reads its own slot of the scene-block ring."""
    W, H = 48, 31
    rng = np.random.default_rng(5)
    objs = []
    while len(objs) != 28:
        objs = h.random_tablewalk_objects(rng, max_objects=28)
    big = (h.make_camera((0.3, 1.5, 6.0), (-0.03, -0.22, -1), (0, 1, 0), 55.0, W, H), (abi.RmObject * 28)(*objs), 28, None, 0, h.make_globals())
    sponge = SB.menger_scene(W, H)
    sponge[5].iTime = 7.5
    bulb = moved_bulb_scene(W, H)
    calls = [(bulb, abi.default_settings(fractalIters=8)), (big, abi.default_settings()), (sponge, abi.default_settings(mengerLevels=3)),
             (bulb, abi.default_settings(fractalIters=8))]
    launched = []
    for scene, s in calls:
        nd, c1 = h.guarded((1, H, W, 4), device=renderer.device)
        ids, c2 = h.guarded((1, H, W), torch.int32, INT_POISON, device=renderer.device)
        pos, c3 = h.guarded((1, H, W, 4), device=renderer.device)
        launched.append((nd, ids, pos, c1, c2, c3))
    for (scene, s), (nd, ids, pos, *_) in zip(calls, launched):  # nothing between the launches but the next launch
        renderer.render_gbuffer(tables_of(scene), s, W, H, out_normal_depth=nd, out_object_id=ids, out_position=pos)
    assert lib().rm_debug_last_path() == 11
    for k, ((scene, s), (nd, ids, pos, c1, c2, c3)) in enumerate(zip(calls, launched)):
        c1(), c2(), c3()
        snd, sids, spos = G.spec_gbuffer(scene[0], scene[1], scene[2], scene[5], s, W, H)
        assert_bits(nd.cpu().numpy()[0], snd, f"launch {k} normalDepth")
        assert (ids.cpu().numpy()[0] == sids).all(), f"launch {k} objectId"
        assert_bits(pos.cpu().numpy()[0], spos, f"launch {k} position")
    assert (launched[0][1].cpu().numpy() == launched[3][1].cpu().numpy()).all() and (launched[1][1].cpu().numpy() >= 0).any()


def counted_hits(renderer, scene, s, W, H):
    out = torch.empty((H, W, 4), dtype=torch.float32, device=renderer.device)
    cnt = abi.RmCounters()
    torch.cuda.synchronize(renderer.device)
    st = lib().rm_render_counted_ex(*tables_of(scene).args(s), W, H, 0, H, C.c_void_p(out.data_ptr()), None, abi.RM_COUNT_EXECUTED, C.byref(cnt))
    assert st == abi.RM_OK, lib().rm_last_error().decode()
    return int(cnt.hitPixels)


def test_hit_count_equals_the_colour_paths(renderer):
    """(object_id >= 0).sum() is hitPixels of the production colour kernel (RM_COUNT_EXECUTED) on the two scenes of
    test_spec_hits_what_the_oracle_hits and on four random table walks without an emissive object."""
    W, H = 64, 36
    cases = [("directional_light_2", directional_light_2(W, H), abi.default_settings()), ("mandelbulb", h.scene_mandelbulb(W, H), abi.default_settings())]
    rng = np.random.default_rng(20261021)
    for i in range(4):
        scene, s = SB.random_tablewalk_case(rng, W, H)
        assert not any(scene[1][k].isEmissive for k in range(scene[2]))
        cases.append((f"random table walk {i}", scene, s))
    for name, scene, s in cases:
        _, ids, _ = gbuffer_guarded(renderer, tables_of(scene), s, W, H)
        assert int((ids >= 0).sum()) == counted_hits(renderer, scene, s, W, H), name


def test_timing_counts_one_launch_all_stage_1(renderer):
    L = lib()
    W, H = 64, 40
    sponge = SB.menger_scene(W, H)  # the sponge prologue runs ahead of the timed launch
    for scene, s, frames in ((sponge, abi.default_settings(mengerLevels=3), 3), (directional_light_2(W, H), abi.default_settings(), 1)):
        try:
            assert L.rm_set_timing(1) == 0
            renderer.render_gbuffer(tables_of(scene), s, W, H, cameras=[scene[0]] * frames, position=True)
            assert L.rm_debug_last_path() == 11 and L.rm_debug_last_split() == 0
            torch.cuda.synchronize(renderer.device)
            total, stages, k = C.c_double(), (C.c_double * 4)(), C.c_int()
            assert L.rm_get_stage_timing(C.byref(total), stages, C.byref(k)) == 0
            assert k.value == 1 and total.value > 0.0
            assert stages[0] == 0.0 and stages[1] == total.value and stages[2] == 0.0 and stages[3] == 0.0
        finally:
            L.rm_set_timing(0)
