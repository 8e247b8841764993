"""rm_render_animated / Renderer.render_animated on the GPU.  An animated pixel is defined by things the contract already has: block
b's frame is the oracle's render of block b's camera, globals, object table and light table, and output frame f is `accumulate`
(test_gpu_accumulate.py: the header's sequential sum) of blocks f·n … f·n + n − 1.  Every call below is compared with that on the
uint32 view, BrightColor included, no tolerance and no excluded pixel.  Frames are 97×53 (partial tiles on both axes) unless a shape
is named."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as h
import scene_builders as SB
from helpers import assert_bit_equal, tables_of, with_globals
from test_gpu_accumulate import accumulate, oracle_accumulated
from raymarcher_amd import abi, lib, translated_objects
from raymarcher_amd.render import shutter_globals

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(ROOT, "tests", "golden", "scenes")
W0, H0 = 97, 53


def clone(x):
    y = type(x)()
    C.memmove(C.byref(y), C.byref(x), C.sizeof(x))
    return y


def table(struct, items):
    return (struct * max(len(items), 1))(*[clone(i) for i in items])


def split(flat, count, blocks):
    """A flat ctypes array of blocks·count structs → `blocks` lists of `count`."""
    return [[flat[b * count + i] for i in range(count)] for b in range(blocks)]


def oracle_animated(scene, cams, globs, s, W, H, n, objects=None, lights=None, textures=None, **resources):
    """(fragColor, BrightColor) of every output frame by the definition: block b through the oracle with ITS tables, then the sum."""
    outs, brs = [], []
    for f in range(len(cams) // n):
        S, Sb = [], []
        for j in range(n):
            b = f * n + j
            objs = table(abi.RmObject, objects[b]) if objects is not None else scene[1]
            lts = table(abi.RmLight, lights[b]) if lights is not None else scene[3]
            g = globs[b] if isinstance(globs, (list, tuple)) else globs
            a, br = h.oracle_render((cams[b], objs, scene[2], lts, scene[4], g), s, W, H, bright=True, threads=16, textures=textures,
                                    **resources)
            assert np.isfinite(a).all() and np.isfinite(br).all(), "the oracle's sub-frame is not finite: choose another case"
            S.append(a)
            Sb.append(br)
        outs.append(accumulate(np.stack(S)))
        brs.append(accumulate(np.stack(Sb)))
    return outs, brs


def anim_vs_oracle(renderer, scene, s, W, H, cams, n, objects=None, lights=None, globs=None, textures=None, what="", **resources):
    """One call against the definition.  objects / lights: None or one list of structs per block."""
    t = tables_of(scene, **resources)
    if textures:
        t.textures = textures
    globs = scene[5] if globs is None else globs
    out, br = renderer.render_animated(t, s, W, H, cams, n, objects=objects, lights=lights, globals_=globs, bright=True)
    assert lib().rm_debug_last_path() == 10 and lib().rm_debug_last_split() == 0
    frames = len(cams) // n
    assert tuple(out.shape) == (frames, H, W, 4) and tuple(br.shape) == (frames, H, W, 4)
    out, br = out.cpu().numpy(), br.cpu().numpy()
    ref, ref_b = oracle_animated(scene, cams, globs, s, W, H, n, objects, lights, textures=textures, **resources)
    for f in range(frames):
        assert_bit_equal(out[f], ref[f], f"{what} n {n} {W}x{H} frame {f}")
        assert_bit_equal(br[f], ref_b[f], f"{what} n {n} {W}x{H} frame {f} bright")
    return out


def moving_sphere(scene, blocks, reach=6.0):
    """The tables of `scene` with object 0 (a sphere) translated by up to `reach` world units along +x, then up, across the blocks."""
    offs = [(reach * b / max(blocks - 1, 1), 0.5 * b / max(blocks - 1, 1), 0.0) for b in range(blocks)]
    return split(translated_objects(list(scene[1]), 0, offs), scene[2], blocks)


# ---------------------------------------------------------------- 1. a moving primitive
def compact_scene(W, H):
    """Four primitives close together (a small floor slab, so that the cull ball and box of the table are tight) and two lights."""
    cam = h.make_camera((1.5, 2.0, 10.0), (0, -0.15, -1), (0, 1, 0), 50.0, W, H)
    objs = (abi.RmObject * 4)(
        h.make_object(abi.RM_SPHERE, model=h.translate(-1.5, 0.2, 0) @ h.scale(1.2, 1.2, 1.2), scale_factor=1.2, ambient=(.1, .1, .1),
                      diffuse=(.8, .2, .2), specular=(1, 1, 1), shininess=30),
        h.make_object(abi.RM_CUBE, model=h.translate(0, -1.0, 0) @ h.scale(3, 0.5, 3), scale_factor=0.5, ambient=(.2, .2, .2),
                      diffuse=(.6, .6, .5), specular=(.3, .3, .3), shininess=5),
        h.make_object(abi.RM_TORUS, model=h.translate(0.8, 0.3, -1.0) @ h.scale(1.5, 1.5, 1.5), scale_factor=1.5, ambient=(.1, .2, .1),
                      diffuse=(.3, .9, .3), specular=(1, 1, 1), shininess=10),
        h.make_object(abi.RM_CYLINDER, model=h.translate(1.6, 0.0, 0.8) @ h.scale(0.8, 1.4, 0.8), scale_factor=0.8, ambient=(.1, .1, .2),
                      diffuse=(.3, .4, .9), specular=(.6, .6, .6), shininess=15))
    lights = (abi.RmLight * 2)(h.make_light(abi.RM_LIGHT_DIRECTIONAL, (1, 1, 1), (-0.5, -1, -0.4)),
                               h.make_light(abi.RM_LIGHT_POINT, (.8, .8, 1), pos=(-3, 4, 3), func=(0.6, 0.05, 0.0)))
    return cam, objs, 4, lights, 2, h.make_globals()


def cull_bounds(objs, g):
    out = (C.c_float * 14)()
    assert lib().rm_debug_cull_bounds(table(abi.RmObject, objs), len(objs), C.byref(g), out) == 0
    return [float(v) for v in out]  # ok, centre xyz, R², soft R², box ok, lo xyz, hi xyz, Lipschitz bound


@pytest.mark.parametrize("n", [1, 3, 8])
def test_moving_sphere_leaves_block_0s_bounds(renderer, n):
    """A sphere among four primitives with two lights moves 6 world units over the blocks of two frames: it ends outside the cull
    ball and box of block 0's table, so the bounds, the evaluation records and the per-object balls must be each block's own.  The
    tables come from translated_objects."""
    W, H = W0, H0
    scene = compact_scene(W, H)
    blocks = 2 * n
    objects = moving_sphere(scene, blocks)
    b0 = cull_bounds(objects[0], scene[5])
    assert b0[0] == 1.0 and b0[6] == 1.0  # block 0 has a ball and a box
    m = np.array(objects[-1][0].invModel[:], dtype=np.float64).reshape(4, 4).T
    c = -np.linalg.inv(m[:3, :3]) @ m[:3, 3]  # the sphere's centre in the last block
    assert np.linalg.norm(c - np.array(b0[1:4])) - 0.6 > np.sqrt(b0[4]) and c[0] - 0.6 > b0[10]  # the whole sphere (radius 0.6) is outside both
    out = anim_vs_oracle(renderer, scene, abi.default_settings(enableSoftShadow=1, enableAmbientOcclusion=1), W, H, [scene[0]] * blocks, n,
                         objects=objects, what="moving sphere")
    assert np.abs(out[0] - out[1]).max() > 0.05  # the frames differ


# ---------------------------------------------------------------- 2. moving lights only
def test_moving_lights_with_one_object_table(renderer):
    W, H, n, frames = W0, H0, 3, 2
    scene = SB.reflect_refract_scene(W, H)
    blocks = n * frames
    lights = []
    for b in range(blocks):
        a = 0.5 * b
        lights.append([h.make_light(abi.RM_LIGHT_SPOT, (1, 1, .9), direction=(-0.3 + 0.15 * b, -1, -0.4), pos=(1.0, 5.0, 2.5),
                                    func=(0.5, 0.02, 0.0), angle=0.6, penumbra=0.25),
                       h.make_light(abi.RM_LIGHT_POINT, (.8, .8, 1), pos=(-3 + 4 * np.sin(a), 4, 3 * np.cos(a)), func=(0.6, 0.05, 0.0))])
    out = anim_vs_oracle(renderer, scene, abi.default_settings(enableSoftShadow=1, enableAmbientOcclusion=1), W, H, [scene[0]] * blocks, n,
                         lights=lights, what="moving lights")
    assert np.abs(out[0] - out[1]).max() > 0.02
    # light kinds may change between blocks too
    lights[4][0] = h.make_light(abi.RM_LIGHT_DIRECTIONAL, (1, 1, 1), (-0.5, -1, -0.4))
    anim_vs_oracle(renderer, scene, abi.default_settings(), W, H, [scene[0]] * blocks, n, lights=lights, what="a light changes kind")


# ---------------------------------------------------------------- 3. the restage pattern
def restage_pattern(renderer, W, H):
    """Tables A, A, B, B, A over n = 5, two frames (the second B, A, A, B, B): equal neighbours keep the staged table, unequal ones
    must replace it, and going back to A must not find B."""
    scene = SB.reflect_refract_scene(W, H)
    A = [clone(o) for o in scene[1]]
    B = split(translated_objects(A, 0, [(2.5, 0.8, 0.5)]), 4, 1)[0]
    B[3].cDiffuse[0], B[3].type = 0.9, abi.RM_CYLINDER  # a material and a type change as well
    objects = [A, A, B, B, A, B, A, A, B, B]
    cams = [h.make_camera((0.5, 1.4, 7.0), (0, -0.2, -1), (0, 1, 0), 45.0, W, H)] * 10
    anim_vs_oracle(renderer, scene, abi.default_settings(enableReflection=1), W, H, cams, 5, objects=objects, what="A A B B A")


def test_restage_pattern(renderer):
    restage_pattern(renderer, W0, H0)


_CHILD = r'''
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_animated as t
from raymarcher_amd import Renderer
r = Renderer(0)
t.restage_pattern(r, 65, 9)
t.restage_pattern(r, 97, 53)
print("ok")
'''


def test_restage_pattern_with_four_waves_per_workgroup():
    """RM_WAVES_PER_BLOCK is read once per process: a child.  At 65×9 the last workgroup of a row has one live wave and three wholly
    outside the frame, which share its barriers."""
    env = dict(os.environ, RM_WAVES_PER_BLOCK="4")
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), (p.returncode, p.stdout[-1000:], p.stderr[-3000:])


# ---------------------------------------------------------------- 4. the class of the call is the union of its blocks'
def test_union_reflective_object_in_one_sub_frame_only(renderer):
    W, H = W0, H0
    scene = SB.reflect_refract_scene(W, H)
    dull = [clone(o) for o in scene[1]]
    for o in dull:
        for k in range(3):
            o.cReflective[k] = 0.0
    objects = [dull, [clone(o) for o in scene[1]], dull, dull]  # secondary rays fire in sub-frame 1 of frame 0 alone
    anim_vs_oracle(renderer, scene, abi.default_settings(enableReflection=1, numReflection=2), W, H, [scene[0]] * 4, 2, objects=objects,
                   what="reflective in one sub-frame")


def test_union_textured_object_in_one_block_only(renderer):
    W, H = W0, H0
    scene = SB.textured_scene(W, H)
    bare = [clone(o) for o in scene[1]]
    for o in bare:
        o.texLoc = -1
    objects = [bare, bare, [clone(o) for o in scene[1]], bare]
    for n in (1, 2):
        anim_vs_oracle(renderer, scene, abi.default_settings(), W, H, [scene[0]] * 4, n, objects=objects, textures=SB.synthetic_textures(),
                       what="textured in one block")


def test_union_area_light_in_a_later_light_table_only(renderer):
    W, H = W0, H0
    scene, s, res = SB.resource_case("area_light", W, H)
    point = [h.make_light(abi.RM_LIGHT_POINT, (1.0, 0.9, 0.6), pos=(0.3, 2.2, -1.0), func=(0.7, 0.05, 0)), clone(scene[3][1])]
    lights = [point, point, [clone(scene[3][0]), clone(scene[3][1])]]
    dark = [clone(o) for o in scene[1]]
    dark[3].isEmissive = 0  # the rectangle glows only where its light is an area light
    objects = [dark, dark, [clone(o) for o in scene[1]]]
    anim_vs_oracle(renderer, scene, s, W, H, [scene[0]] * 3, 3, objects=objects, lights=lights, what="area light in block 2", **res)


def test_union_bulb_in_block_0_and_sphere_in_block_1(renderer):
    W, H = W0, H0
    scene = h.scene_mandelbulb(W, H)
    sphere = h.make_object(abi.RM_SPHERE, model=h.scale(2, 2, 2), scale_factor=2.0, ambient=(.2, .2, .2), diffuse=(.8, .4, .3),
                           specular=(1, 1, 1), shininess=20.0)
    objects = [[clone(scene[1][0])], [sphere]]
    s = abi.default_settings(fractalIters=12)
    for n in (1, 2):
        anim_vs_oracle(renderer, scene, s, W, H, [scene[0]] * 2, n, objects=objects, what="bulb then sphere")


def test_union_plain_bulb_then_the_same_bulb_translated(renderer):
    W, H = W0, H0
    scene = h.scene_mandelbulb(W, H)
    objects = split(translated_objects(list(scene[1]), 0, [(0, 0, 0), (0.4, -0.2, 0.3)]), 1, 2)
    assert lib().rm_debug_bulb_plain(table(abi.RmObject, objects[0]), 1, C.byref(scene[5])) == 1
    assert lib().rm_debug_bulb_plain(table(abi.RmObject, objects[1]), 1, C.byref(scene[5])) == 0
    s = abi.default_settings(fractalIters=12)
    for n in (1, 2):
        anim_vs_oracle(renderer, scene, s, W, H, [scene[0]] * 2, n, objects=objects, what="plain bulb then moved")


# ---------------------------------------------------------------- 5. a Menger sponge in a later block only
@pytest.mark.parametrize("n", [1, 3])
def test_menger_sponge_in_a_later_block_only(renderer, n):
    """Block 0 holds a cube in the sponge's place: the sponge's uniforms (computed on the device per block, from its iTime) must be
    there for the blocks that do hold one."""
    W, H = W0, H0
    scene = SB.menger_scene(W, H)
    cube = clone(scene[1][0])
    cube.type = abi.RM_CUBE
    objects = [[cube], [clone(scene[1][0])], [clone(scene[1][0])]]
    globs = [with_globals(scene[5], iTime=t) for t in (2.9, 3.1, 3.3)]  # the sponge opens between iTime 2.74 and 3.54
    anim_vs_oracle(renderer, scene, abi.default_settings(mengerLevels=3, enableReflection=1), W, H, [scene[0]] * 3, n, objects=objects,
                   globs=globs, what="sponge from block 1")


# ---------------------------------------------------------------- 6. exact equalities
@pytest.mark.parametrize("n", [1, 4])
def test_shared_tables_are_render_accumulated_and_repeats_change_nothing(renderer, n):
    W, H, frames = W0, H0, 2
    scene = SB.reflect_refract_scene(W, H)
    s = abi.default_settings(enableReflection=1, enableSoftShadow=1)
    t = tables_of(scene)
    blocks = frames * n
    cams = [h.make_camera((0.3 * b, 1.2, 5), (0, -0.2, -1), (0, 1, 0), 40.0, W, H) for b in range(blocks)]
    globs = [with_globals(scene[5], iTime=0.2 * b) for b in range(blocks)]
    a, ab = renderer.render_accumulated(t, s, W, H, cams, n, globals_=globs, bright=True)
    one, one_b = renderer.render_animated(t, s, W, H, cams, n, globals_=globs, bright=True)
    assert lib().rm_debug_last_path() == 10
    assert SB.ieq(one, a) and SB.ieq(one_b, ab)
    rep_o, rep_l = [list(scene[1])] * blocks, [list(scene[3])] * blocks
    for kw in (dict(objects=rep_o), dict(lights=rep_l), dict(objects=rep_o, lights=rep_l)):
        rep, rep_b = renderer.render_animated(t, s, W, H, cams, n, globals_=globs, bright=True, **kw)
        assert SB.ieq(rep, a) and SB.ieq(rep_b, ab), sorted(kw)
    if n == 1:
        bt, bt_b = renderer.render_batch(t, s, W, H, cams, globals_=globs, bright=True)
        assert SB.ieq(one, bt) and SB.ieq(one_b, bt_b)


def test_one_sub_frame_with_tables_per_frame_is_rm_render_res(renderer):
    from raymarcher_amd.render import SceneTables
    W, H, frames = W0, H0, 4
    scene = SB.reflect_refract_scene(W, H)
    s = abi.default_settings(enableSoftShadow=1)
    objects = moving_sphere(scene, frames, reach=3.0)
    lights = [[clone(scene[3][0]), h.make_light(abi.RM_LIGHT_POINT, (.8, .8, 1), pos=(-3 + f, 4, 3), func=(0.6, 0.05, 0.0))] for f in range(frames)]
    out, br = renderer.render_animated(tables_of(scene), s, W, H, [scene[0]] * frames, 1, objects=objects, lights=lights, bright=True)
    for f in range(frames):
        tf = SceneTables(scene[0], table(abi.RmObject, objects[f]), 4, table(abi.RmLight, lights[f]), 2, scene[5])
        one, one_b = renderer.render(tf, s, W, H, bright=True)
        assert SB.ieq(out[f], one) and SB.ieq(br[f], one_b), f


# ---------------------------------------------------------------- 7. write coverage
@pytest.mark.parametrize("W,H", [(1, 1), (3, 70), (65, 9), (97, 53)])
@pytest.mark.parametrize("frames", [1, 3])
def test_every_word_is_written_and_nothing_else(renderer, W, H, frames):
    scene = SB.reflect_refract_scene(W, H)
    s = abi.default_settings(enableReflection=1)
    t = tables_of(scene)
    for n in (1, 3):
        blocks = frames * n
        objects = moving_sphere(scene, blocks, reach=1.0)
        cams = [scene[0]] * blocks
        out, c1 = h.guarded((frames, H, W, 4), device=renderer.device)
        br, c2 = h.guarded((frames, H, W, 4), device=renderer.device)
        renderer.render_animated(t, s, W, H, cams, n, objects=objects, out=out, out_bright=br)
        c1()
        c2()
        # d_bright = NULL: the same frames, and a neighbouring poisoned allocation is left alone
        out2, c3 = h.guarded((frames, H, W, 4), device=renderer.device)
        spare = h.Guarded((frames, H, W, 4), renderer.torch.float32, h.FLOAT_POISON, renderer.device)
        renderer.render_animated(t, s, W, H, cams, n, objects=objects, out=out2)
        c3()
        assert SB.ieq(out2, out)
        assert bool(spare._unwritten(spare.buf).all()), "a launch without d_bright wrote outside d_rgba"


# ---------------------------------------------------------------- 8. schedule and state
def test_timing_counts_one_launch_all_stage_1(renderer):
    L = lib()
    W, H, n = 64, 40, 3
    scene = SB.menger_scene(W, H)
    cube = clone(scene[1][0])
    cube.type = abi.RM_CUBE
    objects = [[cube], [clone(scene[1][0])], [clone(scene[1][0])]] * 2  # the sponge prologue runs ahead of the timed launch
    for sub in (1, n):
        try:
            assert L.rm_set_timing(1) == 0
            renderer.render_animated(tables_of(scene), abi.default_settings(mengerLevels=3), W, H, [scene[0]] * (2 * n), sub, objects=objects,
                                     globals_=shutter_globals(scene[5], 0.0, 1.0, 2 * n))
            assert L.rm_debug_last_path() == 10 and L.rm_debug_last_split() == 0
            renderer.torch.cuda.synchronize(renderer.device)
            total, stages, k = C.c_double(), (C.c_double * 4)(), C.c_int()
            assert L.rm_get_stage_timing(C.byref(total), stages, C.byref(k)) == 0
            assert k.value == 1 and total.value > 0.0
            assert stages[0] == 0.0 and stages[1] == total.value and stages[2] == 0.0 and stages[3] == 0.0
        finally:
            L.rm_set_timing(0)


def test_animated_launch_leaves_the_single_frame_tuners_alone(renderer):
    """The sequence of test_gpu_accumulate, with an animated launch of the same picture in the middle."""
    from raymarcher_amd import Scene
    L = lib()
    W, H = 512, 320
    t = Scene(path=os.path.join(SCENES, "lighting", "directional_light_2.json")).tables(W, H)
    s = abi.default_settings(enableSoftShadow=1, enableAmbientOcclusion=1)
    other = tables_of((h.make_camera((0, 1, 8), (0, -0.1, -1), (0, 1, 0), 40.0, W, H), t.objects, t.num_objects, t.lights, t.num_lights,
                       t.globals_))
    objs = [t.objects[i] for i in range(t.num_objects)]
    objects = split(translated_objects(objs, 0, [(0, 0, 0), (0.5, 0, 0), (0, 0, 0), (0, 0.5, 0)]), t.num_objects, 4)

    def sequence(anim_after=None):
        renderer.render(other, s, W, H)  # another picture of the same size: the picture below starts afresh
        splits, frames = [], []
        for k in range(12):
            if k == anim_after:
                renderer.render_animated(t, s, W, H, [other.camera, t.camera, t.camera, other.camera], 2, objects=objects)
                assert L.rm_debug_last_path() == 10 and L.rm_debug_last_split() == 0
            frames.append(renderer.render(t, s, W, H).clone())
            assert L.rm_debug_last_path() == 1
            splits.append(L.rm_debug_last_split())
        return splits, frames

    try:
        assert L.rm_debug_set_tile_shape(3) == 0  # no timed shape tuning: the sequence depends on the tile-order state alone
        assert L.rm_debug_set_light_split(32) == 0  # split a settled picture without measuring
        plain, frames = sequence()
        assert plain[0] == 0 and plain[-1] > 0, plain  # it settles, then splits
        again, frames2 = sequence(anim_after=plain.index(plain[-1]) + 1)
        assert again == plain
        assert all(SB.ieq(a, frames[0]) for a in frames + frames2)
    finally:
        L.rm_debug_set_tile_shape(-1)
        L.rm_debug_set_light_split(-1)


def test_back_to_back_launches_with_different_tables_on_one_stream(renderer):
    """Two calls in flight on one stream: staging the second (another slot of the ring, other tables) does not disturb the first."""
    import torch
    W = H = 24
    n = 4
    scene = SB.reflect_refract_scene(W, H)
    s = abi.default_settings()
    t = tables_of(scene)
    fa, fb = 60, 10
    obj_a = moving_sphere(scene, fa * n, reach=4.0)
    obj_b = split(translated_objects(list(scene[1]), 1, [(0, 0.05 * b, 0) for b in range(fb * n)]), 4, fb * n)
    cams_a, cams_b = [scene[0]] * (fa * n), [scene[0]] * (fb * n)
    stream = torch.cuda.Stream(device=renderer.device)
    torch.cuda.synchronize(renderer.device)
    with torch.cuda.stream(stream):
        a = renderer.render_animated(t, s, W, H, cams_a, n, objects=obj_a)
        b = renderer.render_animated(t, s, W, H, cams_b, n, objects=obj_b)
    stream.synchronize()
    Sa = renderer.render_animated(t, s, W, H, cams_a, 1, objects=obj_a).cpu().numpy()
    Sb = renderer.render_animated(t, s, W, H, cams_b, 1, objects=obj_b).cpu().numpy()
    assert np.isfinite(Sa).all() and np.isfinite(Sb).all()
    a, b = a.cpu().numpy(), b.cpu().numpy()
    for f in range(fa):
        assert_bit_equal(a[f], accumulate(Sa[f * n:(f + 1) * n]), f"first launch, frame {f}")
    for f in range(fb):
        assert_bit_equal(b[f], accumulate(Sb[f * n:(f + 1) * n]), f"second launch, frame {f}")
    assert np.abs(a[0] - a[-1]).max() > 0.02
    # and a sample of both against the oracle
    for got, cams, objects, f in ((a, cams_a, obj_a, fa - 1), (b, cams_b, obj_b, 3)):
        ref, _ = oracle_animated(scene, cams[f * n:(f + 1) * n], scene[5], s, W, H, n, objects[f * n:(f + 1) * n])
        assert_bit_equal(got[f], ref[0], f"frame {f} against the oracle")


def test_host_output_pointer_is_refused_and_hip_stays_clean(renderer):
    L = lib()
    W, H = 16, 8
    scene = SB.reflect_refract_scene(W, H)
    cams = (abi.RmCamera * 4)(*[scene[0]] * 4)
    stacked = translated_objects(list(scene[1]), 0, [(0.1 * b, 0, 0) for b in range(4)])
    host = np.zeros((2, H, W, 4), dtype=np.float32)
    st = L.rm_render_animated(cams, C.byref(scene[5]), 1, stacked, 4, 4, scene[3], 2, 1, 2, 2, C.byref(abi.default_settings()), None, W, H,
                              C.c_void_p(host.ctypes.data), None, None)
    assert st == abi.RM_ERR_INVALID_ARGUMENT and "not device-accessible" in L.rm_last_error().decode()
    out = renderer.render_animated(tables_of(scene), abi.default_settings(), W, H, [scene[0]] * 4, 2, objects=stacked)  # a following render succeeds
    renderer.torch.cuda.synchronize(renderer.device)
    assert bool(renderer.torch.isfinite(out).all())


# ---------------------------------------------------------------- 9. render_sequence(..., objects=…)
def test_render_sequence_with_object_tables_equals_the_oracle_chain(renderer):
    W, H, N, n = 75, 45, 2, 3
    scene = SB.reflect_refract_scene(W, H)
    for li in scene[3]:
        li.color[0] *= 2.5; li.color[1] *= 2.5; li.color[2] *= 2.5  # over-exposed: BrightColor is populated
    s = abi.default_settings(enableReflection=1)
    cams = [scene[0]] * (N * n)
    stacked = translated_objects(list(scene[1]), 0, [(0.25 * b, 0.1 * b, 0) for b in range(N * n)])
    post = abi.RmPostSettings(**{"exposure": 1.0, **SB.POST_CASES["bloom_hdr_fxaa"]})
    imgs = renderer.render_sequence(tables_of(scene), s, W, H, cams, post=post, accumulate=n, objects=stacked)
    assert lib().rm_debug_last_path() == 10
    assert tuple(imgs.shape) == (N, H, W, 4) and imgs.dtype == renderer.torch.uint8
    imgs = imgs.cpu().numpy()
    frag, bright = oracle_animated(scene, cams, scene[5], s, W, H, n, split(stacked, 4, N * n))
    assert bright[0][..., :3].max() > 1.0
    for f in range(N):
        ref = h.oracle_post(frag[f], bright[f], post)
        exp = (np.clip(ref[::-1], 0, 1) * np.float32(255.0) + np.float32(0.5)).astype(np.uint8)
        assert (imgs[f] == exp).all(), f"frame {f}: {(imgs[f] != exp).sum()} bytes differ"
    # without accumulate: one image per camera, each its own table
    per = renderer.render_sequence(tables_of(scene), s, W, H, cams, objects=stacked)
    assert lib().rm_debug_last_path() == 10 and tuple(per.shape) == (N * n, H, W, 4)
    # without the keywords the call is what it was
    bare = renderer.render_sequence(tables_of(scene), s, W, H, cams, post=post)
    assert lib().rm_debug_last_path() == 6 and tuple(bare.shape) == (N * n, H, W, 4)
