"""Write coverage of every render path: each output goes into a freshly poisoned buffer between two guard bands (helpers.guarded),
so a pixel a launch never writes (it still holds the signalling-NaN poison) and a write past either end of the caller's rows (it
changes a guard) both fail, whatever an earlier frame or test left in the allocator's blocks.  Every frame is also compared bit
for bit with the oracle — a repeated picture with its oracle-checked first frame, each repeat in its own fresh buffer.  The
last part keeps frames, batches and the scene-block rings in flight on several streams without synchronising in between."""
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as h
import scene_builders as SB
from helpers import tables_of
from scene_builders import ieq
from raymarcher_amd import abi, lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (3, 70), (65, 9), (636, 388)]  # neither 8×8 nor 4×16 tiles divide any of them
SHAPES = (3, 2)  # rm_debug_set_tile_shape: 8×8, 4 wide × 16 tall


def single_object_scene(W, H):
    cam = h.make_camera((0, 1.0, 5), (0, -0.2, -1), (0, 1, 0), 45.0, W, H)
    objs = (abi.RmObject * 1)(h.make_object(abi.RM_TORUS, model=h.rotation((1, 0, 0), 0.7) @ h.scale(1.5, 1.5, 1.5), scale_factor=1.5,
                                            ambient=(.1, .1, .1), diffuse=(.8, .5, .3), specular=(1, 1, 1), shininess=20))
    lights = (abi.RmLight * 2)(h.make_light(abi.RM_LIGHT_DIRECTIONAL, (1, 1, 1), (-0.4, -1, -0.5)),
                               h.make_light(abi.RM_LIGHT_POINT, (.9, .8, .7), pos=(3, 4, 4), func=(0.7, 0.04, 0.0)))
    return cam, objs, 1, lights, 2, h.make_globals()


def kernel_class(name, W, H):
    """name → (scene, settings, resources) of one render_kernel class."""
    if name == "bulb_plain":
        return h.scene_mandelbulb(W, H), abi.default_settings(fractalIters=10), {}
    if name == "bulb_general":  # a Julia seed: the general form of the bulb kernel, with the shadow pool
        return SB.bulb_scene(W, H, nl=4, julia=(0.35, -0.2)), abi.default_settings(fractalIters=10), {}
    if name == "table":
        return SB.all_primitives_scene(W, H), abi.default_settings(maxSteps=96, enableSoftShadow=1), {}
    if name == "table_single":  # one object: the table walk's single-object fast path
        return single_object_scene(W, H), abi.default_settings(enableAmbientOcclusion=1), {}
    if name == "table_sec":  # secondary rays compiled in and firing
        return SB.reflect_refract_scene(W, H), abi.default_settings(enableReflection=1, enableRefraction=1, numReflection=2), {}
    if name == "layers":
        return SB.env_scene(W, H), abi.default_settings(features=SB.ENV_ALL, maxSteps=64), {}
    if name == "textures":
        return SB.textured_scene(W, H), abi.default_settings(), {"textures": SB.synthetic_textures()}
    if name == "skybox":
        return SB.resource_case("skybox_reflect", W, H)
    if name == "mandelbrot_2d":
        sc = h.scene_mandelbulb(W, H)
        return sc[:5] + (h.make_globals(two_d=1),), abi.default_settings(), {}
    raise KeyError(name)


CLASSES = ["bulb_plain", "bulb_general", "table", "table_single", "table_sec", "layers", "textures", "skybox", "mandelbrot_2d"]
BIG_CLASSES = {"bulb_plain", "bulb_general", "table", "table_single"}  # at 636×388 (the oracle's time stays small)


def check_class(renderer, name, W, H, shapes=SHAPES):
    """Frame and BrightColor of one class into guarded buffers, each tile shape pinned, against the oracle."""
    scene, s, res = kernel_class(name, W, H)
    ref, ref_b = h.oracle_render(scene, s, W, H, bright=True, threads=16, **res)
    t = tables_of(scene, res)
    try:
        for shape in shapes:
            assert lib().rm_debug_set_tile_shape(shape) == 0
            out, br = h.render_guarded(renderer, t, s, W, H, bright=True)
            h.assert_bit_equal(out.cpu().numpy(), ref, f"{name} {W}x{H} shape {shape}")
            h.assert_bit_equal(br.cpu().numpy(), ref_b, f"{name} {W}x{H} shape {shape} bright")
    finally:
        lib().rm_debug_set_tile_shape(-1)


@pytest.mark.parametrize("name,W,H", [(n, W, H) for n in CLASSES for W, H in SIZES if W * H < 20000 or n in BIG_CLASSES])
def test_every_kernel_class_writes_each_pixel_of_ragged_frames(renderer, name, W, H):
    check_class(renderer, name, W, H)


_CHILD = r'''
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_write_coverage as t
from raymarcher_amd import Renderer
r = Renderer(0)
for name in t.CLASSES:
    for W, H in ((3, 70), (65, 9), (1, 1)):
        t.check_class(r, name, W, H)
for name in ("bulb_plain", "table"):
    t.check_class(r, name, 636, 388)
t.test_row_ranges_off_tile_boundaries(r)
print("ok")
'''


@pytest.mark.parametrize("wpb", [2, 4])
def test_waves_per_block(wpb):
    """Two and four waves side by side per workgroup (RM_WAVES_PER_BLOCK is read once per process: a child process)."""
    env = dict(os.environ, RM_WAVES_PER_BLOCK=str(wpb))
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), (p.returncode, p.stdout[-1000:], p.stderr[-3000:])


# ---------------------------------------------------------------- tile orders
def test_every_tile_order_writes_each_tile(renderer):
    """≥ 2048 tiles: raster order, the geometric order of a new picture, cost-ordered repeats, the settled order (frames past
    RM_TILE_ORDER_SETTLE) and the raster fallback of an object without a bounding ball — each frame in a fresh buffer."""
    L = lib()
    W, H = 640, 384  # 3840 8×8 tiles
    prim = SB.all_primitives_scene(W, H)
    sier = (prim[0], (abi.RmObject * 2)(h.make_object(abi.RM_SIERPINSKI, model=h.scale(0.8, 0.8, 0.8), scale_factor=0.8,
                                                      diffuse=(.8, .6, .3)),
                                        h.make_object(abi.RM_SPHERE, model=h.translate(1.5, 0, 0))), 2) + prim[3:]
    moved = (h.make_camera((0.6, 2.2, 6.5), (-0.1, -0.3, -1), (0, 1, 0), 45.0, W, H),) + prim[1:]
    s = abi.default_settings(maxSteps=96)
    try:
        for scene in (prim, sier):
            t = tables_of(scene)
            ref = h.oracle_render(scene, s, W, H, threads=16)
            assert L.rm_set_tile_order(0) == 0
            h.assert_bit_equal(h.render_guarded(renderer, t, s, W, H).cpu().numpy(), ref, "raster order")
            assert L.rm_set_tile_order(1) == 0
            if scene is prim:  # an ordered frame of another picture of this size first (a raster-order frame leaves no history)
                h.render_guarded(renderer, tables_of(moved), s, W, H)
            first = h.render_guarded(renderer, t, s, W, H)  # a new picture: geometric order (raster for the Sierpinski table)
            h.assert_bit_equal(first.cpu().numpy(), ref, "ordered, new picture")
            for k in range(8):  # cost-ordered repeats, the last sort, then the settled order
                assert ieq(h.render_guarded(renderer, t, s, W, H), first), f"repeat {k + 1}"
    finally:
        L.rm_set_tile_order(-1)


# ---------------------------------------------------------------- light split
def split_scene(W, H, nl):
    prim = SB.all_primitives_scene(W, H)
    lights = [h.make_light(abi.RM_LIGHT_DIRECTIONAL, (1, 1, 1), (-0.4, -1, -0.5)),
              h.make_light(abi.RM_LIGHT_POINT, (1, .9, .7), pos=(3, 2, 4), func=(0.7, 0.05, 0.01)),
              h.make_light(abi.RM_LIGHT_SPOT, (.6, .8, 1), direction=(0, -1, -0.3), pos=(0, 5, 1.5), func=(1, 0, 0),
                           angle=np.deg2rad(30.0), penumbra=np.deg2rad(10.0)),
              h.make_light(abi.RM_LIGHT_DIRECTIONAL, (.5, .5, .4), (0.9, 0.2, 0.1))][:nl]
    return prim[0], prim[1], prim[2], (abi.RmLight * nl)(*lights), nl, prim[5]


@pytest.mark.parametrize("nl,shape", [(1, 3), (2, 2), (3, 3), (4, 3), (4, 2)])
def test_light_split_writes_every_tile(renderer, nl, shape):
    """The split tiles are written only by the last of their workgroups to arrive: forced to the heaviest 1/32 and to every tile
    (≥ 50 frames each), then the measured mode — every frame into its own poisoned buffer, every one the oracle's frame."""
    L = lib()
    W, H = 636, 388
    scene = split_scene(W, H, nl)
    s = abi.default_settings(maxSteps=96, enableSoftShadow=1)
    t = tables_of(scene)
    try:
        assert L.rm_debug_set_tile_shape(shape) == 0
        for div, frames in ((32, 50), (1, 50), (-1, 12)):
            assert L.rm_debug_set_light_split(div) == 0
            first = h.render_guarded(renderer, t, s, W, H)
            if div == 32:
                h.assert_bit_equal(first.cpu().numpy(), h.oracle_render(scene, s, W, H, threads=16), "first frame vs oracle")
                want = first
            assert ieq(first, want)
            split = 0
            for k in range(frames):
                assert ieq(h.render_guarded(renderer, t, s, W, H), want), f"split 1/{div}, frame {k + 1}"
                split = max(split, L.rm_debug_last_split())
            if div > 0:
                assert (split > 0) == (nl > 1), "the settled picture was not split"
        assert L.rm_debug_set_light_split(1) == 0
        for k in range(6):  # a row range settles and splits on its own
            assert ieq(h.render_guarded(renderer, t, s, W, H, 37, 371), want[37:371]), f"row range, frame {k}"
    finally:
        L.rm_debug_set_tile_shape(-1)
        L.rm_debug_set_light_split(-1)


# ---------------------------------------------------------------- the wavefront pipeline
def test_wavefront_pipeline_writes_every_pixel(renderer):
    import torch
    L = lib()
    W, H = 150, 83
    scene = SB.menger_scene(W, H)
    t = tables_of(scene)
    s = abi.default_settings(mengerLevels=4, numReflection=2, enableReflection=1)
    ref, ref_b = h.oracle_render(scene, s, W, H, bright=True, threads=16)
    try:
        assert L.rm_set_kernel_path(5) == 0
        out, br = h.render_guarded(renderer, t, s, W, H, bright=True)
        assert L.rm_debug_last_path() == 5
        h.assert_bit_equal(out.cpu().numpy(), ref, "wavefront frame")
        h.assert_bit_equal(br.cpu().numpy(), ref_b, "wavefront bright")
        for r0, r1 in ((17, 60), (0, 1), (82, 83), (40, 40)):
            part = h.render_guarded(renderer, t, s, W, H, r0, r1)
            h.assert_bit_equal(part.cpu().numpy(), ref[r0:r1], f"wavefront rows {r0}-{r1}")
        for N in (2, 3):
            for k in range(N):
                rows = [L.rm_shard_row_to_frame(H, 8, k, N, i) for i in range(L.rm_shard_rows(H, 8, k, N))]
                mine, check = h.guarded((len(rows), W, 4), device=renderer.device)
                renderer.render_tiles(t, s, W, H, 8, k, N, out=mine)
                check()
                assert ieq(mine, out[torch.tensor(rows, device=out.device)]), f"wavefront shard {k}/{N}"
    finally:
        L.rm_set_kernel_path(0)


# ---------------------------------------------------------------- row ranges
def test_row_ranges_off_tile_boundaries(renderer):
    """The output holds exactly rowEnd − rowBegin rows between the guards: ranges that start and end inside tiles, one row, the
    empty range (nothing written, guards intact), with either tile shape."""
    W, H = 67, 70
    for name in ("table", "bulb_plain"):
        scene, s, res = kernel_class(name, W, H)
        ref, ref_b = h.oracle_render(scene, s, W, H, bright=True, threads=16)
        t = tables_of(scene, res)
        try:
            for shape in SHAPES:
                assert lib().rm_debug_set_tile_shape(shape) == 0
                for r0, r1 in ((3, 61), (9, 10), (0, 1), (69, 70), (17, 69), (40, 40), (0, 0), (70, 70)):
                    out, br = h.render_guarded(renderer, t, s, W, H, r0, r1, bright=True)
                    h.assert_bit_equal(out.cpu().numpy(), ref[r0:r1], f"{name} rows {r0}-{r1} shape {shape}")
                    h.assert_bit_equal(br.cpu().numpy(), ref_b[r0:r1], f"{name} rows {r0}-{r1} shape {shape} bright")
        finally:
            lib().rm_debug_set_tile_shape(-1)


# ---------------------------------------------------------------- row tiles, gathers, conversions
@pytest.mark.parametrize("relief", [0, 2])
def test_row_tiles_gathers_and_rgba8(renderer, relief):
    """render_tiles for every shard of 2-4 shards (with and without root relief), then deinterleave and deinterleave_rgba8 (flip
    on and off), tiles_to_rgba8 and to_rgba8, at an odd width — each output guarded, uint8 ones produced under two poisons."""
    import torch
    L = lib()
    W, H, T = 67, 90, 8  # 12 row tiles, the last one partial
    scene, s, _ = kernel_class("bulb_plain", W, H)
    t = tables_of(scene)
    ref = h.oracle_render(scene, s, W, H, threads=16)
    dev = renderer.device
    exp8 = (np.clip(ref, 0, 1) * np.float32(255.0) + np.float32(0.5)).astype(np.uint8)  # rows bottom-up
    img = h.guarded_u8((H, W, 4), lambda o: renderer.to_rgba8(torch.from_numpy(ref).to(dev), out=o), device=dev)
    assert (img.cpu().numpy() == exp8[::-1]).all(), "to_rgba8"
    try:
        assert L.rm_set_root_relief(relief) == 0
        for shards in (2, 3, 4):
            parts = []
            for k in range(shards):
                rows = [L.rm_shard_row_to_frame(H, T, k, shards, i) for i in range(L.rm_shard_rows(H, T, k, shards))]
                p, check = h.guarded((len(rows), W, 4), device=dev)
                renderer.render_tiles(t, s, W, H, T, k, shards, out=p)
                check()
                h.assert_bit_equal(p.cpu().numpy(), ref[rows], f"shard {k}/{shards}")
                p8 = h.guarded_u8((len(rows), W, 4), lambda o: renderer.tiles_to_rgba8(p, out=o), device=dev)
                assert (p8.cpu().numpy() == exp8[rows]).all(), f"tiles_to_rgba8 {k}/{shards}"
                parts.append((p, p8))
            frame, check = h.guarded((H, W, 4), device=dev)
            renderer.deinterleave(torch.cat([p for p, _ in parts], 0).contiguous(), W, H, T, shards, out=frame)
            check()
            h.assert_bit_equal(frame.cpu().numpy(), ref, f"deinterleave {shards}")
            slot = L.rm_gather_slot_rows(H, T, shards)
            g8 = torch.zeros((shards * slot, W, 4), dtype=torch.uint8, device=dev)
            for k, (_, p8) in enumerate(parts):
                g8[k * slot:k * slot + p8.shape[0]] = p8
            for flip in (True, False):
                d8 = h.guarded_u8((H, W, 4), lambda o: renderer.deinterleave_rgba8(g8, W, H, T, shards, slot, flip=flip, out=o),
                                  device=dev)
                assert (d8.cpu().numpy() == (exp8[::-1] if flip else exp8)).all(), f"deinterleave_rgba8 {shards} flip {flip}"
    finally:
        L.rm_set_root_relief(0)


# ---------------------------------------------------------------- batches
def batch_refs(scene, s, W, H, cams, globs):
    return [h.oracle_render((cams[f],) + tuple(scene[1:5]) + (globs[f],), s, W, H, bright=True, threads=16) for f in range(len(cams))]


def render_batch_guarded(renderer, t, s, W, H, cams, globs):
    n = len(cams)
    out, c1 = h.guarded((n, H, W, 4), device=renderer.device)
    br, c2 = h.guarded((n, H, W, 4), device=renderer.device)
    renderer.render_batch(t, s, W, H, cams, globals_=globs, out=out, out_bright=br)
    return out, br, lambda: (c1(), c2())


@pytest.mark.parametrize("n", [1, 3, 17])
def test_batch_writes_every_frame_and_nothing_after_the_last(renderer, n):
    W, H = 37, 23
    scene, s, _ = kernel_class("table", W, H)
    cams = SB.orbit((0.5, 1.8, 6), (-0.1, -0.25, -1), 45.0, W, H, n)
    globs = [scene[5]] * n
    out, br, check = render_batch_guarded(renderer, tables_of(scene), s, W, H, cams, globs)
    check()  # the guard after frame N − 1 is intact
    for f, (ref, ref_b) in enumerate(batch_refs(scene, s, W, H, cams, globs)):
        h.assert_bit_equal(out[f].cpu().numpy(), ref, f"batch of {n}, frame {f}")
        h.assert_bit_equal(br[f].cpu().numpy(), ref_b, f"batch of {n}, frame {f} bright")


def test_batch_with_frames_taking_the_wavefront_pipeline_alone(renderer):
    """Path 5 requested: the 3-D frames of a reflective table go through the wavefront pipeline one by one, the 2-D frames between
    them through the batched launches — two writers into one buffer, every frame written once."""
    L = lib()
    W, H = 45, 31
    scene = SB.menger_scene(W, H)
    s = abi.default_settings(mengerLevels=3, numReflection=1, enableReflection=1)
    n = 5
    cams = SB.orbit((2.6, 2.2, 3.0), (-2.6, -2.2, -3.0), 30.0, W, H, n)
    globs = [h.with_globals(scene[5], iTime=0.7 * f, isTwoD=int(f in (1, 2))) for f in range(n)]
    refs = batch_refs(scene, s, W, H, cams, globs)
    try:
        assert L.rm_set_kernel_path(5) == 0
        out, br, check = render_batch_guarded(renderer, tables_of(scene), s, W, H, cams, globs)
        check()
    finally:
        L.rm_set_kernel_path(0)
    for f, (ref, ref_b) in enumerate(refs):
        h.assert_bit_equal(out[f].cpu().numpy(), ref, f"frame {f}")
        h.assert_bit_equal(br[f].cpu().numpy(), ref_b, f"frame {f} bright")


# ---------------------------------------------------------------- post passes and probes
@pytest.mark.parametrize("W,H", [(700, 45), (257, 33), (64, 32), (1, 1), (3, 70)])
def test_post_process_writes_every_pixel(renderer, W, H):
    import torch
    rng = np.random.default_rng(W * 1000 + H + 7)
    frag = rng.random((H, W, 4), dtype=np.float32) * np.float32(1.6)
    frag[..., 3] = 1.0
    luma = (frag[..., :3] * np.array([0.2126, 0.7152, 0.0722], dtype=np.float32)).sum(-1, keepdims=True)
    bright = np.where(luma > 1.0, frag, np.float32(0.0)).astype(np.float32)
    bright[..., 3] = 1.0
    fd, bd = torch.from_numpy(frag).to(renderer.device), torch.from_numpy(bright).to(renderer.device)
    for name in ("bloom", "bloom_hdr_fxaa", "hdr", "gamma_fxaa"):
        post = abi.RmPostSettings(**{"exposure": 1.0, **SB.POST_CASES[name]})
        for with_bright in (True, False) if "bloom" not in name else (True,):  # bloom needs the BrightColor plane
            b = bright if with_bright else None
            out, check = h.guarded((H, W, 4), device=renderer.device)
            renderer.post_process(fd, bd if with_bright else None, post, out=out)
            check()
            h.assert_bit_equal(out.cpu().numpy(), h.oracle_post(frag, b, post), f"post {name} {W}x{H} bright={with_bright}")


@pytest.mark.parametrize("n", [1, 63, 65, 1000])
def test_probes_write_exactly_n_results(renderer, n):
    import torch
    rng = np.random.default_rng(n)
    x = rng.uniform(-30, 30, n).astype(np.float32)
    ref = np.empty_like(x)
    assert h.oracle().rmo_probe_math(abi.RM_FN_SIN, h.fptr(x), None, None, h.fptr(ref), n) == 0
    out, check = h.guarded((n,), device=renderer.device)
    renderer.probe_math(abi.RM_FN_SIN, torch.from_numpy(x).to(renderer.device), out=out)
    check()
    h.assert_bit_equal(out.cpu().numpy(), ref, f"probe_math n={n}")
    scene = SB.all_primitives_scene(64, 64)
    s = abi.default_settings()
    pts = rng.uniform(-3, 3, (n, 3)).astype(np.float32)
    ref4 = np.empty((n, 4), dtype=np.float32)
    cam, objs, no, lights, nl, g = scene
    import ctypes as C
    assert h.oracle().rmo_probe_sdscene(objs, no, C.byref(g), C.byref(s), h.fptr(pts), h.fptr(ref4), n) == 0
    out4, check4 = h.guarded((n, 4), device=renderer.device)
    renderer.probe_sdscene(tables_of(scene), s, torch.from_numpy(pts).to(renderer.device), out=out4)
    check4()
    h.assert_bit_equal(out4.cpu().numpy(), ref4, f"probe_sdscene n={n}")


# ---------------------------------------------------------------- frames in flight
def test_frames_in_flight_on_three_streams(renderer):
    """Four pictures interleaved on three streams, every frame into its own guarded buffer, one synchronisation at the end: a
    settled bulb, a table of C2's class with the light split forced, a small wavefront Menger frame and a layer frame."""
    import torch
    L = lib()
    W, H = 640, 384
    bulb = h.scene_mandelbulb(W, H)
    sb = abi.default_settings(fractalIters=8, maxSteps=96)
    table = split_scene(W, H, 3)
    st = abi.default_settings(maxSteps=96, enableSoftShadow=1, enableAmbientOcclusion=1)
    Wm, Hm = 96, 61
    menger = SB.menger_scene(Wm, Hm)
    sm = abi.default_settings(mengerLevels=4, numReflection=2, enableReflection=1)
    Wl, Hl = 72, 40
    layers, sl, _ = kernel_class("layers", Wl, Hl)
    jobs = {"bulb": (tables_of(bulb), sb, W, H), "table": (tables_of(table), st, W, H), "menger": (tables_of(menger), sm, Wm, Hm),
            "layers": (tables_of(layers), sl, Wl, Hl)}
    want = {"bulb": h.oracle_render(bulb, sb, W, H, threads=16), "table": h.oracle_render(table, st, W, H, threads=16),
            "menger": h.oracle_render(menger, sm, Wm, Hm, threads=16), "layers": h.oracle_render(layers, sl, Wl, Hl, threads=16)}
    streams = [torch.cuda.Stream(device=renderer.device) for _ in range(3)]
    plan = [[("bulb", 0)] * 8, [("table", 0)] * 8, [("menger", 5), ("layers", 0)] * 4]  # per stream: (picture, kernel path)
    try:
        assert L.rm_debug_set_light_split(1) == 0
        torch.cuda.synchronize()
        outs = []
        for k in range(8):
            for st_, seq in zip(streams, plan):
                name, path = seq[k]
                t, s, w, hh = jobs[name]
                with torch.cuda.stream(st_):  # poisoned on the stream that renders into it
                    out, check = h.guarded((hh, w, 4), device=renderer.device)
                    assert L.rm_set_kernel_path(path) == 0
                    renderer.render(t, s, w, hh, out=out)
                outs.append((name, k, out, check))
        torch.cuda.synchronize()
    finally:
        L.rm_set_kernel_path(0)
        L.rm_debug_set_light_split(-1)
    for name, k, out, check in outs:
        check()
        h.assert_bit_equal(out.cpu().numpy(), want[name], f"{name}, frame {k}")


# Both launch rings of acquire_slot (single frames, batches) only grow, once per process: their cases run in a fresh child process,
# and every launch is queued behind a gate — torch.cuda._sleep spinning the stream for GATE_CYCLES GPU clock cycles (tens of
# milliseconds at least) — so that all of them are still in flight when the host has queued the last one.
GATE_CYCLES = 50_000_000


def ring_growth_case(renderer):
    """One heavy frame behind the gate, then 14 small frames on the same stream: 15 launches in flight, so acquire_slot grows the
    frames ring (it starts empty, a fresh slot in front of each busy one) while its slots are busy.  Every frame is its own
    picture's."""
    import torch
    W, H = 1280, 720
    heavy = h.scene_mandelbulb(W, H)
    sh = abi.default_settings(fractalIters=20, maxSteps=256)
    Ws, Hs = 33, 19
    prim = SB.all_primitives_scene(Ws, Hs)
    small = [(h.make_camera((0.2 * i - 1.3, 1.6, 6), (0, -0.2, -1), (0, 1, 0), 45.0, Ws, Hs),) + prim[1:] for i in range(14)]
    s = abi.default_settings(maxSteps=96)
    # every table and buffer before the first launch: nothing but the launches themselves between the gate and the last one
    t_heavy, t_small = tables_of(heavy), [tables_of(sc) for sc in small]
    big, cbig = h.guarded((H, W, 4), device=renderer.device)
    outs = [h.guarded((Hs, Ws, 4), device=renderer.device) for _ in small]
    torch.cuda._sleep(GATE_CYCLES)
    renderer.render(t_heavy, sh, W, H, out=big)
    for t, (out, _) in zip(t_small, outs):
        renderer.render(t, s, Ws, Hs, out=out)
    torch.cuda.synchronize()
    cbig()
    for i, (scene, (out, check)) in enumerate(zip(small, outs)):
        check()
        h.assert_bit_equal(out.cpu().numpy(), h.oracle_render(scene, s, Ws, Hs), f"small frame {i}")
    for r in (0, 360, 719):  # the heavy frame: its first, middle and last rows against the oracle
        h.assert_bit_equal(big[r:r + 1].cpu().numpy(), h.oracle_render(heavy, sh, W, H, r, r + 1, threads=16), f"heavy row {r}")


def batch_slot_case(renderer):
    """Six batches behind the gate on one stream: the first four fill the batch ring (at most 4 slots, each busy slot gets a
    fresh one in front of it), the fifth and sixth find every slot busy and wait for the oldest (hipEventSynchronize).  Then a
    40-frame batch, larger than the 16 scene blocks every slot of this process holds: the idle slot it lands on grows.  Every
    batch into its own guarded buffers."""
    import torch
    W, H = 64, 40
    scene, s, _ = kernel_class("bulb_plain", W, H)
    t = tables_of(scene)
    cams = SB.orbit((0, 0, 4.5), (0, 0, -1), 30.0, W, H, 40, deg=3.0)
    globs = [h.with_globals(scene[5], iTime=0.1 * f) for f in range(40)]
    refs = batch_refs(scene, s, W, H, cams, globs)
    sizes = [3, 2, 3, 1, 3, 2]
    bufs = [(h.guarded((k, H, W, 4), device=renderer.device), h.guarded((k, H, W, 4), device=renderer.device)) for k in sizes]
    torch.cuda._sleep(GATE_CYCLES)
    for k, ((out, _), (br, _)) in zip(sizes, bufs):
        renderer.render_batch(t, s, W, H, cams[:k], globals_=globs[:k], out=out, out_bright=br)
    big, big_br, check_big = render_batch_guarded(renderer, t, s, W, H, cams, globs)
    torch.cuda.synchronize()
    check_big()
    for f in range(len(cams)):
        h.assert_bit_equal(big[f].cpu().numpy(), refs[f][0], f"40-frame batch, frame {f}")
        h.assert_bit_equal(big_br[f].cpu().numpy(), refs[f][1], f"40-frame batch, frame {f} bright")
    for i, (k, ((out, c1), (br, c2))) in enumerate(zip(sizes, bufs)):
        c1()
        c2()
        for f in range(k):
            h.assert_bit_equal(out[f].cpu().numpy(), refs[f][0], f"batch {i}, frame {f}")
            h.assert_bit_equal(br[f].cpu().numpy(), refs[f][1], f"batch {i}, frame {f} bright")


_RING_CHILD = r'''
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_write_coverage as t
from raymarcher_amd import Renderer
getattr(t, sys.argv[2])(Renderer(0))
print("ok")
'''


def run_ring_case(case):
    p = subprocess.run([sys.executable, "-c", _RING_CHILD, ROOT, case], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), (p.returncode, p.stdout[-1000:], p.stderr[-3000:])


def test_scene_block_ring_grows_behind_a_heavy_frame():
    run_ring_case("ring_growth_case")


def test_batches_in_flight_beyond_the_slot_limit():
    run_ring_case("batch_slot_case")


def test_caller_buffers_of_the_wrong_shape_are_refused(renderer):
    """A caller's out / out_bright must be exactly the rows the launch writes: anything else is refused before the launch."""
    import torch
    W, H = 33, 19
    scene, s, _ = kernel_class("table", W, H)
    t = tables_of(scene)
    dev = renderer.device
    good = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
    for bad in (torch.empty((H - 1, W, 4), dtype=torch.float32, device=dev), torch.empty((H, W, 4), dtype=torch.float64, device=dev),
                torch.empty((W, H, 4), dtype=torch.float32, device=dev).transpose(0, 1)):
        with pytest.raises(ValueError, match="out_bright"):
            renderer.render(t, s, W, H, out=good, out_bright=bad)
        with pytest.raises(ValueError, match="out "):
            renderer.render(t, s, W, H, out=bad)
    with pytest.raises(ValueError, match="out "):
        renderer.render(t, s, W, H, row_begin=3, row_end=10, out=good)
    with pytest.raises(ValueError, match="out_bright"):
        renderer.render_batch(t, s, W, H, [scene[0]] * 2, out_bright=torch.empty((1, H, W, 4), dtype=torch.float32, device=dev))
    with pytest.raises(ValueError, match="out "):
        renderer.render_tiles(t, s, W, H, 8, 0, 2, out=good)
