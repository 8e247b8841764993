"""The bulb kernels' wave-wide shadow pool (renderPooled / shadowPool in rm_device.hip.h), bit for bit against the oracle: every
lane of a wave marches the hard-shadow rays of any pixel of the wave, light-major, after each pixel's shared first step.  The
frames put pressure on the pool: silhouettes (most lanes without a ray), 1-10 directional lights with some facing away (N·L
drops them for part of the pixels), maxSteps 0-3 (the shared first step's edge cases), a far plane that ends rays early,
frame sizes that are not multiples of the tile, the 4×16 tile, 2 and 4 waves per workgroup, plain and general bulbs, the
algebraic power-8 step, batches and row shards.  The reference counters stay the reference's."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as h
from helpers import assert_bit_equal, tables_of
from scene_builders import bulb_scene
from raymarcher_amd import abi, lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# directional light directions: the c3 frame's three, then ones that light the bulb from the sides and from behind the camera


CLOSE = dict(pos=(0.35, 0.25, 1.9))  # a close-up: the frame is mostly silhouette and crevices
VIEWS = {
    "c3_camera": dict(),
    "close_up": CLOSE,
    "rotated_scaled": dict(model=h.scale(1.2, 1.2, 1.2) @ h.rotation((1, 2, 0.5), 0.6), sf=1.2),
    "julia": dict(julia=(0.35, -0.2)),
}


def check(renderer, scene, s, W, H, what):
    assert_bit_equal(renderer.render(tables_of(scene), s, W, H).cpu().numpy(), h.oracle_render(scene, s, W, H), what)


@pytest.mark.parametrize("view", sorted(VIEWS))
@pytest.mark.parametrize("nl", [1, 2, 3, abi.RM_MAX_LIGHTS])
def test_pool_lights_and_views(renderer, view, nl):
    W, H = 61, 37  # not multiples of 8: the edge lanes leave before the pool
    check(renderer, bulb_scene(W, H, nl=nl, **VIEWS[view]), abi.default_settings(), W, H, f"{view} nl={nl}")


@pytest.mark.parametrize("steps", [0, 1, 2, 3, 24])
def test_pool_step_caps(renderer, steps):
    """maxSteps 0 (no evaluation at all), 1 (every ray ends after the shared first step), 2, 3, and a cap that cuts long rays."""
    W, H = 45, 29
    for view in ("c3_camera", "close_up"):
        scene = bulb_scene(W, H, nl=4, **VIEWS[view])
        check(renderer, scene, abi.default_settings(maxSteps=steps), W, H, f"{view} maxSteps={steps}")


@pytest.mark.parametrize("far", [2.2, 2.6, 3.0])
def test_pool_short_far_plane(renderer, far):
    """A far plane that ends shadow rays after a few steps (some rays' end falls below their first step)."""
    W, H = 53, 31
    check(renderer, bulb_scene(W, H, nl=5, far=far, **CLOSE), abi.default_settings(), W, H, f"far={far}")


def test_pool_without_bump_and_with_ambient_occlusion(renderer):
    W, H = 47, 33
    for s in (abi.default_settings(features=abi.RM_FEAT_WHITE_BACKGROUND),
              abi.default_settings(enableAmbientOcclusion=1)):
        for view in ("c3_camera", "close_up"):
            check(renderer, bulb_scene(W, H, nl=3, **VIEWS[view]), s, W, H, f"{view} features={s.features}")


def test_pool_algebraic_power8(renderer):
    W, H = 61, 37
    s = abi.default_settings(features=abi.RM_FEAT_REFERENCE_DEFAULT | abi.RM_FEAT_BULB_POWER8_ALGEBRAIC)
    for view in ("c3_camera", "close_up", "julia"):
        check(renderer, bulb_scene(W, H, nl=4, **VIEWS[view]), s, W, H, f"algebraic {view}")


def test_pool_4x16_tiles(renderer):
    L = lib()
    W, H = 61, 37
    try:
        assert L.rm_debug_set_tile_shape(2) == 0
        for view in ("c3_camera", "close_up", "rotated_scaled"):
            check(renderer, bulb_scene(W, H, nl=3, **VIEWS[view]), abi.default_settings(), W, H, f"4x16 {view}")
    finally:
        L.rm_debug_set_tile_shape(-1)


def test_pool_batch_and_row_shards(renderer):
    W, H = 53, 35
    scene = bulb_scene(W, H, nl=4)
    s = abi.default_settings()
    positions = [(0, 0, 4.5), CLOSE["pos"], (1.2, 0.8, 2.6), (-2.0, 0.5, 3.0)]
    cams = [h.make_camera(p, tuple(-np.asarray(p)), (0, 1, 0), 30.0, W, H) for p in positions]
    got = renderer.render_batch(tables_of(scene), s, W, H, cams).cpu().numpy()
    for i, cam in enumerate(cams):
        one = (cam,) + scene[1:]
        assert_bit_equal(got[i], h.oracle_render(one, s, W, H), f"batch frame {i}")
    scene = bulb_scene(W, H, nl=3, **CLOSE)
    ref = h.oracle_render(scene, s, W, H)
    tile_rows, shards = 4, 3
    for k in range(shards):
        part = renderer.render_tiles(tables_of(scene), s, W, H, tile_rows, k, shards).cpu().numpy()
        rows = [lib().rm_shard_row_to_frame(H, tile_rows, k, shards, i) for i in range(part.shape[0])]
        assert_bit_equal(part, ref[rows], f"shard {k}")


def test_pool_counters(renderer):
    """The reference counters are the oracle's; the executed ones (the pool, with its shared first steps) do not exceed them."""
    W, H = 45, 29
    scene = bulb_scene(W, H, nl=3, **CLOSE)
    s = abi.default_settings()
    ref, rc = h.oracle_render(scene, s, W, H, counters=True)
    out, c1 = renderer.render_counted(tables_of(scene), s, W, H, abi.RM_COUNT_REFERENCE)
    assert_bit_equal(out.cpu().numpy(), ref, "reference-counted")
    for f in ("sceneEvals", "bulbIters", "hitPixels", "shadedPoints"):
        assert getattr(c1, f) == getattr(rc, f), f
    out, c2 = renderer.render_counted(tables_of(scene), s, W, H, abi.RM_COUNT_EXECUTED)
    assert_bit_equal(out.cpu().numpy(), ref, "executed-counted")
    assert 0 < c2.sceneEvals < c1.sceneEvals and c2.hitPixels == c1.hitPixels


_CHILD = r'''
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_bulb_shadow_pool as t
from raymarcher_amd import Renderer, abi
r = Renderer(0)
W, H = 61, 37
for view in ("c3_camera", "close_up", "rotated_scaled"):
    t.check(r, t.bulb_scene(W, H, nl=4, **t.VIEWS[view]), abi.default_settings(), W, H, view)
print("ok")
'''


@pytest.mark.parametrize("wpb", [2, 4])
def test_pool_waves_per_block(wpb):
    """Two and four waves per workgroup, each wave with its own list (the environment is read once per process)."""
    env = dict(os.environ, RM_WAVES_PER_BLOCK=str(wpb))
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), (p.returncode, p.stdout[-1000:], p.stderr[-2000:])
