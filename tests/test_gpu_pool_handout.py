"""The shadow pool's hand-out from prepared per-light constants (shadowPool's PREP form, rm_device.hip.h; SceneBlock::lightPrep
filled by scene_light_prep in rm_frame.cpp), bit for bit against the oracle: a lane that takes a ray reads its light's normalised
direction, that direction in object space and its square from LDS and computes only the pixel's part of the cull.  64×64 frames,
fragColor and BrightColor, over what the hand-out depends on: the number of lights (the table in LDS: 1, 3, RM_MAX_LIGHTS), tables
that must leave the pool (a point light among directional ones), the bulb's class (plain: the cull takes the origin for its object
space image; general: it transforms it), the cull's radius (|seed|² in (1.2996, 4]: the wide ball) and its absence (|seed|² > 4), a
camera inside the ball, a far plane below the ball's exit (rays that do not own their end: the wave leaves the PRE form in
mid-pool), maxSteps 1 and 2, 2 and 4 waves per workgroup (one table, several writers), edge tiles whose waves call the pool with
a few lanes (which still have to write the whole table), a direction that normalises to NaN (no shared first step), the
supersampling and the ray-shading kernels.  The plain form's shortcut is probed on its own: origins with
zeros of either sign in every coordinate, and a non-finite origin among finite ones of the same wave."""
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as h
from helpers import assert_bit_equal, tables_of
from scene_builders import BULB_LIGHT_COLORS, BULB_LIGHT_DIRS, bulb_scene
from raymarcher_amd import abi, lib
from raymarcher_amd.render import camera_rays

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = H = 64

BULBS = {
    "plain": dict(),
    "general": dict(model=h.scale(1.2, 1.2, 1.2) @ h.rotation((1, 2, 0.5), 0.6), sf=1.2),
    "julia_wide_ball": dict(julia=(1.2, 0.5)),   # |seed|² = 1.69: tight is false, R = 2.1
    "julia_no_cull": dict(julia=(1.8, 1.0)),     # |seed|² = 4.24: the cull is off, every end is `far`
}


def directional(n):
    return [h.make_light(abi.RM_LIGHT_DIRECTIONAL, BULB_LIGHT_COLORS[i % 5], BULB_LIGHT_DIRS[i]) for i in range(n)]


LIGHTS = {
    "one": lambda: directional(1),
    "three": lambda: directional(3),
    "max": lambda: directional(abi.RM_MAX_LIGHTS),
    "with_point_lights": lambda: directional(2) + [h.make_light(abi.RM_LIGHT_POINT, (1, 0.8, 0.6), pos=(1.5, 2.0, 2.5), func=(1, 0.1, 0.02)),
                                                   directional(4)[3]],
}


def check(renderer, scene, s, what, plain=None):
    frag, bright = renderer.render(tables_of(scene), s, W, H, bright=True)
    if plain is not None:
        assert lib().rm_debug_bulb_plain(scene[1], 1, scene[5]) == int(plain)
    ref, ref_b = h.oracle_render(scene, s, W, H, bright=True)
    assert_bit_equal(frag.cpu().numpy(), ref, what)
    assert_bit_equal(bright.cpu().numpy(), ref_b, what + " bright")


@pytest.mark.parametrize("bulb", sorted(BULBS))
@pytest.mark.parametrize("table", sorted(LIGHTS))
def test_light_tables_and_bulbs(renderer, table, bulb):
    scene = bulb_scene(W, H, lights=LIGHTS[table](), **BULBS[bulb])
    check(renderer, scene, abi.default_settings(), f"{table} lights, {bulb} bulb", plain=bulb == "plain")


@pytest.mark.parametrize("size", [(61, 37), (9, 70), (66, 3)])
def test_edge_tiles_after_another_light_table(renderer, size):
    """Waves of edge tiles call the pool with a few lanes (one column, three rows), which must still write the whole table of
    constants: a frame with another light table goes first, so that words left unwritten would hold ITS constants."""
    w, hh = size
    s = abi.default_settings()
    for bulb in ("plain", "general"):
        first = bulb_scene(w, hh, lights=directional(abi.RM_MAX_LIGHTS)[::-1], **BULBS[bulb])
        renderer.render(tables_of(first), s, w, hh)
        scene = bulb_scene(w, hh, lights=directional(abi.RM_MAX_LIGHTS), **BULBS[bulb])
        frag, bright = renderer.render(tables_of(scene), s, w, hh, bright=True)
        ref, ref_b = h.oracle_render(scene, s, w, hh, bright=True)
        assert_bit_equal(frag.cpu().numpy(), ref, f"{w}x{hh}, {bulb} bulb")
        assert_bit_equal(bright.cpu().numpy(), ref_b, f"{w}x{hh}, {bulb} bulb, bright")


@pytest.mark.parametrize("bulb", ["plain", "general"])
def test_camera_inside_the_ball(renderer, bulb):
    pos = (0.8, 0.45, 0.55)  # |pos| = 1.07 < 1.15: primary and shadow rays start inside the cull ball
    scene = bulb_scene(W, H, nl=4, pos=pos, look=tuple(-np.asarray(pos)), **BULBS[bulb])
    check(renderer, scene, abi.default_settings(), f"camera inside the ball, {bulb} bulb")


@pytest.mark.parametrize("far", [2.2, 2.6])
@pytest.mark.parametrize("bulb", ["plain", "general"])
def test_far_below_the_balls_exit(renderer, bulb, far):
    """Shadow rays whose end is `far`, not the cull's: they do not own it, and the wave that hands one out leaves the PRE form."""
    scene = bulb_scene(W, H, nl=5, far=far, pos=(0.35, 0.25, 1.9), **BULBS[bulb])
    check(renderer, scene, abi.default_settings(), f"far = {far}, {bulb} bulb")


@pytest.mark.parametrize("steps", [1, 2])
def test_step_caps(renderer, steps):
    for bulb in ("plain", "general"):
        scene = bulb_scene(W, H, nl=4, pos=(0.35, 0.25, 1.9), **BULBS[bulb])
        check(renderer, scene, abi.default_settings(maxSteps=steps), f"maxSteps = {steps}, {bulb} bulb")


def test_a_direction_that_normalises_to_nan(renderer):
    """The table check does not read a light's direction: a zero one gives L = NaN, which takes every pixel out of the shared first
    step (`shared` is false) and its rays through the pool from the start."""
    lights = directional(3)
    for k in range(3):
        lights[1].dir[k] = 0.0
    for bulb in ("plain", "general"):
        check(renderer, bulb_scene(W, H, lights=lights, **BULBS[bulb]), abi.default_settings(), f"zero direction, {bulb} bulb")


def test_supersampled_and_shaded_rays(renderer):
    s = abi.default_settings()
    ss = 2

    def resolve(a):  # the header's tree for ss = 2: x pairs, y pairs, · 1/4
        a = a[:, 0::2] + a[:, 1::2]
        return (a[0::2] + a[1::2]) * np.float32(0.25)
    # the sample frame of a W/2 × H/2 frame with ss = 2 is the W × H frame of the same camera
    scene_half = bulb_scene(W // ss, H // ss, nl=4, pos=(0.35, 0.25, 1.9))
    out, br = renderer.render_supersampled(tables_of(scene_half), s, W // ss, H // ss, [scene_half[0]], ss, bright=True)
    S, Sb = h.oracle_render(scene_half, s, W, H, bright=True)
    assert np.isfinite(S).all() and np.isfinite(Sb).all()  # NaN payloads could differ between NumPy's adds and the GPU's
    assert_bit_equal(out[0].cpu().numpy(), resolve(S), "supersampled")
    assert_bit_equal(br[0].cpu().numpy(), resolve(Sb), "supersampled bright")
    for bulb in ("plain", "general"):
        scene = bulb_scene(W, H, nl=abi.RM_MAX_LIGHTS, **BULBS[bulb])
        rays = camera_rays(scene[0], W, H)
        col, colb = renderer.shade_rays(tables_of(scene), s, rays, far=scene[0].initialFar, bright=True)
        ref, ref_b = h.oracle_render(scene, s, W, H, bright=True)
        assert_bit_equal(col.cpu().numpy().reshape(H, W, 4), ref, f"shaded rays, {bulb} bulb")
        assert_bit_equal(colb.cpu().numpy().reshape(H, W, 4), ref_b, f"shaded rays, {bulb} bulb, bright")


_CHILD = r'''
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_pool_handout as t
from raymarcher_amd import Renderer, abi
r = Renderer(0)
for bulb in ("plain", "general"):
    for table in ("three", "max"):
        t.check(r, t.bulb_scene(t.W, t.H, lights=t.LIGHTS[table](), pos=(0.35, 0.25, 1.9), **t.BULBS[bulb]), abi.default_settings(),
                f"{table} {bulb}")
print("ok")
'''


@pytest.mark.parametrize("wpb", [2, 4])
def test_waves_per_block(wpb):
    """Two and four waves per workgroup: one table of constants in LDS, written by each of them (the environment is read once per
    process, hence the child)."""
    env = dict(os.environ, RM_WAVES_PER_BLOCK=str(wpb))
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), (p.returncode, p.stdout[-1000:], p.stderr[-2000:])


# ---------------------------------------------------------------- the cull of a hand-out, probed (rm_probe_pool_cull)
def probe_origins():
    """Three waves of 64 shadow origins: (0) every sign pattern of zeros in every coordinate, with the other coordinates on, in
    and outside the ball; (1) random origins around the bulb's surface and beyond both cull radii, with huge but finite ones whose
    square overflows; (2) wave 0's origins again with ONE non-finite origin among them."""
    z = np.float32(0.0)
    vals = [z, -z, np.float32(0.6), np.float32(-1.1), np.float32(2.5)]
    zeros = [(a, b, c) for a in vals for b in vals for c in vals if any(f2 == 0 for f2 in (a, b, c))]
    rng = np.random.default_rng(5)
    pick = rng.permutation(len(zeros))[:56]
    w0 = [zeros[i] for i in pick] + [(z, z, z), (-z, -z, -z), (z, -z, z), (-z, z, -z), (z, z, -z), (-z, -z, z), (-z, z, z), (z, -z, -z)]
    w1 = (rng.standard_normal((64, 3)) * rng.choice([0.5, 1.0, 1.3, 3.0], (64, 1))).astype(np.float32)
    w1[60] = (2e19, 1.0, -0.5)
    w1[61] = (-0.0, 3e38, 0.0)
    w2 = np.array(w0, dtype=np.float32)
    w2[17] = (0.3, np.inf, -0.0)
    return np.concatenate([np.array(w0, dtype=np.float32), w1, w2]).astype(np.float32)


@pytest.mark.parametrize("bulb", ["plain", "general", "julia_wide_ball", "julia_no_cull"])
def test_prepared_cull_equals_the_whole_computation(renderer, bulb):
    torch = renderer.torch
    lights = directional(abi.RM_MAX_LIGHTS)
    scene = bulb_scene(W, H, lights=lights, **BULBS[bulb])
    t, s = tables_of(scene), abi.default_settings()
    plain = lib().rm_debug_bulb_plain(scene[1], 1, scene[5])
    assert plain == int(bulb == "plain")
    staged = np.zeros((abi.RM_MAX_LIGHTS, 8), np.float32)
    assert lib().rm_debug_light_prep(scene[1], 1, scene[3], scene[4], h.fptr(staged)) == 0
    pts = torch.from_numpy(probe_origins()).to(renderer.device)
    assert pts.shape[0] == 192
    for far in (100.0, 0.7):  # the cull's end wins, and `far` wins (the ray does not own its end)
        for light in range(abi.RM_MAX_LIGHTS):  # axis-aligned directions (zeros in pd, a zero b) and oblique ones
            out = renderer.probe_pool_cull(t, s, pts, 2 if plain else 1, light, far).cpu().numpy()
            what = f"{bulb} bulb, light {light}, far {far}"
            nan = np.isnan(out[:, 2])
            assert (np.isnan(out[:, 0]) == nan).all() and not nan.any(), what  # min_(end, NaN) is `end`: no NaN comes back
            assert_bit_equal(out[:, 0:2], out[:, 2:4], what)
            assert_bit_equal(out[:, 4:7], np.broadcast_to(staged[light, :3], (192, 3)), what + ": L")
            if bulb == "julia_no_cull":
                assert (out[:, 0] == np.float32(far)).all() and not out[:, 1].any()
    if bulb == "plain":  # the cases are what they claim to be: both outcomes of `own`, ends of both kinds
        out = renderer.probe_pool_cull(t, s, pts, 2, 3, 100.0).cpu().numpy()
        assert out[:, 1].any() and not out[:, 1].all() and (out[:, 0] < 0).any() and (out[:, 0] == 100.0).any()
