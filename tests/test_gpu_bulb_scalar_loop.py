"""The plain bulb class's pooled kernels count the iterations of a Mandelbulb evaluation in a scalar register (bulbIterate's
SCALAR form in rm_device.hip.h: march()'s bulb branch in both orders of its end test, getNormal's taps, the shadow pool's loop and
renderPooled's shared first evaluation).  No operation on a pixel's values changes, so every frame is held bit for bit against the
oracle, fragColor and BrightColor:

  * 64×40 and 70×41 (ragged edge tiles), a plain bulb (the class that takes the new loop) and a general one (rotated and scaled:
    the class that keeps the former one), RM_FEAT_BULB_POWER8_ALGEBRAIC off and on (both step forms have the loop),
    fractalIters 0, 1, 2 and 12, maxSteps 1, 2 and 64, three directional lights with hard shadows (the pool) and the same frame
    with soft shadows (no pool: the primary march and shadowQueue's former loop in one kernel);
  * a far plane in front of the ball's exit for some lanes of a wave and behind it for others (the wave is refused the form
    that ends a march before an evaluation);
  * a camera whose rays are non-finite in one pixel column, so that waves hold non-finite lanes beside lanes that hit the bulb
    (the plain class then takes the object transform, and the iteration its guarded step, for the whole wave);
  * the same loops through rm_render_supersampled and rm_shade_rays.

The tests without the gpu mark establish on the CPU, with the oracle and the G-buffer's specification, that these frames contain
what they are there for: hit and background pixels, lights that N·L drops and lights that are marched, waves with lanes of both
kinds of end, waves with non-finite lanes beside hit pixels."""
import numpy as np
import pytest

import gbuffer_helpers as gb
import helpers as h
from helpers import assert_bit_equal, tables_of
from scene_builders import BULB_LIGHT_DIRS, bulb_scene
from raymarcher_amd import abi, lib
from raymarcher_amd.render import camera_rays

gpu = pytest.mark.gpu

SIZES = [(64, 40), (70, 41)]
BULBS = {
    "plain": dict(),
    "general": dict(model=h.scale(1.2, 1.2, 1.2) @ h.rotation((1, 2, 0.5), 0.6), sf=1.2),
}
CLOSE = dict(pos=(0.35, 0.25, 1.9))  # mostly silhouette and crevices: primary rays start 0.8 in front of the ball
FAR = 2.4                            # between the nearest and the farthest exit from the ball of CLOSE's rays
ZERO_COLUMN = 20                     # the pixel column of the 64-wide frame whose rays are non-finite (broken_camera)


def settings(algebraic=False, **kw):
    s = abi.default_settings(**kw)
    if algebraic:
        s.features |= abi.RM_FEAT_BULB_POWER8_ALGEBRAIC
    return s


def check(renderer, scene, s, W, H, what):
    frag, bright = renderer.render(tables_of(scene), s, W, H, bright=True)
    ref, ref_b = h.oracle_render(scene, s, W, H, bright=True)
    assert_bit_equal(frag.cpu().numpy(), ref, what)
    assert_bit_equal(bright.cpu().numpy(), ref_b, what + ", bright")


def broken_camera(scene, W, H):
    """The scene with a camera whose homogeneous w is 64·I − 20.5 along a row (I = (x + ½)/64, both planes): exactly zero in pixel
    column 20 of a 64-wide frame, where origin and direction come out non-finite.  Column 20 + k looks down −z from z = 4/k,
    column 20 − k up +z from z = −4/k, each an orthographic view 4/k wide: the neighbours of the non-finite column see the bulb."""
    assert W == 64
    cam = h.make_camera((0, 0, 4.5), (0, 0, -1), (0, 1, 0), 30.0, W, H)
    M = np.zeros((4, 4), dtype=np.float32)
    M[0, 0] = M[1, 1] = 2.0
    M[2, 2], M[2, 3] = -1.0, 3.0   # z·w = 4 on the near plane, 2 on the far one
    M[3, 0], M[3, 3] = 32.0, 11.5  # w = 32·X + 11.5 with X = 2·I − 1
    for c in range(4):
        for r in range(4):
            cam.invProjView[c * 4 + r] = M[r, c]  # column-major
    return (cam,) + tuple(scene[1:])


# ---------------------------------------------------------------- what the frames contain (CPU)
def _hit_mask(scene, s, W, H):
    _, ids, _ = gb.spec_gbuffer(scene[0], scene[1], scene[2], scene[5], s, W, H, position=False)
    return ids >= 0


@pytest.mark.parametrize("bulb", sorted(BULBS))
def test_the_frames_hold_hits_background_and_dropped_lights(bulb):
    assert lib().rm_debug_bulb_plain(bulb_scene(8, 8, **BULBS[bulb])[1], 1, h.make_globals()) == int(bulb == "plain")
    for W, H in SIZES:
        scene = bulb_scene(W, H, nl=3, **BULBS[bulb])
        for algebraic in (False, True):
            s = settings(algebraic, fractalIters=12, maxSteps=64)
            nd, ids, _ = gb.spec_gbuffer(scene[0], scene[1], scene[2], scene[5], s, W, H, position=False)
            hit = ids >= 0
            assert 0.15 < hit.mean() < 0.85, (W, H, hit.mean())  # whole tiles of background, whole tiles of surface
            L = -np.array(BULB_LIGHT_DIRS[:3], dtype=np.float64)
            L /= np.linalg.norm(L, axis=1, keepdims=True)
            ndl = nd[hit][:, :3].astype(np.float64) @ L.T  # the geometric normal; the bump moves it by little
            dropped, marched = (ndl <= -0.1).mean(), (ndl >= 0.1).mean()
            assert dropped > 0.05 and marched > 0.2, (W, H, dropped, marched)
            with_both = ((ndl <= -0.1).any(axis=1) & (ndl >= 0.1).any(axis=1)).mean()
            assert with_both > 0.2, (W, H, with_both)  # pixels that march some of their lights only


def _owns_its_end(rays, far, R2=1.3225):
    """bulbCullEnd's `own` for the unit bulb at the origin (float64; the margins are far from these rays' values)."""
    ro, rd = rays[:, 0:3].astype(np.float64), rays[:, 4:7].astype(np.float64)
    a, b, c = (rd * rd).sum(1), (ro * rd).sum(1), (ro * ro).sum(1) - R2
    disc = b * b - a * c
    t = (np.sqrt(np.maximum(disc, 0.0)) - b) / a * 1.0001 + 1.0e-3
    t = np.where((c > 0) & ((b >= 0) | (disc < 0)), -1.0, t)
    return (t <= far) & ((c > 0) | (t > 0))


def test_the_short_far_plane_gives_waves_with_both_kinds_of_end():
    for W, H in SIZES:
        scene = bulb_scene(W, H, nl=3, far=FAR, **CLOSE)
        own = _owns_its_end(camera_rays(scene[0], W, H), FAR).reshape(H, W)
        mixed = whole = 0
        for ty in range(0, H, 8):
            for tx in range(0, W, 8):
                t = own[ty:ty + 8, tx:tx + 8]
                mixed += int(t.any() and not t.all())
                whole += int(t.all())
        assert mixed >= 3 and whole >= 1, (W, H, mixed, whole)
        assert _hit_mask(scene, settings(), W, H).mean() > 0.2


def test_the_broken_camera_gives_waves_with_non_finite_lanes_beside_hits():
    W, H = SIZES[0]
    scene = broken_camera(bulb_scene(W, H, nl=3), W, H)
    rays = camera_rays(scene[0], W, H).reshape(H, W, 8)
    bad = ~np.isfinite(rays[..., [0, 1, 2, 4, 5, 6]]).all(axis=-1)
    assert bad.any() and set(np.where(bad)[1]) == {ZERO_COLUMN}, np.unique(np.where(bad)[1])
    hit = _hit_mask(scene, settings(), W, H)
    assert not hit[bad].any() and hit.mean() > 0.2
    tiles = 0
    for ty in range(0, H, 8):
        tx = ZERO_COLUMN // 8 * 8
        tiles += int(bad[ty:ty + 8, tx:tx + 8].any() and hit[ty:ty + 8, tx:tx + 8].any())
    assert tiles >= 2, tiles


# ---------------------------------------------------------------- the frames (GPU)
@gpu
@pytest.mark.parametrize("steps", [1, 2, 64])
@pytest.mark.parametrize("iters", [0, 1, 2, 12])
@pytest.mark.parametrize("algebraic", [False, True], ids=["trig", "algebraic"])
@pytest.mark.parametrize("bulb", sorted(BULBS))
def test_frames(renderer, bulb, algebraic, iters, steps):
    for W, H in SIZES:
        scene = bulb_scene(W, H, nl=3, **BULBS[bulb])
        what = f"{W}x{H} {bulb} bulb, algebraic {algebraic}, fractalIters {iters}, maxSteps {steps}"
        check(renderer, scene, settings(algebraic, fractalIters=iters, maxSteps=steps), W, H, what + ", hard shadows")
        check(renderer, scene, settings(algebraic, fractalIters=iters, maxSteps=steps, enableSoftShadow=1), W, H,
              what + ", soft shadows")


@gpu
@pytest.mark.parametrize("algebraic", [False, True], ids=["trig", "algebraic"])
@pytest.mark.parametrize("bulb", sorted(BULBS))
def test_far_plane_inside_the_ball_for_part_of_a_wave(renderer, bulb, algebraic):
    for W, H in SIZES:
        scene = bulb_scene(W, H, nl=3, far=FAR, **dict(BULBS[bulb], **CLOSE))
        for iters in (2, 12):
            check(renderer, scene, settings(algebraic, fractalIters=iters), W, H, f"{W}x{H} {bulb} bulb, far {FAR}, fractalIters {iters}")
            check(renderer, scene, settings(algebraic, fractalIters=iters, enableSoftShadow=1), W, H,
                  f"{W}x{H} {bulb} bulb, far {FAR}, fractalIters {iters}, soft shadows")


@gpu
@pytest.mark.parametrize("algebraic", [False, True], ids=["trig", "algebraic"])
@pytest.mark.parametrize("bulb", sorted(BULBS))
def test_non_finite_rays_in_part_of_a_tile(renderer, bulb, algebraic):
    W, H = SIZES[0]
    scene = broken_camera(bulb_scene(W, H, nl=3, **BULBS[bulb]), W, H)
    for iters in (1, 12):
        for steps in (2, 64):
            check(renderer, scene, settings(algebraic, fractalIters=iters, maxSteps=steps), W, H,
                  f"non-finite column, {bulb} bulb, fractalIters {iters}, maxSteps {steps}")
    check(renderer, scene, settings(algebraic, enableSoftShadow=1), W, H, f"non-finite column, {bulb} bulb, soft shadows")


@gpu
@pytest.mark.parametrize("algebraic", [False, True], ids=["trig", "algebraic"])
def test_supersampled_and_shaded_rays(renderer, algebraic):
    ss = 2

    def resolve(a):  # the header's tree for ss = 2: x pairs, y pairs, · 1/4
        a = a[:, 0::2] + a[:, 1::2]
        return (a[0::2] + a[1::2]) * np.float32(0.25)
    for W, H in SIZES:
        for iters, steps in ((0, 64), (1, 2), (2, 1), (12, 64)):
            s = settings(algebraic, fractalIters=iters, maxSteps=steps)
            what = f"{W}x{H}, fractalIters {iters}, maxSteps {steps}"
            # the sample frame of a W × H frame with ss = 2 is the 2W × 2H frame of the same camera
            scene = bulb_scene(W, H, nl=3)
            out, br = renderer.render_supersampled(tables_of(scene), s, W, H, [scene[0]], ss, bright=True)
            S, Sb = h.oracle_render(scene, s, W * ss, H * ss, bright=True)
            assert np.isfinite(S).all() and np.isfinite(Sb).all()  # NaN payloads could differ between NumPy's adds and the GPU's
            assert_bit_equal(out[0].cpu().numpy(), resolve(S), "supersampled " + what)
            assert_bit_equal(br[0].cpu().numpy(), resolve(Sb), "supersampled " + what + ", bright")
            for bulb in sorted(BULBS):
                scene = bulb_scene(W, H, nl=3, **BULBS[bulb])
                col, colb = renderer.shade_rays(tables_of(scene), s, camera_rays(scene[0], W, H), far=scene[0].initialFar, bright=True)
                ref, ref_b = h.oracle_render(scene, s, W, H, bright=True)
                assert_bit_equal(col.cpu().numpy().reshape(H, W, 4), ref, f"shaded rays {what}, {bulb} bulb")
                assert_bit_equal(colb.cpu().numpy().reshape(H, W, 4), ref_b, f"shaded rays {what}, {bulb} bulb, bright")
