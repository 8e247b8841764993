"""The specification of rm_trace_rays (tests/trace_spec/rm_trace_spec.c, the oracle's own raymarch, getNormal, bumpNormal and
softshadow) on the CPU, before the GPU tests compare the kernel with it: on a camera's own rays it equals the G-buffer specification
in every bit, and on lone spheres it agrees with the analytic intersection for every one of 20 000 seeded rays per scale."""
import numpy as np
import pytest

import gbuffer_helpers as G
import helpers as h
import scene_builders as SB
import trace_helpers as T
from raymarcher_amd import abi, camera_rays

SURFACE_DIST = 1e-3  # frag:32


# ---------------------------------------------------------------- against the G-buffer specification
@pytest.mark.parametrize("W,H", [(64, 36), (37, 23)])
@pytest.mark.parametrize("name", ["directional_light_2", "mandelbulb"])
def test_spec_on_a_cameras_rays_equals_the_gbuffer_spec_in_every_bit(name, W, H):
    scene = SB.directional_light_2(W, H) if name == "directional_light_2" else h.scene_mandelbulb(W, H)
    s = abi.default_settings()
    rays = camera_rays(scene[0], W, H)
    hits = T.spec_trace(scene[1], scene[2], scene[5], s, rays)
    nd, ids, pos = G.spec_gbuffer(scene[0], scene[1], scene[2], scene[5], s, W, H)
    ids = ids.reshape(-1)
    assert 0 < (ids >= 0).sum() < W * H, "the frame should hold hits and misses"
    assert (T.ids_of(hits) == ids).all()
    T.assert_bits(hits[:, 0:4], nd.reshape(-1, 4), f"{name} normal and depth")  # a miss: zeros and depth = far = tMax
    T.assert_bits(hits[:, 4:7], pos.reshape(-1, 4)[:, 0:3], f"{name} position")
    # without normals: the same ids and t, zeros elsewhere
    bare = T.spec_trace(scene[1], scene[2], scene[5], s, rays, "no_normal")
    assert (T.ids_of(bare) == ids).all()
    T.assert_bits(bare[:, 3], hits[:, 3], "t without normals")
    assert (T.bits(bare[:, 0:3]) == 0).all() and (T.bits(bare[:, 4:7]) == 0).all()


def test_spec_invalid_rays_and_edges():
    objs, n = T.sphere_table(1.0, (0.0, 0.0, 0.0))
    g, s = h.make_globals(), abi.default_settings()
    rays, n_invalid = T.invalid_rays()
    for mode in T.MODES:
        hits = T.spec_trace(objs, n, g, s, rays, mode)
        ids = T.ids_of(hits)
        assert (ids[:n_invalid] == abi.RM_RAY_INVALID).all() and (T.bits(hits[:n_invalid, 0:7]) == 0).all(), mode
        assert (ids[n_invalid:] != abi.RM_RAY_INVALID).all(), mode  # tMax = +inf and −0 are valid
    # tMax = 0 is the reference's loop with end = 0: `rayDepth > end` is tested AFTER the evaluation, so the march takes one full
    # step, and a hit found there counts (sphere tracing lands on this sphere head-on in one step); sideways it is a miss with t = 0
    ray = T.make_rays([[0, 0, 5], [0, 0, 5]], [[0, 0, -1], [0, 1, 0]], 0.0)
    first = T.spec_trace(objs, n, g, s, ray)
    assert T.ids_of(first).tolist() == [0, -1] and first[1, 3] == 0.0
    far = T.make_rays([[0, 0, 5]], [[0, 0, -1]], 50.0)
    assert T.ids_of(T.spec_trace(objs, n, g, s, far))[0] == 0
    empty, _ = h.table([])
    for mode in T.MODES:
        assert T.ids_of(T.spec_trace(empty, 0, g, s, far, mode))[0] == -1
        assert T.ids_of(T.spec_trace(objs, n, g, abi.default_settings(maxSteps=0), far, mode))[0] == -1
    # dir is used as given: the same line at half the speed hits the same point at twice the t
    slow = T.make_rays([[0.1, 0.05, 5]], [[0, 0, -0.5]], 50.0)
    fast = T.make_rays([[0.1, 0.05, 5]], [[0, 0, -1.0]], 50.0)
    a, b = T.spec_trace(objs, n, g, s, slow), T.spec_trace(objs, n, g, s, fast)
    assert abs(a[0, 3] - 2 * b[0, 3]) <= 4 * SURFACE_DIST and np.abs(a[0, 4:7] - b[0, 4:7]).max() <= 2 * SURFACE_DIST


# ---------------------------------------------------------------- against the analytic sphere
# scale, centre, seed, and twice the largest |normal − radial| component measured on this specification (profiles/trace_rays.md has
# the figures and what they were measured on): binary32 cancellation in the 5e-4 taps grows as the sphere shrinks.
SPHERES = [(1.0, (0.3, -0.2, 0.5), 11, 2 * 3.9202e-4), (2.0, (-1.0, 0.7, 0.2), 12, 2 * 3.5375e-4), (0.25, (0.1, 0.1, -0.4), 13, 2 * 1.1638e-3)]


@pytest.mark.parametrize("scale,centre,seed,normal_bound", SPHERES)
def test_spec_on_a_lone_sphere_against_the_analytic_intersection(scale, centre, seed, normal_bound):
    """RM_SPHERE of radius R = 0.5·scale.  20 000 seeded rays from distance 3 to 8 with impact parameter <= 0.9 R: every one hits
    object 0.  |t − t_analytic| <= 4·SURFACE_DIST + 1e-5·t: the march stops within SURFACE_DIST of the surface, at most
    SURFACE_DIST / cos 64° = 2.3·SURFACE_DIST along the ray (asin 0.9 = 64°), and res.d steps back by less than SURFACE_DIST.
    | |position − c| − R | <= 2·SURFACE_DIST + 1e-5 by the same argument.  No ray is excluded from any check."""
    R = 0.5 * scale
    c = np.array(centre, dtype=np.float64)
    objs, n = T.sphere_table(scale, centre)
    g, s = h.make_globals(), abi.default_settings(features=abi.RM_FEAT_WHITE_BACKGROUND)  # no bump: the normal is the surface's
    rng = np.random.default_rng(seed)
    rays, o, d = T.sphere_rays(rng, 20000, centre, R, 0.0, 0.9)
    oc = o - c
    a, b, cc = (d * d).sum(1), (oc * d).sum(1), (oc * oc).sum(1) - R * R
    disc = b * b - a * cc
    assert (disc > 0).all() and (np.sqrt(np.maximum(cc + R * R - b * b / a, 0)) <= 0.9 * R * (1 + 1e-6)).all()
    t_analytic = (-b - np.sqrt(disc)) / a
    hits = T.spec_trace(objs, n, g, s, rays)
    assert (T.ids_of(hits) == 0).all()
    t = hits[:, 3].astype(np.float64)
    t_err = np.abs(t - t_analytic)
    p = hits[:, 4:7].astype(np.float64)
    r_err = np.abs(np.linalg.norm(p - c, axis=1) - R)
    radial = (p - c) / np.linalg.norm(p - c, axis=1, keepdims=True)
    n_err = np.abs(hits[:, 0:3].astype(np.float64) - radial).max()
    print(f"scale {scale}: max |t - t_analytic| = {t_err.max() / SURFACE_DIST:.3f} SURFACE_DIST, max ||p - c| - R| = {r_err.max():.4e}, "
          f"max |normal - radial| = {n_err:.4e}")
    assert (t_err <= 4 * SURFACE_DIST + 1e-5 * t_analytic).all()
    assert (r_err <= 2 * SURFACE_DIST + 1e-5).all()
    assert n_err <= normal_bound
    # occlusion along the same rays: the sphere is in the way; without normals: the same ids and t
    occ = T.spec_trace(objs, n, g, s, rays, "occlusion")
    assert (T.ids_of(occ) == 0).all() and (T.bits(occ[:, 0:3]) == 0).all() and (T.bits(occ[:, 4:7]) == 0).all()
    bare = T.spec_trace(objs, n, g, s, rays, "no_normal")
    assert (T.ids_of(bare) == 0).all()
    T.assert_bits(bare[:, 3], hits[:, 3], "t without normals")
    # rays that pass at 1.1 R or more: −1 in both modes; the closest modes store tMax as given and zeros, occlusion its penumbra
    # factor, which a ray that passes close has below 1
    wide, o, d = T.sphere_rays(rng, 20000, centre, R, 1.1, 2.0)
    oc = o - c
    assert (np.sqrt((oc * oc).sum(1) - (oc * d).sum(1) ** 2 / (d * d).sum(1)) >= 1.1 * R * (1 - 1e-6)).all()
    for mode in ("closest", "no_normal"):
        miss = T.spec_trace(objs, n, g, s, wide, mode)
        assert (T.ids_of(miss) == -1).all(), mode
        T.assert_bits(miss[:, 3], wide[:, 3], f"t of a miss, {mode}")
        assert (T.bits(miss[:, 0:3]) == 0).all() and (T.bits(miss[:, 4:7]) == 0).all()
    occ = T.spec_trace(objs, n, g, s, wide, "occlusion")
    assert (T.ids_of(occ) == -1).all()
    assert ((occ[:, 3] > 0) & (occ[:, 3] <= 1)).all() and (occ[:, 3] < 1).any()


def test_the_soft_shadow_ball_does_not_hold_for_a_far_origin():
    """Why the occlusion launch stages cullR2Soft = 0.  The launcher's larger ball for soft-shadow rays argues from a
    start inside the cull ball; a ray from 200 away that never enters that larger ball would end after one evaluation with the
    factor still 1.  The reference goes on and lowers it: 8·d/t with d ≈ 0.24 and t ≈ 200."""
    import ctypes as C
    from raymarcher_amd import lib
    objs, n = T.sphere_table(1.0, (0.0, 0.0, 0.0))
    g = h.make_globals()
    out = (C.c_float * 14)()
    assert lib().rm_debug_cull_bounds(objs, n, C.byref(g), out) == 0
    assert out[0] == 1.0 and out[5] > out[4] > 0.25  # cullOk, cullR2Soft > cullR2 > R²
    x = 1.05 * float(np.sqrt(out[5]))  # passes outside the soft-shadow ball
    far = T.make_rays([[x, 0.0, 200.0]], [[0.0, 0.0, -1.0]], 1000.0)
    occ = T.spec_trace(objs, n, g, abi.default_settings(), far, "occlusion")
    assert T.ids_of(occ)[0] == -1 and 0.0 < occ[0, 3] < 0.02
