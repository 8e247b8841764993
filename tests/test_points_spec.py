"""The specification of rm_shade_points (tests/points_spec/rm_points_spec.c: the header's definition restated with the oracle's own
functions) on the CPU, before the GPU tests compare the kernel with it.  (a) At the hit points of a camera's primary rays, seen along
those rays, it gives the shade spec's colour and the trace spec's normal — which ties the restated lines to what rm_shade_rays and
rm_trace_rays already pin.  (b) The projection closes in on the iso-surface and obeys max_move.  (c) Every subset of outputs holds the
same bits.  Then the invariants of the definition: invalid points, the empty table, the order of the array."""
import itertools

import numpy as np
import pytest

import helpers as h
import points_helpers as PH
import scene_builders as SB
import shade_helpers as S
import trace_helpers as T
from raymarcher_amd import abi

W = H = 48


def _bulb(Wd, Hd):
    return h.scene_mandelbulb(Wd, Hd), abi.default_settings(fractalIters=8)


def _menger(Wd, Hd):
    sc = SB.menger_scene(Wd, Hd)
    return sc[:5] + (h.make_globals(itime=7.5),), abi.default_settings(mengerLevels=3)


SCENES = {
    "all_primitives": (lambda: (SB.all_primitives_scene(W, H), abi.default_settings()), True),
    "reflect_refract": (lambda: (SB.reflect_refract_scene(W, H), abi.default_settings()), True),
    "menger": (lambda: _menger(W, H), False),       # the trap at the hit point is not the march's last one: normal and id only
    "mandelbulb": (lambda: _bulb(W, H), False),
}


# ---------------------------------------------------------------- (a) the hit points of a camera's rays
@pytest.mark.parametrize("name", list(SCENES))
def test_spec_at_hit_points_equals_the_shade_and_trace_specs(name):
    build, colour = SCENES[name]
    scene, s = build()
    assert not s.enableReflection and not s.enableRefraction
    rays, hits = PH.hit_points(scene, s, W, H)
    n = len(rays)
    assert n > 1000, "the frame should show the scene"
    far = scene[0].initialFar
    sf, _, col = PH.spec_points(scene, s, hits[:, 4:7], view=rays[:, 4:7], far=far, outputs="sc" if colour else "s")
    same = PH.ids_of(sf) == T.ids_of(hits)
    print(f"{name}: {n} hits, {n - same.sum()} left out (sdScene's object at the hit point is not the march's)")
    assert n - same.sum() <= n // 100, "more than 1 % of the hits left out"
    h.assert_bit_equal(sf[same, 0:3], hits[same, 0:3], f"{name} normal")
    h.assert_bit_equal(sf[same, 4:7], hits[same, 4:7], f"{name} position")
    if colour:
        # The colour of a hit on a sponge or a bulb reads the orbit trap.  The definition takes it from sdScene at the hit point; the
        # march has it from its last evaluated point, res.d short of it along the ray: the rule of the pure fractal scenes — normal
        # and id only — holds for such a hit in a mixed table too.  all_primitives holds one of each (364 and 96 of its 1615 hits, and
        # every one of the 450 hits whose colour differs lies on them); every hit on a primitive is compared in all four words.
        kinds = np.array([scene[1][i].type for i in range(scene[2])])
        trapped = np.isin(kinds[T.ids_of(hits)], (abi.RM_MENGERSPONGE, abi.RM_MANDELBULB))
        print(f"{name}: {trapped.sum()} hits on a sponge or a bulb compared in normal and id only")
        want, _ = S.spec_shade(scene, s, rays, far)
        h.assert_bit_equal(col[same & ~trapped], want[same & ~trapped], f"{name} colour")
        assert (same & ~trapped).sum() > 1000 and len(np.unique(col, axis=0)) > 100


# ---------------------------------------------------------------- (b) projection
def _near_surface_points(rng, n=300, off=0.05):
    """(scene, settings, points): all_primitives_scene and n points within `off` of the surfaces of its nine primitives — hit points
    of the camera's rays on them, pushed along ± their normals.  The table's fractals are left out: a Newton step along the normal
    is a statement about distance functions, not about a Mandelbulb's estimate or a sponge's folded one."""
    scene, s = SB.all_primitives_scene(W, H), abi.default_settings()
    _, hits = PH.hit_points(scene, s, W, H)
    kinds = np.array([scene[1][i].type for i in range(scene[2])])
    hits = hits[np.isin(kinds[T.ids_of(hits)], h.PRIMITIVES)]
    assert len(np.unique(T.ids_of(hits))) == 9, "every primitive of the table is seen"
    pick = rng.choice(len(hits), n, replace=False)
    t = rng.uniform(-off, off, (n, 1)).astype(np.float32)
    return scene, s, (hits[pick, 4:7] + t * hits[pick, 0:3]).astype(np.float32)


def test_projection_closes_in_on_the_iso_surface():
    scene, s, pts = _near_surface_points(np.random.default_rng(3))
    iso = 0.001
    err = []
    for steps in range(4):
        sf, _, _ = PH.spec_points(scene, s, pts, iso=iso, project=steps, outputs="s")
        assert (PH.ids_of(sf) >= 0).all()
        err.append(np.abs(sf[:, 3].astype(np.float64) - np.float32(iso)))
    err = np.array(err)
    print("max |distance − iso| after 0, 1, 2, 3 steps:", err.max(axis=1))
    assert err[0].max() > 0.03, "the points should start off the surface"
    # "Never grows" down to the rounding of one evaluation: a point that has arrived sits within rounding of the surface and its
    # error moves by that rounding from step to step.  The scene lies within |coordinate| < 8, where a float32 coordinate has an ulp
    # of at most 2^-21; madd rounds each of the three coordinates once and the distance functions are 1-Lipschitz chains of a few
    # operations on values of that size: 8 ulp = 2^-18 (3.8e-6) bounds it, 260 times below the 0.001 the steps must reach.
    floor = 2.0 ** -18
    assert np.abs(pts).max() < 8.0
    assert (err[1:] <= err[:-1] + floor).all(), "|distance − iso| never grows from step to step"
    assert err[3].max() < 0.001, "three steps end below SURFACE_DIST"


def test_max_move_zero_returns_the_input_positions_in_every_bit():
    scene, s, pts = _near_surface_points(np.random.default_rng(4), n=200)
    sf, _, _ = PH.spec_points(scene, s, pts, project=3, max_move=0.0, outputs="s")
    h.assert_bit_equal(sf[:, 4:7], pts, "position")
    plain, _, _ = PH.spec_points(scene, s, pts, project=0, outputs="s")
    h.assert_bit_equal(sf, plain, "max_move = 0 is no projection at all")
    # a finite limit: no point ends farther from its start than the limit, and a point that would have is left where it was accepted last
    lim = 0.02
    sf, _, _ = PH.spec_points(scene, s, pts, project=3, max_move=lim, outputs="s")
    moved = np.linalg.norm(sf[:, 4:7].astype(np.float64) - pts.astype(np.float64), axis=1)
    assert moved.max() <= lim * (1 + 1e-6) and (moved == 0).any() and (moved > 0).any()


# ---------------------------------------------------------------- (c) output independence
@pytest.mark.parametrize("name", ["reflect_refract", "mandelbulb"])
def test_every_subset_of_outputs_gives_the_same_bits(name):
    scene, s = SCENES[name][0]()
    s.enableAmbientOcclusion = 1
    _, hits = PH.hit_points(scene, s, W, H)
    pts = hits[::7, 4:7]
    full = PH.spec_points(scene, s, pts, project=1, outputs="sac")
    for k in (1, 2):
        for outs in itertools.combinations("sac", k):
            got = PH.spec_points(scene, s, pts, project=1, outputs="".join(outs))
            for letter, a, b in zip("sac", got, full):
                if letter in outs:
                    h.assert_bit_equal(a, b, f"{name} output {letter} of {outs}")
                else:
                    assert a is None
    PH.spec_points(scene, s, pts, outputs="", expect=abi.RM_ERR_INVALID_ARGUMENT)


# ---------------------------------------------------------------- invariants of the definition
def test_invalid_points_store_the_marker_and_zeros():
    scene, s = SB.reflect_refract_scene(W, H), abi.default_settings()
    pts, views, point_bad = PH.invalid_points()
    sf, ao, col = PH.spec_points(scene, s, pts, view=views)
    assert (PH.ids_of(sf) == abi.RM_RAY_INVALID).all() and (h.bits(sf[:, 0:7]) == 0).all()
    assert (h.bits(ao) == 0).all() and (h.bits(col) == 0).all()
    # without views only the points count: a row whose view alone is bad is a valid point
    sf, _, col = PH.spec_points(scene, s, pts)
    assert ((PH.ids_of(sf) == abi.RM_RAY_INVALID) == point_bad).all()
    assert (col[~point_bad, 3] == 1.0).all(), "a valid point on an object has alpha 1"


def test_empty_table_and_far_points():
    empty, _ = h.table([])
    s = abi.default_settings()
    sf, ao, col = PH.spec_points((None, empty, 0, None, 0, h.make_globals()), s, [[0.1, 0.2, 0.3]], project=2)
    assert PH.ids_of(sf)[0] == -1 and sf[0, 3] == np.float32(1000000.0) and (h.bits(sf[0, 0:3]) == 0).all()
    h.assert_bit_equal(sf[0, 4:7], np.float32([0.1, 0.2, 0.3]), "position")
    assert h.bits(ao)[0] == 0 and (h.bits(col) == 0).all()
    scene = SB.reflect_refract_scene(W, H)
    sf, _, col = PH.spec_points(scene, s, [[300.0, -200.0, 100.0]])
    assert PH.ids_of(sf)[0] >= 0 and sf[0, 3] > 100.0 and col[0, 3] == 1.0, "a point far outside still has a nearest object"


def test_spec_of_a_shuffled_array_is_the_shuffled_result():
    scene, s = SCENES["all_primitives"][0]()
    _, hits = PH.hit_points(scene, s, W, H)
    pts = hits[::5, 4:7]
    perm = np.random.default_rng(6).permutation(len(pts))
    a = PH.spec_points(scene, s, pts, project=1)
    b = PH.spec_points(scene, s, pts[perm], project=1)
    for x, y, what in zip(a, b, ("surface", "ao", "colour")):
        h.assert_bit_equal(y, x[perm], what)


def test_spec_refuses_what_the_entry_point_refuses():
    scene, s = SB.reflect_refract_scene(W, H), abi.default_settings()
    pts = [[0.0, 0.0, 1.0]]
    for feat in (abi.RM_FEAT_TERRAIN, abi.RM_FEAT_CLOUD, abi.RM_FEAT_SEA):
        PH.spec_points(scene, abi.default_settings(features=feat), pts, expect=abi.RM_ERR_UNSUPPORTED)
    for far in (np.nan, -1.0, np.inf):
        PH.spec_points(scene, s, pts, far=far, expect=abi.RM_ERR_INVALID_ARGUMENT)
    for kw in (dict(iso=np.nan), dict(iso=np.inf), dict(max_move=-1.0), dict(max_move=np.nan), dict(project=-1),
               dict(project=abi.RM_MAX_PROJECT_STEPS + 1)):
        PH.spec_points(scene, s, pts, expect=abi.RM_ERR_INVALID_ARGUMENT, **kw)
    PH.spec_points(scene, s, pts, project=abi.RM_MAX_PROJECT_STEPS)
