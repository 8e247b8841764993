"""The work around the Mandelbulb iterations (rm_device.hip.h), bit for bit against the oracle.

Part A — marches that end BEFORE an evaluation whose outcome the bulb cull has already proven (march()'s PRE form, shadowPool's):
views and scenes that put rays on every side of the test — never entering the ball, leaving it, starting inside it, starting
just outside and looking away, tangent to it, ended by a far plane in front of the ball's exit, both ball radii with scaleFactor
and the Julia seed at and just past their admitted limits, the cull switched off, step caps 0-2, 1-10 directional lights with
some behind the surface, and a point light (which leaves the pool for march<SHADOW>).  The executed counters stay at or below
the reference's.

Part B — the one range guard of the estimate's log / sqrt / reciprocal (bulbIterate's tail): points that leave the fused path
(the origin, the y axis, |p| near 1e-20, interior and boundary points run to the iteration cap, |p| from 1e5 to 3e19 where dz
passes the reciprocal's range and overflows, NaN) mixed into waves of ordinary lanes, and whole waves of each, through the probe
of every bulb instantiation."""
import ctypes as C
import types

import numpy as np
import pytest

import helpers as h
from helpers import assert_bit_equal, tables_of
from scene_builders import bulb_scene
from raymarcher_amd import abi, lib

pytestmark = pytest.mark.gpu

F32 = np.float32
# directional lights: the c3 frame's three, then ones from the sides and from behind the camera


def check(renderer, scene, s, W, H, what):
    assert_bit_equal(renderer.render(tables_of(scene), s, W, H).cpu().numpy(), h.oracle_render(scene, s, W, H), what)


def scaled(sf, **kw):
    """A bulb of size sf seen as the c3 camera sees the unit one (the near plane scales along)."""
    return dict(model=h.scale(sf, sf, sf), sf=sf, pos=(0, 0, 4.5 * sf), near=0.1 * sf, **kw)


CLOSE = dict(pos=(0.35, 0.25, 1.9))  # mostly silhouette and crevices
VIEWS = {
    "c3_camera": dict(),                                               # the corner tiles never enter the ball
    "close_up": CLOSE,
    "inside_ball": dict(pos=(0.3, 0.2, 1.0)),                          # |pos| = 1.06 < 1.15: c <= 0 on every primary ray
    "inside_ball_looking_out": dict(pos=(0.3, 0.2, 1.0), look=(0.2, 0.1, 1)),
    "outside_looking_away": dict(pos=(0, 0, 1.3), look=(0, 0.1, 1)),   # c > 0, b >= 0: no evaluation at all
    "outside_looking_across": dict(pos=(0, 0, 1.3), look=(1, 0, -0.2)),  # b changes sign across the frame
    "tangent": dict(pos=(1.15, 0, 3.0)),                               # the centre column's rays graze R = 1.15: disc ~ 0
    "tangent_wide_ball": dict(pos=(2.1, 0, 4.0), julia=(1.5, 0.0)),    # the same for R = 2.1
    "rotated_scaled": dict(model=h.scale(1.2, 1.2, 1.2) @ h.rotation((1, 2, 0.5), 0.6), sf=1.2),
}


@pytest.mark.parametrize("view", sorted(VIEWS))
def test_views(renderer, view):
    W, H = 61, 37
    check(renderer, bulb_scene(W, H, nl=3, **VIEWS[view]), abi.default_settings(), W, H, view)


@pytest.mark.parametrize("far", [2.2, 2.6, 3.0])
def test_far_plane_in_front_of_the_balls_exit(renderer, far):
    """far < t_exit on some rays and not on others: primary rays from 1.95 and 4.5 away, and their shadow rays."""
    W, H = 45, 29
    for view in ("close_up", "rotated_scaled"):
        check(renderer, bulb_scene(W, H, nl=3, far=far, **VIEWS[view]), abi.default_settings(), W, H, f"{view} far={far}")
    check(renderer, bulb_scene(W, H, nl=3, far=far + 1.5), abi.default_settings(), W, H, f"c3 far={far + 1.5}")


@pytest.mark.parametrize("sf", [0.05, 0.01, 0.009])
def test_scale_factor_at_the_culls_limits(renderer, sf):
    """0.05: the last scale of the R = 1.15 ball; 0.01: the last of R = 2.1; 0.009: the cull is off."""
    W, H = 45, 29
    check(renderer, bulb_scene(W, H, nl=3, **scaled(sf)), abi.default_settings(), W, H, f"scaleFactor {sf}")
    rot = h.scale(sf, sf, sf) @ h.rotation((1, 2, 0.5), 0.6)
    check(renderer, bulb_scene(W, H, nl=2, **dict(scaled(sf), model=rot)), abi.default_settings(), W, H, f"rotated scaleFactor {sf}")


@pytest.mark.parametrize("seed", [(1.14, 0.0), (1.1401, 0.0), (0.0, -1.1402), (2.0, 0.0), (2.0001, 0.0), (1.2, 1.6), (1.2001, 1.6)])
def test_julia_seed_at_the_culls_limits(renderer, seed):
    """|seed|² at 1.2996 and just above (the ball grows to 2.1), at 4.0 and just above (the cull is off)."""
    W, H = 45, 29
    for view in ("c3_camera", "close_up"):
        check(renderer, bulb_scene(W, H, nl=2, julia=seed, **VIEWS[view]), abi.default_settings(), W, H, f"{view} seed {seed}")


@pytest.mark.parametrize("steps", [0, 1, 2])
def test_step_caps(renderer, steps):
    W, H = 45, 29
    for view in ("c3_camera", "close_up", "inside_ball", "outside_looking_away"):
        check(renderer, bulb_scene(W, H, nl=3, **VIEWS[view]), abi.default_settings(maxSteps=steps), W, H, f"{view} maxSteps={steps}")


@pytest.mark.parametrize("nl", [1, 3, abi.RM_MAX_LIGHTS])
def test_directional_lights(renderer, nl):
    W, H = 61, 37
    for view in ("close_up", "inside_ball"):
        check(renderer, bulb_scene(W, H, nl=nl, **VIEWS[view]), abi.default_settings(), W, H, f"{view} nl={nl}")


def test_point_light_leaves_the_pool(renderer):
    """A point light: the frame's shadow rays go through march<SHADOW> with the distance to the light as their end."""
    W, H = 45, 29
    lights = [h.make_light(abi.RM_LIGHT_POINT, (1, 1, 1), pos=(0.4, 0.9, 1.6)),
              h.make_light(abi.RM_LIGHT_DIRECTIONAL, (1.5, 1.1, 0.7), (0, -1, 0)),
              h.make_light(abi.RM_LIGHT_POINT, (0.4, 0.6, 0.9), pos=(-3.0, 0.5, -2.0))]  # behind the bulb, outside the ball
    for view in ("c3_camera", "close_up"):
        check(renderer, bulb_scene(W, H, lights=lights, **VIEWS[view]), abi.default_settings(), W, H, f"point light, {view}")


def test_4x16_tiles(renderer):
    L = lib()
    W, H = 61, 37
    try:
        assert L.rm_debug_set_tile_shape(2) == 0
        for view in ("c3_camera", "inside_ball", "tangent"):
            check(renderer, bulb_scene(W, H, nl=3, **VIEWS[view]), abi.default_settings(), W, H, f"4x16 {view}")
    finally:
        L.rm_debug_set_tile_shape(-1)


def test_batch(renderer):
    W, H = 45, 29
    scene = bulb_scene(W, H, nl=3)
    s = abi.default_settings()
    cams = [h.make_camera(v.get("pos", (0, 0, 4.5)), v.get("look", (0, 0, -1)), (0, 1, 0), 30.0, W, H)
            for v in (VIEWS[k] for k in ("c3_camera", "close_up", "inside_ball", "outside_looking_away", "tangent"))]
    got = renderer.render_batch(tables_of(scene), s, W, H, cams).cpu().numpy()
    for i, cam in enumerate(cams):
        assert_bit_equal(got[i], h.oracle_render((cam,) + scene[1:], s, W, H), f"batch frame {i}")


# Executed sceneEvals of the 61x37 c3 frame below at the parent of this change, commit 3018f58 ("Tests: G-buffer on random tables,
# ragged frames, float64 arbiter"), measured once on an MI355X (its bulbIters: 115162; the reference's work: 94473 / 183451).
# With the marches that end before a certain-miss evaluation the same frame executes 49419.
PARENT_C3_EXECUTED_SCENE_EVALS = 51732
# Executed sceneEvals of the 45x29 inside_ball frame at the same parent commit, and equally of a build of this change whose
# shadowPool keeps the former order while march() ends early: the view that pins the pool's own path (this change: 74826).
POOL_FORMER_ORDER_INSIDE_BALL_SCENE_EVALS = 76059


def test_counters_executed_do_not_exceed_the_references(renderer):
    W, H = 61, 37
    scene = bulb_scene(W, H, nl=3)
    s = abi.default_settings()
    ref, rc = h.oracle_render(scene, s, W, H, counters=True)
    out, c1 = renderer.render_counted(tables_of(scene), s, W, H, abi.RM_COUNT_REFERENCE)
    assert_bit_equal(out.cpu().numpy(), ref, "reference-counted")
    for f in ("sceneEvals", "bulbIters", "hitPixels", "shadedPoints"):
        assert getattr(c1, f) == getattr(rc, f), f
    out, c2 = renderer.render_counted(tables_of(scene), s, W, H, abi.RM_COUNT_EXECUTED)
    assert_bit_equal(out.cpu().numpy(), ref, "executed-counted")
    print(f"c3 61x37: executed sceneEvals {c2.sceneEvals} bulbIters {c2.bulbIters}; reference {c1.sceneEvals} {c1.bulbIters}")
    assert 0 < c2.sceneEvals < PARENT_C3_EXECUTED_SCENE_EVALS
    assert c2.sceneEvals <= c1.sceneEvals and c2.bulbIters <= c1.bulbIters and c2.hitPixels == c1.hitPixels
    # the other views: executed <= reference still holds
    for view in ("close_up", "inside_ball", "outside_looking_away"):
        scene = bulb_scene(45, 29, nl=3, **VIEWS[view])
        _, a = renderer.render_counted(tables_of(scene), s, 45, 29, abi.RM_COUNT_REFERENCE)
        _, b = renderer.render_counted(tables_of(scene), s, 45, 29, abi.RM_COUNT_EXECUTED)
        assert b.sceneEvals <= a.sceneEvals and b.bulbIters <= a.bulbIters and b.hitPixels == a.hitPixels, view
        if view == "inside_ball":  # primary rays start inside the ball, so only the shadow pool's rays can end ahead of an evaluation
            assert b.sceneEvals < POOL_FORMER_ORDER_INSIDE_BALL_SCENE_EVALS
        if view == "outside_looking_away":  # no ray enters the ball: nothing is evaluated (the parent: one evaluation per pixel)
            assert b.sceneEvals == 0 and b.bulbIters == 0


# ---------------------------------------------------------------- part B: the probe
def _probe_tables(objs, g):
    arr = (abi.RmObject * len(objs))(*objs)
    return types.SimpleNamespace(objects=arr, num_objects=len(objs), globals_=g)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _oracle(t, s, pts):
    p = np.ascontiguousarray(pts, dtype=F32)
    out = np.empty((len(p), 6), dtype=F32)
    assert h.oracle().rmo_probe_sdscene_trap4(t.objects, t.num_objects, C.byref(t.globals_), C.byref(s), h.fptr(p), h.fptr(out),
                                              len(p)) == 0
    return out


def _edge_points(rng):
    nan = np.nan
    P = [(0, 0, 0), (-0.0, 0, -0.0)]                                                     # the origin: m = 0
    P += [(0, 0.7, 0), (0, -0.7, 0), (0, 1.3, 0), (-0.0, 0.2, 0)]                        # the y axis
    P += [(1e-20, 0, 0), (6e-21, 6e-21, 6e-21), (0, 1e-20, 0), (1e-23, 0, 1e-23)]        # m denormal or zero
    P += [(1e10, 0, 0), (6e9, -6e9, 5e9), (0, 1e10, 0)]                                  # |p| = 1e10: m finite, the first step overflows
    P += [(3e19, 0, 0), (1.7e19, 1.7e19, -1.7e19), (0, 0, -3e19)]                        # |p| = 3e19: m overflows
    P += [(nan, 0.5, 0.5), (0.5, nan, 0.5), (0.5, 0.5, nan)]
    # dz = 8·|p|^7 + 1 after the first step, which also sends m to inf: around the reciprocal's 2^126 from |p| = 1.9e5, inf from 3e5
    P += [(r, 0, 0) for r in (1.0e5, 1.9e5, 1.95e5, 2.0e5, 2.5e5, 3.0e5)] + [(1.1e5, -1.2e5, 1.1e5), (1.2e5, 1.2e5, -1.2e5)]
    d = rng.normal(size=(12, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    P += [tuple(v) for v in d * rng.uniform(0.75, 1.0, (12, 1))]                         # interior: every iteration runs, m <= 2 at the end
    return np.concatenate([np.array(P, dtype=F32), _boundary_points(rng)])


def _boundary_points(rng, n=12):
    """Points of the plain bulb's boundary to binary32 precision (bisection with the oracle on `escaped within 64 iterations`):
    their orbits stay near |w| = 1 for dozens of iterations, which is where dz grows largest without the orbit escaping.  (At
    power 8 that is about 1e11 after 64 iterations, far from the reciprocal's 2^126: dz leaves the fused range only through
    non-finite arithmetic, the large-|p| points above.)"""
    t = _probe_tables([h.make_object(abi.RM_MANDELBULB)], h.make_globals())
    s = abi.default_settings(fractalIters=64)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    lo, hi = np.full(n, 0.4), np.full(n, 1.4)
    for _ in range(40):
        mid = (lo + hi) / 2
        esc = _oracle(t, s, (d * mid[:, None]).astype(F32))[:, 2] > 2  # trap.x is the final m
        hi, lo = np.where(esc, mid, hi), np.where(esc, lo, mid)
    return (d * lo[:, None]).astype(F32)


def _ordinary_points(rng):
    d = rng.normal(size=(63, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[:, 1] *= 0.9
    r = np.r_[rng.uniform(0.35, 1.0, 32), rng.uniform(1.2, 1.5, 31)]  # iterate to the cap, or bail out at once: both fused exits
    return (d * r[:, None]).astype(F32)


def _layout(nE):
    """Point numbers (0…62 ordinary, 63… edge) in wave order: per edge point a wave of the 63 ordinary points with it at a lane
    of its own; the edge points alone; the ordinary points alone (a whole wave on the fused path); a partial last wave."""
    ids = []
    for e in range(nE):
        w = list(range(63))
        w.insert((7 * e) % 64, 63 + e)
        ids += w
    edge = [63 + e for e in range(nE)]
    ids += edge + edge[:(-nE) % 64]
    ids += list(range(63)) + [0]
    ids += list(range(20, 37))
    return np.array(ids)


def test_estimate_guard_on_mixed_waves(renderer):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(23)
    E, O = _edge_points(rng), _ordinary_points(rng)
    P = np.concatenate([O, E])
    ids = _layout(len(E))
    dev_pts = torch.from_numpy(np.ascontiguousarray(P[ids])).to(renderer.device)
    bulb = lambda **kw: h.make_object(abi.RM_MANDELBULB, **kw)  # noqa: E731
    rot = bulb(model=h.translate(0.1, -0.2, 0.05) @ h.rotation((1, 2, 3), 0.7) @ h.scale(1.5, 1.5, 1.5), scale_factor=1.5)
    scenes = [("plain", [bulb()], h.make_globals(), True), ("rotated", [rot], h.make_globals(), False),
              ("julia", [bulb()], h.make_globals(julia=(0.35, -0.2)), False), ("power6", [bulb()], h.make_globals(power=6.0), False)]
    algebraic = abi.default_settings().features | abi.RM_FEAT_BULB_POWER8_ALGEBRAIC
    for name, objs, g, plain_ok in scenes:
        t = _probe_tables(objs, g)
        settings = [(f"iters {k}", abi.default_settings(fractalIters=k)) for k in (0, 1, 12, 20, 40, 64)]
        if g.power == 8.0:
            settings += [(f"algebraic iters {k}", abi.default_settings(fractalIters=k, features=algebraic)) for k in (1, 20, 64)]
        for sname, s in settings:
            ref = _oracle(t, s, P)
            ref = ref[ids]
            variants = [(1, c, tr) for c in (0, 1, 2) for tr in (0, 1)] + ([(2, 0, 0), (2, 0, 1)] if plain_ok else [])
            for cls, count, trap in variants:
                dev = renderer.probe_sdscene_variant(t, s, dev_pts, bulb_class=cls, count=count, trap=trap).cpu().numpy()
                what = f"{name}, {sname}, class {cls} count {count} trap {trap}"
                for col in (0, 1):
                    bad = _bits(dev[:, col]) != _bits(ref[:, col])
                    assert not bad.any(), f"{what}: column {col} differs at points {ids[bad][:8]}: {dev[bad, col][:4]} vs {ref[bad, col][:4]}"
                if trap:
                    for col in (2, 3, 4, 5):  # a NaN produced by arithmetic has no defined bits
                        bad = (_bits(dev[:, col]) != _bits(ref[:, col])) & ~(np.isnan(dev[:, col]) & np.isnan(ref[:, col]))
                        assert not bad.any(), f"{what}: trap[{col - 2}] differs at points {ids[bad][:8]}"
