"""The specification of rm_trace_rays and rm_camera_rays for the tests: tests/trace_spec/rm_trace_spec.c, which includes the oracle's
source and calls its own raymarch, getNormal, bumpNormal, v3_madd and softshadow as the definition reads, built on demand and
loaded with ctypes by helpers.load_spec.  Nothing under oracle/ is touched.  Also the seeded ray sets and object tables that more
than one trace test module uses."""
import ctypes as C

import numpy as np

import helpers as h
from raymarcher_amd import abi

P = C.POINTER
SIGNATURES = {
    "rmo_spec_trace": (C.c_int, [P(abi.RmObject), C.c_int, P(abi.RmGlobals), P(abi.RmSettings), P(C.c_float), C.c_int, C.c_uint,
                                 P(C.c_float)]),
    "rmo_spec_primary_rays": (C.c_int, [P(abi.RmCamera), C.c_int, C.c_int, P(C.c_int32), C.c_int, P(C.c_float)]),
}
MODES = {"closest": abi.RM_TRACE_CLOSEST, "no_normal": abi.RM_TRACE_NO_NORMAL, "occlusion": abi.RM_TRACE_OCCLUSION}
bits, assert_bits = h.bits, h.assert_bit_equal


def spec():
    """ctypes handle of the spec library (helpers.load_spec: rebuilt when a source it is made of is newer)."""
    return h.load_spec("trace", SIGNATURES)


def spec_trace(objs, num_objects, g, s, rays, mode="closest"):
    """The RmRayHit rows of `rays` (float32 (n, 8)) by the specification → float32 (n, 8); word 7 holds the int32 object index."""
    rays = np.ascontiguousarray(rays, dtype=np.float32)
    hits = np.empty_like(rays)
    st = spec().rmo_spec_trace(objs, num_objects, C.byref(g), C.byref(s), h.fptr(rays), len(rays), MODES[mode], h.fptr(hits))
    assert st == 0, f"spec status {st}"
    return hits


def spec_primary_rays(cam, W, H, pixels=None):
    """The primary rays of a frame's pixels by the specification → float32 (n, 8), row-major with row 0 at the bottom, or of the
    listed (x, y) pairs."""
    xy = None if pixels is None else np.ascontiguousarray(pixels, dtype=np.int32).reshape(-1, 2)
    n = W * H if xy is None else len(xy)
    rays = np.empty((n, 8), dtype=np.float32)
    st = spec().rmo_spec_primary_rays(C.byref(cam), W, H, None if xy is None else xy.ctypes.data_as(C.POINTER(C.c_int32)), n,
                                      h.fptr(rays))
    assert st == 0, f"spec status {st}"
    return rays


def ids_of(hits):
    return np.ascontiguousarray(hits[:, 7]).view(np.int32)


def make_rays(origin, direction, tmax):
    """float32 (n, 8) RmRay rows from (n, 3) origins, (n, 3) directions and tMax (scalar or (n,))."""
    o = np.asarray(origin, dtype=np.float32).reshape(-1, 3)
    r = np.zeros((len(o), 8), dtype=np.float32)
    r[:, 0:3] = o
    r[:, 3] = tmax
    r[:, 4:7] = np.asarray(direction, dtype=np.float32).reshape(-1, 3)
    return r


def invalid_rays():
    """Every kind of invalid ray (the header's list), one row each, and two valid rays that look similar (tMax = +inf, −0)."""
    inf, nan = np.inf, np.nan
    rows = []
    for k in range(3):
        for bad in (nan, inf, -inf):
            o, d = [0.1, 0.2, 5.0], [0.0, 0.0, -1.0]
            o[k] = bad
            rows.append(o + [10.0] + d + [0.0])
            o, d = [0.1, 0.2, 5.0], [0.0, 0.0, -1.0]
            d[k] = bad
            rows.append(o + [10.0] + d + [0.0])
    rows.append([0.1, 0.2, 5.0, 10.0, 0.0, 0.0, 0.0, 0.0])      # dir all zeros
    rows.append([0.1, 0.2, 5.0, 10.0, -0.0, 0.0, -0.0, 0.0])    # … of either sign
    rows.append([0.1, 0.2, 5.0, nan, 0.0, 0.0, -1.0, 0.0])      # tMax NaN
    rows.append([0.1, 0.2, 5.0, -1.0, 0.0, 0.0, -1.0, 0.0])     # tMax negative
    rows.append([0.1, 0.2, 5.0, -inf, 0.0, 0.0, -1.0, 0.0])
    n_invalid = len(rows)
    rows.append([0.1, 0.2, 5.0, inf, 0.0, 0.0, -1.0, 0.0])      # valid: tMax = +inf
    rows.append([0.1, 0.2, 5.0, -0.0, 0.0, 0.0, -1.0, 0.0])     # valid: tMax = −0
    return np.array(rows, dtype=np.float32), n_invalid


def cull_bounds(objs, num_objects, g):
    """(centre, radius) of the ball the launcher stages for ending marches (rm_debug_cull_bounds), or ((0, 0, 0), 3) for a table
    without one: where 'inside, on and outside the cull ball' is."""
    from raymarcher_amd import lib
    out = (C.c_float * 14)()
    assert lib().rm_debug_cull_bounds(objs, num_objects, C.byref(g), out) == 0
    if out[0] != 0.0 and out[4] > 0.0:
        return (out[1], out[2], out[3]), float(np.sqrt(out[4]))
    return (0.0, 0.0, 0.0), 3.0


def seeded_rays(rng, n, centre=(0.0, 0.0, 0.0), radius=2.0):
    """n seeded rays around a scene whose cull ball is (centre, radius): origins inside, on and outside that ball (and so inside
    and outside the cull box) and far away, directions of length 0.3 to 3 toward the scene, axis-aligned directions with exact zero
    components, rays pointing away from everything, tMax of 0, of less than the distance to the ball and of 1e6, and every kind of
    invalid ray.  The kinds cycle along the array, so every wave of 64 holds all of them."""
    c = np.asarray(centre, dtype=np.float64)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    kind = np.arange(n) % 16
    dist = np.select([kind % 4 == 0, kind % 4 == 1, kind % 4 == 2], [rng.uniform(0.0, 0.9, n) * radius, np.full(n, radius),
                                                                      rng.uniform(1.2, 4.0, n) * radius], rng.uniform(20.0, 400.0, n))
    dist[kind == 9] = 3.0 * radius
    origin = c + u * dist[:, None]
    target = c + rng.uniform(-0.5, 0.5, (n, 3)) * radius
    d = target - origin
    d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-9)
    d *= rng.uniform(0.3, 3.0, (n, 1))
    tmax = np.full(n, 1000.0)
    d[kind == 5] *= -1.0                                  # pointing away from everything
    axis = (kind == 6) | (kind == 7)                      # axis-aligned: two components are exact zeros
    ax = rng.integers(0, 3, n)
    rows = np.arange(n)
    origin[kind == 7] = (c + rng.uniform(-0.3, 0.3, (n, 3)) * radius)[kind == 7]
    origin[kind == 7, ax[kind == 7]] += (rng.choice([-2.5, 2.5], n) * radius)[kind == 7]   # outside, on a line through the scene
    axd = np.zeros((n, 3))
    axd[rows, ax] = np.where(origin[rows, ax] > c[ax], -1.0, 1.0) * rng.uniform(0.3, 3.0, n)
    d[axis] = axd[axis]
    tmax[kind == 8] = 0.0
    tmax[kind == 9] = radius / np.linalg.norm(d[kind == 9], axis=1)   # ends a ball's radius short of the ball
    tmax[kind == 10] = 1e6
    rays = make_rays(origin, d, tmax)
    bad, _ = invalid_rays()
    for j, i in enumerate(np.nonzero(kind == 11)[0]):
        rays[i] = bad[j % len(bad)]
    return rays


def sphere_table(scale, centre):
    """One RM_SPHERE of radius 0.5·scale at `centre` (the loader's uniform scale: scaleFactor = scale)."""
    return h.table([h.make_object(abi.RM_SPHERE, model=h.translate(*centre) @ h.scale(scale, scale, scale), scale_factor=float(scale))])


def sphere_rays(rng, n, centre, R, impact_lo, impact_hi, tmax=100.0):
    """n seeded unit-direction rays from distance 3 to 8 of `centre` whose line passes the centre at impact_lo·R … impact_hi·R →
    (rays float32 (n, 8), float64 origins, float64 unit directions as stored)."""
    c = np.asarray(centre, dtype=np.float64)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    D = rng.uniform(3.0, 8.0, (n, 1))
    origin = c + u * D
    w = np.cross(u, rng.normal(size=(n, 3)))
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    sin = rng.uniform(impact_lo, impact_hi, (n, 1)) * R / D  # the line passes the centre at D·sin θ, θ its angle to −u
    d = -u * np.sqrt(1.0 - sin * sin) + w * sin
    rays = make_rays(origin, d, tmax)
    return rays, rays[:, 0:3].astype(np.float64), rays[:, 4:7].astype(np.float64)
