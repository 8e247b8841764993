"""The specification of rm_shade_points for the tests: tests/points_spec/rm_points_spec.c, which includes the oracle's source and
restates the header's definition with the oracle's own sdScene, getNormal, bumpNormal, calcAO and getPhong, built on demand and
loaded with ctypes by helpers.load_spec.  Nothing under oracle/ is touched.  Also the point sets that more than one points test
module uses."""
import ctypes as C

import numpy as np

import helpers as h
import trace_helpers as th
from raymarcher_amd import abi

P = C.POINTER
SIGNATURES = {"rmo_spec_points": (C.c_int, [P(abi.RmObject), C.c_int, P(abi.RmLight), C.c_int, P(abi.RmGlobals), P(abi.RmSettings),
                                            P(abi.RmResources), P(C.c_float), P(C.c_float), C.c_int, C.c_float, C.c_float, C.c_float,
                                            C.c_int, P(C.c_float), P(C.c_float), P(C.c_float)])}
PATH_POINTS = 17  # rm_debug_last_path() of a launch of rm_shade_points
INF = float("inf")


def spec():
    """ctypes handle of the spec library (helpers.load_spec: rebuilt when a source it is made of is newer)."""
    return h.load_spec("points", SIGNATURES)


def points4(p):
    """(n, 3) or (n, 4) → float32 (n, 4), the fourth word 0 where it was missing."""
    p = np.asarray(p, dtype=np.float32).reshape(len(p), -1)
    out = np.zeros((len(p), 4), dtype=np.float32)
    out[:, :p.shape[1]] = p
    return out


def spec_points(scene, s, points, view=None, far=100.0, iso=0.001, max_move=INF, project=0, res=None, outputs="sac", expect=0):
    """(surface float32 (n, 8), ao float32 (n), colour float32 (n, 4)) of `points` by the specification; an output whose letter
    (s, a, c) is not in `outputs` is not asked for and comes back None.  scene: the tests' tuple (camera, objects, count, lights,
    count, globals) — the camera is not read; res: the resources dict of scene_builders.resource_case."""
    pts = points4(points)
    vw = None if view is None else points4(view)
    n = len(pts)
    sf = np.full((n, 8), np.nan, dtype=np.float32) if "s" in outputs else None
    ao = np.full((n,), np.nan, dtype=np.float32) if "a" in outputs else None
    col = np.full((n, 4), np.nan, dtype=np.float32) if "c" in outputs else None
    r, _keep = h.host_resources(**(res or {}))
    _, objs, no, lights, nl, g = scene[:6]
    ptr = lambda a: None if a is None else h.fptr(a)  # noqa: E731
    st = spec().rmo_spec_points(objs, no, lights, nl, C.byref(g), C.byref(s), C.byref(r), h.fptr(pts), ptr(vw), n, far, iso, max_move,
                                project, ptr(sf), ptr(ao), ptr(col))
    assert st == expect, f"spec status {st}"
    return sf, ao, col


def ids_of(surface):
    return np.ascontiguousarray(surface[:, 7]).view(np.int32)


def hit_points(scene, s, W, H):
    """The primary rays of the scene's camera that the trace spec reports as hits → (rays (m, 8), hits (m, 8) RmRayHit rows).  The
    hit position of a row is rd·t + ro in render's fused form: the spec's `position`."""
    cam, objs, no, _, _, g = scene[:6]
    rays = th.spec_primary_rays(cam, W, H)
    hits = th.spec_trace(objs, no, g, s, rays)
    ok = th.ids_of(hits) >= 0
    return rays[ok], hits[ok]


def invalid_points():
    """Every kind of invalid (point, view) pair, one row each → (points (k, 4), views (k, 4), rows whose POINT alone is invalid).  The
    fourth words are NaN: they are not read."""
    inf, nan = np.inf, np.nan
    pts, views, point_bad = [], [], []
    for k in range(3):
        for bad in (nan, inf, -inf):
            p = [0.1, 0.2, 0.3, nan]
            p[k] = bad
            pts.append(p); views.append([0.0, 0.0, -1.0, nan]); point_bad.append(True)
            v = [0.0, 0.0, -1.0, nan]
            v[k] = bad
            pts.append([0.1, 0.2, 0.3, nan]); views.append(v); point_bad.append(False)
    pts.append([0.1, 0.2, 0.3, nan]); views.append([0.0, 0.0, 0.0, nan]); point_bad.append(False)
    pts.append([0.1, 0.2, 0.3, nan]); views.append([-0.0, 0.0, -0.0, nan]); point_bad.append(False)
    return np.array(pts, dtype=np.float32), np.array(views, dtype=np.float32), np.array(point_bad)


def mesh_vertices(scene, s, dims=(9, 9, 9), iso=0.001):
    """The vertices (n, 3) of the NumPy surface-nets spec on a dims lattice of the oracle's sdScene over the table's cull ball: what
    rm_sdf_mesh hands rm_shade_points — points up to half a cell off the surface."""
    import sdf_mesh_spec as M
    _, objs, no, _, _, g = scene[:6]
    centre, radius = th.cull_bounds(objs, no, g)
    lo = np.asarray(centre, dtype=np.float64) - radius
    origin = lo.astype(np.float32)
    step = np.full(3, 2.0 * radius / (dims[0] - 1), dtype=np.float32)
    pts = M.lattice_points(origin, step, dims)
    out = np.empty((len(pts), 4), dtype=np.float32)
    assert h.oracle().rmo_probe_sdscene(objs, no, C.byref(g), C.byref(s), h.fptr(pts), h.fptr(out), len(pts)) == 0
    nx, ny, nz = dims
    mesh = M.surface_nets(np.ascontiguousarray(out[:, 0]).reshape(nz, ny, nx), origin, step, np.float32(iso))
    return np.ascontiguousarray(mesh["vertices"][:, 0:3])


def point_set(scene, s, n, seed, W=40, H=40):
    """n seeded (points (n, 4), views (n, 4)) around the scene, the kinds cycling along the array so that every wave of 64 holds all
    of them: hit points of the camera's rays seen along those rays (kinds 0-2), surface-nets vertices of a 9×9×9 lattice (3), points
    deep inside (4: hit points pushed 0.2 under the surface), points far outside (5), every kind of invalid point and view (6), and
    points a few hundredths off the surface, what a projection is for (7).  A scene without a hit (the empty table) gets seeded points
    around the origin in their place.  The fourth words are NaN where nothing may read them."""
    rng = np.random.default_rng(seed)
    rays, hits = hit_points(scene, s, W, H) if scene[2] else (np.zeros((0, 8), np.float32),) * 2
    pts = np.full((n, 4), np.nan, dtype=np.float32)
    views = np.full((n, 4), np.nan, dtype=np.float32)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    views[:, 0:3] = d * rng.uniform(0.3, 2.0, (n, 1))  # directions as given: not unit
    pts[:, 0:3] = rng.uniform(-1.5, 1.5, (n, 3))
    kind = np.arange(n) % 8
    if len(hits):
        pick = rng.integers(0, len(hits), n)
        on = np.isin(kind, (0, 1, 2, 4, 7))
        pts[on, 0:3] = hits[pick[on], 4:7]
        views[kind <= 2, 0:3] = rays[pick[kind <= 2], 4:7]
        pts[kind == 4, 0:3] -= np.float32(0.2) * hits[pick[kind == 4], 0:3]
        pts[kind == 7, 0:3] += rng.uniform(-0.04, 0.04, ((kind == 7).sum(), 1)).astype(np.float32) * hits[pick[kind == 7], 0:3]
        verts = mesh_vertices(scene, s)
        if len(verts):
            pts[kind == 3, 0:3] = verts[rng.integers(0, len(verts), (kind == 3).sum())]
    pts[kind == 5, 0:3] = (d * rng.uniform(50.0, 400.0, (n, 1)))[kind == 5]
    bp, bv, _ = invalid_points()
    for j, i in enumerate(np.nonzero(kind == 6)[0]):
        pts[i], views[i] = bp[j % len(bp)], bv[j % len(bp)]
    return pts, views
