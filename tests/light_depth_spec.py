"""The three definitions of the probe depth moments (include/raymarcher_amd.h) in NumPy, written from the header's text and sharing
no code with the library: rm_probe_depth_weights in float64 rounded once, rm_light_probes_depth's leaves and tree in float32 from
distances that are already there, and step 5a of rm_light_grid_irradiance_visible in float32 on top of light_grid_spec's steps.
Every float32 array below stays float32 and every operation on it is one rounded binary32 operation."""
import math

import numpy as np

import light_grid_spec as G
import light_probes_spec as L

f32 = np.float32
TEXELS, SIDE = 64, 8
FLOOR = f32(1.0e-6)  # RM_LIGHT_GRID_VIS_FLOOR
DEPTH = np.dtype([("moments", "<f4", (TEXELS, 2))])  # RmProbeDepth
assert DEPTH.itemsize == 512


# ---------------------------------------------------------------- the map
def oct_decode(u, v):
    """The unit vector of the point (u, v) of the unfolded octahedron, float64."""
    z = 1.0 - abs(u) - abs(v)
    x, y = u, v
    if z < 0.0:
        x, y = (1.0 - abs(v)) * (1.0 if u >= 0.0 else -1.0), (1.0 - abs(u)) * (1.0 if v >= 0.0 else -1.0)
    length = math.sqrt(x * x + y * y + z * z)
    return (x / length, y / length, z / length)


def texel_centres():
    """(64, 3) float64: c_x of texel x = tx + 8·ty."""
    return np.array([oct_decode(((x % SIDE + 0.5) / SIDE) * 2.0 - 1.0, ((x // SIDE + 0.5) / SIDE) * 2.0 - 1.0) for x in range(TEXELS)])


# ---------------------------------------------------------------- rm_probe_depth_weights, in float64
def depth_weights(table, K, sets, sharpness):
    """float32 (sets·K, 64): the header's text, row by row in ascending k, scalars of Python's own float64."""
    table = np.asarray(table, f32).reshape(sets * K, 16)
    ok = L.valid_rows(table)
    centres = texel_centres()
    sharp = float(f32(sharpness))
    out = np.zeros((sets * K, TEXELS), f32)
    for s in range(sets):
        rows = range(s * K, (s + 1) * K)
        dots = {}
        for k in rows:
            if ok[k]:
                dx, dy, dz = (float(c) for c in table[k, 0:3])
                length = math.sqrt((dx * dx + dy * dy) + dz * dz)
                dots[k] = [(c[0] * (dx / length) + c[1] * (dy / length)) + c[2] * (dz / length) for c in centres]
        for x in range(TEXELS):
            total, raw = 0.0, {}
            for k in rows:
                if ok[k]:
                    raw[k] = math.pow(max(dots[k][x], 0.0), sharp)
                    total += raw[k]
            if total == 0.0 and raw:
                best = max(dots[k][x] for k in raw)
                nearest = min(k for k in raw if dots[k][x] == best)
                out[nearest, x] = 1.0
            else:
                for k in raw:
                    out[k, x] = raw[k] / total  # the one rounding, on assignment
    return out


# ---------------------------------------------------------------- rm_light_probes_depth from its rays' distances
def moments(positions, table, weights, K, sets, t, first=0):
    """DEPTH records (n) from t (n·K), the distances rm_trace_rays stores for L.rays(positions, table, K, sets, maxDistance):
    r = t of a valid row and +0 of an invalid one, leaves w·r and w·(r·r), the pairwise tree over k."""
    n, K = len(positions), int(K)
    table, weights = np.asarray(table, f32).reshape(-1, 16), np.asarray(weights, f32).reshape(-1, TEXELS)
    which = L.rows_of(n, K, sets, first)
    r = np.where(L.valid_rows(table)[which], np.asarray(t, f32).reshape(n, K), f32(0)).astype(f32)
    w = weights[which]  # (n, K, 64)
    with np.errstate(all="ignore"):
        rr = r * r
        leaves = np.stack([w * r[:, :, None], w * rr[:, :, None]], axis=3).reshape(n, K, 2 * TEXELS)
    assert leaves.dtype == f32
    sums = L.tree(leaves).reshape(n, TEXELS, 2)
    out = np.zeros(n, DEPTH)
    ok = L.valid_positions(positions)
    out["moments"][ok] = sums[ok]
    return out


# ---------------------------------------------------------------- step 5a
def _texel(o):
    with np.errstate(all="ignore"):
        u = o * f32(4) + f32(3.5)
        u = np.where(u > f32(0), u, f32(0)).astype(f32)
        u = np.where(u > f32(7), f32(7), u).astype(f32)
        i = np.minimum(np.floor(u).astype(np.int64), SIDE - 2)
        f = u - i.astype(f32)
    assert f.dtype == f32
    return i, f


def visibility(q, probe_position, depth):
    """vis (m) float32 of points q (m, 3) from probes at probe_position (m, 3) whose moments are depth (m, 64, 2)."""
    q, pp, depth = np.asarray(q, f32), np.asarray(probe_position, f32), np.asarray(depth, f32)
    with np.errstate(all="ignore"):
        v = q - pp
        vx, vy, vz = v[:, 0], v[:, 1], v[:, 2]
        r = np.sqrt((vx * vx + vy * vy) + vz * vz)
        l1 = (np.abs(vx) + np.abs(vy)) + np.abs(vz)
        ox, oy = vx / l1, vy / l1
        sx, sy = np.where(ox >= f32(0), f32(1), f32(-1)).astype(f32), np.where(oy >= f32(0), f32(1), f32(-1)).astype(f32)
        fx, fy = (f32(1) - np.abs(oy)) * sx, (f32(1) - np.abs(ox)) * sy
        ox, oy = np.where(vz < f32(0), fx, ox).astype(f32), np.where(vz < f32(0), fy, oy).astype(f32)
        ix, tx = _texel(ox)
        iy, ty = _texel(oy)
        x0 = ix + SIDE * iy
        at = np.arange(len(q))
        a, b, c, d = depth[at, x0], depth[at, x0 + 1], depth[at, x0 + SIDE], depth[at, x0 + SIDE + 1]  # (m, 2) each
        gx, gy = (f32(1) - tx)[:, None], (f32(1) - ty)[:, None]
        blend = (a * gx + b * tx[:, None]) * gy + (c * gx + d * tx[:, None]) * ty[:, None]
        m, m2 = blend[:, 0], blend[:, 1]
        var = np.abs(m2 - m * m)
        dd = r - m
        den = var + dd * dd
        cheb = np.where(den == f32(0), f32(1), var / den).astype(f32)
        vis = (cheb * cheb) * cheb
        vis = np.where(vis > FLOOR, vis, FLOOR).astype(f32)
        vis = np.where((r == f32(0)) | (r <= m), f32(1), vis).astype(f32)
    assert vis.dtype == f32
    return vis


def grid_light_visible(probes, depth, dims, origin, step, points, normals, facing, normal_bias):
    """rm_light_grid_irradiance_visible by the definition → GRIDLIGHT records (n): light_grid_spec's steps with w_c·vis between."""
    probes, depth = np.asarray(probes), np.asarray(depth)
    assert probes.dtype == G.PROBE and depth.dtype == DEPTH and len(depth) == len(probes) == int(np.prod(np.asarray(dims, np.int64)))
    pts, nrm = np.asarray(points, f32)[:, 0:3], np.asarray(normals, f32)[:, 0:3]
    ok = G.valid_points(pts, nrm)
    out = np.zeros(len(pts), G.GRIDLIGHT)
    out["probes"][~ok] = G.INVALID
    if ok.any():
        p, n = pts[ok], nrm[ok]
        index, valid, w = G.corners(probes["hits"], dims, origin, step, p, n, facing)
        pos = G.positions(origin, step, dims)
        with np.errstate(all="ignore"):
            q = p + f32(normal_bias) * n
            assert q.dtype == f32
            for c in range(8):
                # an invalid probe's depth words are not looked at: its weight stays the +0 that corners gave it
                vis = visibility(q, pos[index[:, c]], np.where(valid[:, c, None, None], depth["moments"][index[:, c]], f32(0)))
                w[:, c] = np.where(valid[:, c], w[:, c] * vis, w[:, c])
        E = G.convolve(probes["sh"][index], G.lobe(n)[:, None, :])
        out[ok] = G.blend(valid, w, E)
    return out


def as_words(records):
    """DEPTH records as uint32 (n, 128): every word as it is."""
    return np.ascontiguousarray(records).view(np.uint32).reshape(-1, 2 * TEXELS)


def assert_depth_equal(got, want, what):
    g, w = as_words(got), as_words(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.nonzero((g != w).any(axis=1))[0]
    if len(bad):
        i = int(bad[0])
        words = np.nonzero(g[i] != w[i])[0].tolist()
        raise AssertionError(f"{what}: {len(bad)} of {len(g)} records differ (probes {bad[:8].tolist()}); the first is probe {i}, "
                             f"{len(words)} words from {words[:8]}: got {[hex(v) for v in g[i][words[:4]]]} want {[hex(v) for v in w[i][words[:4]]]}")
