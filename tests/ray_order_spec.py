"""The NumPy specification of rm_rays_order: which rays are valid for ordering, their five coordinates, the bounds, the keys and
the order, in binary32 as include/raymarcher_amd.h defines them.  Every operation is an elementwise float32 NumPy operation (add,
subtract, multiply, divide: correctly rounded, never fused); the order is np.argsort(keys, kind="stable")."""
import numpy as np

f32 = np.float32
MAX_ORIGIN_BITS, MAX_DIR_BITS = 10, 11
BIT_PAIRS = ((0, 0), (0, 11), (10, 0), (7, 8), (10, 11))


def _rays(rays):
    rays = np.ascontiguousarray(rays, dtype=f32)
    assert rays.ndim == 2 and rays.shape[1] == 8
    return rays


def valid(rays):
    """Every component of origin and dir finite, dir not all zeros; tMax (word 3) and `reserved` (word 7) are not read."""
    rays = _rays(rays)
    o, d = rays[:, 0:3], rays[:, 4:7]
    return np.isfinite(o).all(1) & np.isfinite(d).all(1) & (d != 0).any(1)


def sgn(x):
    """−1 where the sign bit is set (−0 too), +1 otherwise."""
    return np.where(np.signbit(x), f32(-1), f32(1)).astype(f32)


def coordinates(rays):
    """float32 (n, 5): ox, oy, oz, u, v.  Rows of rays that are not valid hold whatever the arithmetic gives; nobody reads them."""
    rays = _rays(rays)
    with np.errstate(all="ignore"):
        dx, dy, dz = rays[:, 4], rays[:, 5], rays[:, 6]
        s = (np.abs(dx) + np.abs(dy)) + np.abs(dz)
        px, py = dx / s, dy / s
        one = f32(1)
        u = np.where(dz < 0, (one - np.abs(py)) * sgn(px), px)
        v = np.where(dz < 0, (one - np.abs(px)) * sgn(py), py)
    return np.stack([rays[:, 0], rays[:, 1], rays[:, 2], u, v], axis=1).astype(f32)


def bounds(rays):
    """(lo, hi), float32 (5,) each, over the valid rays; (+inf, −inf) where there is none."""
    c = coordinates(rays)[valid(rays)]
    if len(c) == 0:
        return np.full(5, np.inf, f32), np.full(5, -np.inf, f32)
    return c.min(0), c.max(0)


def quantise(x, lo, hi, b):
    """uint32 of x's shape."""
    x = np.asarray(x, f32)
    if not hi > lo:
        return np.zeros(x.shape, np.uint32)
    with np.errstate(all="ignore"):
        t = (x - f32(lo)) / (f32(hi) - f32(lo))
        scaled = t * f32(1 << b)
    inside = (t > 0) & ~(t >= 1)
    q = np.zeros(x.shape, np.uint32)
    q[inside] = scaled[inside].astype(np.uint32)  # a truncation; t < 1 makes t·2^b < 2^b
    q[t >= 1] = (1 << b) - 1
    return q


def _spread(q, stride, nbits):
    r = np.zeros(q.shape, np.uint64)
    q = q.astype(np.uint64)
    for i in range(nbits):
        r |= ((q >> np.uint64(i)) & np.uint64(1)) << np.uint64(stride * i)
    return r


def keys(rays, origin_bits, dir_bits, lo_hi=None):
    """uint64 (n,), in input order.  lo_hi: bounds to use in place of the rays' own (for the test of the zeros' signs)."""
    assert 0 <= origin_bits <= MAX_ORIGIN_BITS and 0 <= dir_bits <= MAX_DIR_BITS
    rays = _rays(rays)
    lo, hi = bounds(rays) if lo_hi is None else lo_hi
    c = coordinates(rays)
    q = [quantise(c[:, k], lo[k], hi[k], origin_bits if k < 3 else dir_bits) for k in range(5)]
    o = _spread(q[0], 3, MAX_ORIGIN_BITS) | (_spread(q[1], 3, MAX_ORIGIN_BITS) << np.uint64(1)) | (_spread(q[2], 3, MAX_ORIGIN_BITS) << np.uint64(2))
    d = _spread(q[3], 2, MAX_DIR_BITS) | (_spread(q[4], 2, MAX_DIR_BITS) << np.uint64(1))
    k = (o << np.uint64(2 * dir_bits)) | d
    k[~valid(rays)] = np.uint64(1) << np.uint64(3 * origin_bits + 2 * dir_bits)
    return k


def order(rays, origin_bits, dir_bits):
    """int32 (n,): order[k] = the input index of the ray at sorted position k."""
    return np.argsort(keys(rays, origin_bits, dir_bits), kind="stable").astype(np.int32)


def restore(rows, order_):
    """rm_rays_restore on the host: out[order[k]] = rows[k]; entries outside [0, n) are skipped → (out, written mask)."""
    rows, order_ = np.asarray(rows), np.asarray(order_)
    out, written = np.zeros_like(rows), np.zeros(len(rows), bool)
    ok = (order_ >= 0) & (order_ < len(rows))
    out[order_[ok]] = rows[ok]
    written[order_[ok]] = True
    return out, written


def median_wave_box(order_, pixels, wave=64):
    """The median, over the runs of `wave` consecutive rays in `order_`, of the area of the pixel bounding box of the run;
    pixels: int (n, 2), the pixel each INPUT ray belongs to."""
    p = np.asarray(pixels)[np.asarray(order_)]
    areas = []
    for a in range(0, len(p), wave):
        run = p[a:a + wave]
        w = run.max(0) - run.min(0) + 1
        areas.append(int(w[0]) * int(w[1]))
    return float(np.median(areas))
