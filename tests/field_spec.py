"""The definitions of rm_sdf_sample, rm_sdf_sample_blocks, rm_sdf_trace and rm_sdf_trace_blocks (include/raymarcher_amd.h) in NumPy
float32, sharing no code with the library.  Everything starts from a DENSE lattice (nz, ny, nx): a block list only says which blocks
of it a query may read — a listed block's slot holds the dense lattice's values (sdf_blocks_spec.pack_blocks), so reading the dense
array at the global cell IS reading the slot.  Vectorised over points and rays with masks; every operation is one float32 operation."""
import numpy as np

import sdf_blocks_spec as B

f32 = np.float32
INVALID, OUTSIDE, UNLISTED, MISS = -2, -5, -6, -1
SAMPLE = np.dtype([("gradient", "<f4", 3), ("value", "<f4"), ("cell", "<i4", 3), ("objectId", "<i4")])
HIT = np.dtype([("normal", "<f4", 3), ("t", "<f4"), ("position", "<f4", 3), ("objectId", "<i4")])
assert SAMPLE.itemsize == 32 and HIT.itemsize == 32


def fmin(a, b):
    return np.where(a < b, a, b)


def fmax(a, b):
    return np.where(a > b, a, b)


def clamp(x, lo, hi):
    """min(max(x, lo), hi) with max(x, lo) = x > lo ? x : lo: a NaN clamps to lo."""
    return fmin(fmax(x, lo), hi)


def lerp(a, b, w):
    return a + w * (b - a)


def _corners(dense, cell):
    """The eight values of the cells (n, 3) as (8, n), corner c = cx + 2·cy + 4·cz."""
    i, j, k = cell[:, 0], cell[:, 1], cell[:, 2]
    return np.stack([dense[k + ((c >> 2) & 1), j + ((c >> 1) & 1), i + (c & 1)] for c in range(8)])


def cell_value(v, f):
    fx, fy, fz = f[:, 0], f[:, 1], f[:, 2]
    x0, x1, x2, x3 = lerp(v[0], v[1], fx), lerp(v[2], v[3], fx), lerp(v[4], v[5], fx), lerp(v[6], v[7], fx)
    return lerp(lerp(x0, x1, fy), lerp(x2, x3, fy), fz)


def cell_gradient(v, f, step):
    fx, fy, fz = f[:, 0], f[:, 1], f[:, 2]
    gx = lerp(lerp(v[1] - v[0], v[3] - v[2], fy), lerp(v[5] - v[4], v[7] - v[6], fy), fz) / step[0]
    gy = lerp(lerp(v[2] - v[0], v[3] - v[1], fx), lerp(v[6] - v[4], v[7] - v[5], fx), fz) / step[1]
    gz = lerp(lerp(v[4] - v[0], v[5] - v[1], fx), lerp(v[6] - v[2], v[7] - v[3], fx), fy) / step[2]
    return np.stack([gx, gy, gz], axis=1)


def _corner_ids(ids, cell, f, without):
    if ids is None:
        return np.full(len(cell), without, np.int32)
    up = (f >= f32(0.5)).astype(np.int64)
    return ids[cell[:, 2] + up[:, 2], cell[:, 1] + up[:, 1], cell[:, 0] + up[:, 0]].astype(np.int32)


def _listed_map(dense, block_list):
    """bool (mz, my, mx): which blocks a query may read; None for the dense entries."""
    if block_list is None:
        return None
    return B.first_positions(np.asarray(block_list, np.int32).reshape(-1, 4), B.blocks_of(dense)) >= 0


def sample(dense, origin, step, points, ids=None, block_list=None):
    """rm_sdf_sample (block_list None) / rm_sdf_sample_blocks → SAMPLE records (n).  points: (n, 3) or (n, 4) float32."""
    dense = np.asarray(dense, f32)
    origin, step = np.asarray(origin, f32), np.asarray(step, f32)
    p = np.asarray(points, f32)[:, :3]
    nz, ny, nx = dense.shape
    N = np.array([nx - 1, ny - 1, nz - 1], np.int64)
    listed = _listed_map(dense, block_list)
    out = np.zeros(len(p), SAMPLE)
    with np.errstate(all="ignore"):
        valid = np.isfinite(p).all(axis=1)
        u = (p - origin) / step
        inside = valid & ((u >= f32(0)) & (u <= N.astype(f32))).all(axis=1)
        out["objectId"] = np.where(valid, OUTSIDE, INVALID)
        w = np.nonzero(inside)[0]
        uw = u[w]
        cell = np.minimum(np.floor(uw).astype(np.int64), N - 1)
        out["cell"][w] = cell
        if listed is not None:
            m = np.array(B.blocks_of(dense), np.int64)
            b = np.minimum(cell >> 3, m - 1)
            has = listed[b[:, 2], b[:, 1], b[:, 0]]
            out["objectId"][w[~has]] = UNLISTED
            w, uw, cell = w[has], uw[has], cell[has]
        f = uw - cell.astype(f32)
        v = _corners(dense, cell)
        out["value"][w] = cell_value(v, f)
        out["gradient"][w] = cell_gradient(v, f, step)
        out["objectId"][w] = _corner_ids(ids, cell, f, -1)
    return out


def trace(dense, origin, step, rays, iso, max_steps, ids=None, block_list=None, normals=True, stats=None):
    """rm_sdf_trace (block_list None) / rm_sdf_trace_blocks → HIT records (n).  rays: (n, 8) float32 rows of RmRay.  stats: a dict
    that receives `iterations` and `skips` per ray."""
    dense = np.asarray(dense, f32)
    origin, step, iso = np.asarray(origin, f32), np.asarray(step, f32), f32(iso)
    rays = np.asarray(rays, f32)
    ro, tmax, rd = rays[:, 0:3], rays[:, 3], rays[:, 4:7]
    n = len(rays)
    nz, ny, nx = dense.shape
    Ni = np.array([nx - 1, ny - 1, nz - 1], np.int64)
    N = Ni.astype(f32)
    listed = _listed_map(dense, block_list)
    m = np.array(B.blocks_of(dense), np.int64) if listed is not None else None
    out = np.zeros(n, HIT)
    iterations, skips = np.zeros(n, np.int64), np.zeros(n, np.int64)
    with np.errstate(all="ignore"):
        uo, ud = (ro - origin) / step, rd / step
        valid = (np.isfinite(ro).all(axis=1) & np.isfinite(rd).all(axis=1) & (tmax >= f32(0)) & np.isfinite(uo).all(axis=1)
                 & np.isfinite(ud).all(axis=1) & (ud != f32(0)).any(axis=1))
        out["objectId"] = np.where(valid, MISS, INVALID)
        out["t"] = np.where(valid, tmax, f32(0))
        # the box
        near, far = np.full(n, -np.inf, f32), np.full(n, np.inf, f32)
        alive = valid.copy()
        for a in range(3):
            moving = ud[:, a] != f32(0)
            t1, t2 = (f32(0) - uo[:, a]) / ud[:, a], (N[a] - uo[:, a]) / ud[:, a]
            near = np.where(moving, fmax(near, fmin(t1, t2)), near)
            far = np.where(moving, fmin(far, fmax(t1, t2)), far)
            alive &= moving | ~((uo[:, a] < f32(0)) | (uo[:, a] > N[a]))
        t = fmax(near, f32(0)).astype(f32)
        t_end = fmin(tmax, far)
        alive &= t <= t_end
        forced = np.zeros(n, bool)
        b = np.zeros((n, 3), np.int64)
        for _ in range(int(max_steps)):
            alive &= ~(t > t_end)
            w = np.nonzero(alive)[0]
            if len(w) == 0:
                break
            iterations[w] += 1
            u = uo[w] + ud[w] * t[w][:, None]
            if listed is None:
                u = clamp(u, f32(0), N)
                cell = np.minimum(np.floor(u).astype(np.int64), Ni - 1)
                has = np.ones(len(w), bool)
            else:
                fw = forced[w][:, None]
                bw = b[w]
                u = np.where(fw, clamp(u, (8 * bw).astype(f32), (8 * bw + 8).astype(f32)), clamp(u, f32(0), N))
                bw = np.where(fw, bw, np.minimum(np.floor(u).astype(np.int64) >> 3, m - 1))
                b[w] = bw
                has = listed[bw[:, 2], bw[:, 1], bw[:, 0]]
                cell = np.minimum(np.floor(u).astype(np.int64), 8 * bw + 7)
                # unlisted: skip to the block's exit
                s = np.nonzero(~has)[0]
                if len(s):
                    ws = w[s]
                    skips[ws] += 1
                    best = np.full(len(s), np.inf, f32)
                    axis = np.full(len(s), -1, np.int64)
                    for a in range(3):
                        moving = ud[ws, a] != f32(0)
                        face = (8 * (bw[s, a] + (ud[ws, a] > f32(0)))).astype(f32)
                        ta = (face - uo[ws, a]) / ud[ws, a]
                        take = moving & ((axis < 0) | (ta < best))
                        best, axis = np.where(take, ta, best), np.where(take, a, axis)
                    rows = np.arange(len(s))
                    sign = np.where(ud[ws, axis] > f32(0), 1, -1)
                    nb = bw[s].copy()
                    nb[rows, axis] += sign
                    b[ws] = nb
                    left = (nb[rows, axis] < 0) | (nb[rows, axis] >= m[axis])
                    alive[ws[left]] = False
                    t[ws] = fmax(best, t[ws])
                    forced[ws] = True
            k = np.nonzero(has)[0]
            wk, uk, ck = w[k], u[k], cell[k]
            f = uk - ck.astype(f32)
            v = _corners(dense, ck)
            value = cell_value(v, f)
            forced[wk] = False
            hit = value < iso
            t[wk[~hit]] = (t[wk] + value)[~hit]
            wh, fh, ch, vh = wk[hit], f[hit], ck[hit], v[:, hit]
            alive[wh] = False
            out["t"][wh] = t[wh]
            out["objectId"][wh] = _corner_ids(ids, ch, fh, 0)
            if normals and len(wh):
                g = cell_gradient(vh, fh, step)
                length = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
                unit = np.isfinite(length) & (length != f32(0))
                out["normal"][wh] = np.where(unit[:, None], g / length[:, None], f32(0))
                out["position"][wh] = ro[wh] + rd[wh] * t[wh][:, None]
    if stats is not None:
        stats["iterations"], stats["skips"] = iterations, skips
    return out


def as_words(records):
    """SAMPLE or HIT records as uint32 (n, 8), for bit comparisons.  Every word as it is, but for one thing IEEE 754 leaves to the
    hardware: which NaN an operation returns (x86 gives inf − inf the sign bit, the GPU does not, and payloads propagate by other
    rules).  A NaN in a float field is written as 0x7FC00000; that a word IS a NaN is compared like any other bit."""
    records = np.ascontiguousarray(records)
    assert records.dtype in (SAMPLE, HIT), "as_words() of something that is no record array"
    words = records.view(np.uint32).reshape(-1, 8).copy()
    floats = records.view(np.float32).reshape(-1, 8)
    columns = 4 if records.dtype == SAMPLE else 7  # behind them: cell and objectId
    words[:, :columns][np.isnan(floats[:, :columns])] = 0x7FC00000
    return words
