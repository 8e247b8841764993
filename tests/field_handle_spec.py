"""The definition of rm_field_trace (include/raymarcher_amd.h, "Lattice handles") in NumPy float32, built on field_spec's functions and
sharing no code with the library: rm_sdf_trace_blocks' state machine in which max_steps counts SAMPLES only — a skip of an unlisted
block is free — and the occlusion mode's penumbra tracker.  rm_field_sample is field_spec.sample as it is.  Vectorised over the rays
with masks: one pass of the loop below is one iteration of every live ray's state machine."""
import numpy as np

import field_spec as F
import sdf_blocks_spec as B

f32 = np.float32
CLOSEST, NO_NORMAL, OCCLUSION = 0, 1, 2
PENUMBRA_K = f32(8.0)
sample = F.sample


def trace(dense, origin, step, rays, iso, max_steps, ids=None, block_list=None, mode=CLOSEST, stats=None):
    """rm_field_trace on a dense handle (block_list None) or a block handle → HIT records (n).  rays: (n, 8) float32 rows of RmRay.
    stats: a dict that receives per ray `samples`, `skips`, `iterations` (the passes of the loop, the one that ended the ray included)
    and `exhausted` (the ray ended because its samples were used up: only such a ray depends on the budget), and `never_ends`: the
    ray reached a state that repeats — a sample that was not forced and left t with the bits it had, or a NaN t, which stays one; b
    is then recomputed from the same t for ever, in this march and in rm_sdf_trace_blocks' alike, so no budget ends such a ray."""
    assert mode in (CLOSEST, NO_NORMAL, OCCLUSION)
    occlusion = mode == OCCLUSION
    dense = np.asarray(dense, f32)
    origin, step, iso = np.asarray(origin, f32), np.asarray(step, f32), f32(iso)
    rays = np.asarray(rays, f32)
    ro, tmax, rd = rays[:, 0:3], rays[:, 3], rays[:, 4:7]
    n = len(rays)
    nz, ny, nx = dense.shape
    Ni = np.array([nx - 1, ny - 1, nz - 1], np.int64)
    N = Ni.astype(f32)
    listed = F._listed_map(dense, block_list)
    m = np.array(B.blocks_of(dense), np.int64) if listed is not None else None
    out = np.zeros(n, F.HIT)
    samples, skips, iterations = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    with np.errstate(all="ignore"):
        uo, ud = (ro - origin) / step, rd / step
        valid = (np.isfinite(ro).all(axis=1) & np.isfinite(rd).all(axis=1) & (tmax >= f32(0)) & np.isfinite(uo).all(axis=1)
                 & np.isfinite(ud).all(axis=1) & (ud != f32(0)).any(axis=1))
        out["objectId"] = np.where(valid, F.MISS, F.INVALID)
        res = np.ones(n, f32)
        near, far = np.full(n, -np.inf, f32), np.full(n, np.inf, f32)
        alive = valid.copy()
        for a in range(3):
            moving = ud[:, a] != f32(0)
            t1, t2 = (f32(0) - uo[:, a]) / ud[:, a], (N[a] - uo[:, a]) / ud[:, a]
            near = np.where(moving, F.fmax(near, F.fmin(t1, t2)), near)
            far = np.where(moving, F.fmin(far, F.fmax(t1, t2)), far)
            alive &= moving | ~((uo[:, a] < f32(0)) | (uo[:, a] > N[a]))
        t = F.fmax(near, f32(0)).astype(f32)
        t_end = F.fmin(tmax, far)
        alive &= t <= t_end
        forced = np.zeros(n, bool)
        b = np.zeros((n, 3), np.int64)
        hit_rows, exhausted, never_ends = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool)
        while True:
            w = np.nonzero(alive)[0]
            if len(w) == 0:
                break
            iterations[w] += 1
            alive[w[t[w] > t_end[w]]] = False
            w = np.nonzero(alive)[0]
            if len(w) == 0:
                break
            u = uo[w] + ud[w] * t[w][:, None]
            if listed is None:
                u = F.clamp(u, f32(0), N)
                cell = np.minimum(np.floor(u).astype(np.int64), Ni - 1)
                has = np.ones(len(w), bool)
            else:
                fw = forced[w][:, None]
                bw = b[w]
                u = np.where(fw, F.clamp(u, (8 * bw).astype(f32), (8 * bw + 8).astype(f32)), F.clamp(u, f32(0), N))
                bw = np.where(fw, bw, np.minimum(np.floor(u).astype(np.int64) >> 3, m - 1))
                b[w] = bw
                has = listed[bw[:, 2], bw[:, 1], bw[:, 0]]
                cell = np.minimum(np.floor(u).astype(np.int64), 8 * bw + 7)
                s = np.nonzero(~has)[0]
                if len(s):  # unlisted: the skip of rm_sdf_trace_blocks' step 3, which costs nothing here
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
                    t[ws] = F.fmax(best, t[ws])
                    forced[ws] = True
            k = np.nonzero(has)[0]
            spent = samples[w[k]] >= int(max_steps)  # miss if samples == maxSteps
            alive[w[k][spent]] = False
            exhausted[w[k][spent]] = True
            k = k[~spent]
            wk, uk, ck = w[k], u[k], cell[k]
            samples[wk] += 1
            f = uk - ck.astype(f32)
            v = F._corners(dense, ck)
            value = F.cell_value(v, f)
            free = ~forced[wk]
            forced[wk] = False
            hit = value < iso
            go = wk[~hit]
            moved = (t[wk] + value)[~hit]
            never_ends[go] |= free[~hit] & ((moved.view(np.uint32) == t[go].view(np.uint32)) | (np.isnan(moved) & np.isnan(t[go])))
            if occlusion:  # before t advances; a NaN q never enters
                q = (PENUMBRA_K * value[~hit]) / t[go]
                res[go] = np.where(q < res[go], q, res[go])
            t[go] = moved
            wh, fh, ch, vh = wk[hit], f[hit], ck[hit], v[:, hit]
            alive[wh] = False
            hit_rows[wh] = True
            out["objectId"][wh] = F._corner_ids(ids, ch, fh, 0)
            if not occlusion:
                out["t"][wh] = t[wh]
                if mode == CLOSEST and len(wh):
                    g = F.cell_gradient(vh, fh, step)
                    length = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
                    unit = np.isfinite(length) & (length != f32(0))
                    out["normal"][wh] = np.where(unit[:, None], g / length[:, None], f32(0))
                    out["position"][wh] = ro[wh] + rd[wh] * t[wh][:, None]
        if occlusion:
            out["t"] = np.where(valid, res, f32(0))
        else:
            out["t"] = np.where(valid & ~hit_rows, tmax, out["t"])
    if stats is not None:
        stats["samples"], stats["skips"], stats["iterations"], stats["exhausted"] = samples, skips, iterations, exhausted
        stats["never_ends"] = never_ends
    return out
