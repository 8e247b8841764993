"""The definition of rm_sdf_blocks_select_pruned (include/raymarcher_amd.h) in NumPy float32, sharing no code with the library.
Everything is a function of a DENSE float32 lattice of 8·m + 1 points per axis, as sdf_blocks_spec.active_blocks is: the corner
lattice is every eighth point of it, the candidates are read off the corners, and the list is the exhaustive list restricted to
the candidates."""
import numpy as np

import sdf_blocks_spec as B

f32 = np.float32


def bounds(step, l_out, l_in):
    """(bOut, bIn) = (l_out · h, l_in · h), h = 4 · sqrt((sx·sx + sy·sy) + sz·sz): every operation rounded to float32.  A step whose
    square overflows gives h = +inf; 0 · inf is NaN, a bound that no comparison passes."""
    sx, sy, sz = (f32(v) for v in step)
    with np.errstate(over="ignore", invalid="ignore"):
        h = f32(4) * np.sqrt(f32(f32(f32(sx * sx) + f32(sy * sy)) + f32(sz * sz)), dtype=f32)
        return f32(f32(l_out) * h), f32(f32(l_in) * h)


def candidates_of_corners(corners, step, iso, l_out, l_in):
    """corners: float32 (mz + 1, my + 1, mx + 1) → bool (mz, my, mx): False where all eight corners of the block are far outside
    (c − iso > bOut) or all eight are far inside (c − iso < −bIn).  A NaN corner is neither; a value at a bound is not far."""
    c = np.asarray(corners, f32)
    b_out, b_in = bounds(step, l_out, l_in)
    with np.errstate(invalid="ignore"):
        d = c - f32(iso)
        far_out, far_in = d > b_out, d < -b_in

    def all_eight(far):
        out = np.ones(tuple(n - 1 for n in far.shape), bool)
        for cz in (0, 1):
            for cy in (0, 1):
                for cx in (0, 1):
                    out &= far[cz:far.shape[0] - 1 + cz, cy:far.shape[1] - 1 + cy, cx:far.shape[2] - 1 + cx]
        return out
    return ~(all_eight(far_out) | all_eight(far_in))


def candidates(dense, step, iso, l_out, l_in):
    """The candidate flags bool (mz, my, mx) of a dense lattice (nz, ny, nx) of 8·m + 1 points per axis."""
    B.blocks_of(dense)
    return candidates_of_corners(np.asarray(dense)[::8, ::8, ::8], step, iso, l_out, l_in)


def pruned_blocks(dense, step, iso, l_out, l_in, active=None):
    """rm_sdf_blocks_select_pruned → (int32 (n, 4): the candidates that are active by the exact rule, in linear order; the number of
    candidates).  active: sdf_blocks_spec.active_blocks(dense, iso), for a caller that has it already."""
    cand = candidates(dense, step, iso, l_out, l_in)
    act = B.active_blocks(dense, iso) if active is None else np.asarray(active)
    return act[cand[act[:, 2], act[:, 1], act[:, 0]]].reshape(-1, 4), int(cand.sum())
