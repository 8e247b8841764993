"""The definition of rm_field_ambient (include/raymarcher_amd.h) in NumPy float32, sharing no code with the library: the point's
normal, the frame of Duff et al. around it, the rays as (n·K, 8) rows of RmRay, their march through field_handle_spec.trace — the
specification of rm_field_trace, which the definition names —, the leaves and the pairwise tree.  Every array below is float32 and
every operation on them one rounded binary32 operation, in the order the header writes."""
import numpy as np

import field_handle_spec as S
import field_spec as F

f32 = np.float32
AMBIENT = np.dtype([("bent", "<f4", 3), ("visibility", "<f4"), ("normal", "<f4", 3), ("hits", "<i4")])
assert AMBIENT.itemsize == 32
SOFT, HARD = 0, 1
MAX_DIRS, MAX_TABLE = 256, 1024


def point_normals(dense, origin, step, points, normals=None, ids=None, block_list=None):
    """Steps a and b → (n float32 (m, 3), code int32 (m)): code 0 where the point has a normal, else what `hits` stores."""
    p = np.asarray(points, f32)[:, 0:3]
    m = len(p)
    code = np.zeros(m, np.int32)
    n = np.zeros((m, 3), f32)
    with np.errstate(all="ignore"):
        bad_point = ~np.isfinite(p).all(axis=1)
        if normals is not None:
            n = np.array(np.asarray(normals, f32)[:, 0:3], f32)
            code[~np.isfinite(n).all(axis=1) | (n == f32(0)).all(axis=1)] = F.INVALID
        else:
            s = F.sample(dense, origin, step, p, ids, block_list)
            g = s["gradient"]
            length = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
            n = g / length[:, None]
            code[~np.isfinite(length) | (length == f32(0))] = F.INVALID
            refused = np.isin(s["objectId"], (F.OUTSIDE, F.UNLISTED))
            code[refused] = s["objectId"][refused]
        code[bad_point] = F.INVALID
    n = np.where((code != 0)[:, None], f32(0), n).astype(f32)
    return n, code


def frame(n):
    """Step c: (T, B) of the unit vectors n (m, 3), the association as written."""
    nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
    with np.errstate(all="ignore"):
        s = np.copysign(f32(1), nz)
        a = f32(-1) / (s + nz)
        b = (nx * ny) * a
        T = np.stack([f32(1) + (s * (nx * nx)) * a, s * b, (-s) * nx], axis=1)
        B = np.stack([b, s + (ny * ny) * a, -ny], axis=1)
    assert T.dtype == f32 and B.dtype == f32
    return T, B


def rays(points, n, table, num_dirs, num_sets, bias, max_distance, first=0):
    """Step d's rays of the points that have a normal n → (m·K, 8) float32 rows of RmRay, point-major.  first: the index of
    points[0] in the call, which selects the sets."""
    p = np.asarray(points, f32)[:, 0:3]
    m, K = len(p), int(num_dirs)
    table = np.asarray(table, f32).reshape(int(num_sets), K, 4)
    e = table[(first + np.arange(m)) % int(num_sets)]  # (m, K, 4)
    T, B = frame(n)
    with np.errstate(all="ignore"):
        d = (e[:, :, 0:1] * T[:, None, :] + e[:, :, 1:2] * B[:, None, :]) + e[:, :, 2:3] * n[:, None, :]
        o = p + n * f32(bias)
    rows = np.zeros((m, K, 8), f32)
    rows[:, :, 0:3], rows[:, :, 3], rows[:, :, 4:7] = o[:, None, :], f32(max_distance), d
    assert d.dtype == f32 and o.dtype == f32
    return rows.reshape(m * K, 8), e[:, :, 3]


def tree(leaves):
    """Step e: the pairwise tree over axis 1 of (m, K, c), level by level, s[j] = s[2j] + s[2j + 1]."""
    s = np.asarray(leaves, f32)
    assert s.shape[1] & (s.shape[1] - 1) == 0
    with np.errstate(all="ignore"):
        while s.shape[1] > 1:
            s = s[:, 0::2] + s[:, 1::2]
    assert s.dtype == f32
    return s[:, 0]


def fold(hit_records, dirs, weights, n, code, mode):
    """The leaves of HIT records (m·K) of rm_field_trace (occlusion records for SOFT, closest ones for HARD) and their sums →
    AMBIENT records (m).  dirs: the rays' directions (m·K, 3); weights (m, K); n, code: point_normals' of ALL m points — the records
    of a refused point are not looked at."""
    m, K = weights.shape
    obj, t = hit_records["objectId"].reshape(m, K), hit_records["t"].reshape(m, K)
    with np.errstate(all="ignore"):
        seen = np.where(t > f32(0), t, f32(0)) if mode == SOFT else np.ones((m, K), f32)
        v = np.where(obj == F.MISS, seen, f32(0)).astype(f32)
        c = weights * v
        leaves = np.concatenate([c[:, :, None] * dirs.reshape(m, K, 3), c[:, :, None]], axis=2)
    sums = tree(leaves)
    out = np.zeros(m, AMBIENT)
    ok = code == 0
    out["bent"][ok], out["visibility"][ok], out["normal"][ok] = sums[ok, 0:3], sums[ok, 3], n[ok]
    out["hits"] = np.where(ok, ((obj != F.MISS) & (obj != F.INVALID)).sum(axis=1), code)
    return out


def ambient(dense, origin, step, points, normals, table, num_dirs, num_sets, bias, max_distance, iso, max_steps, mode, ids=None,
            block_list=None, march=None):
    """rm_field_ambient on a dense handle (block_list None) or a block handle → AMBIENT records (m).  march: None — the rays go
    through field_handle_spec.trace — or a function rays (r, 8) → HIT records (r) of the mode's march, for the composition through
    a shipped entry."""
    n, code = point_normals(dense, origin, step, points, normals, ids, block_list)
    safe_n = np.where((code != 0)[:, None], np.array([0, 0, 1], f32), n).astype(f32)  # a refused point's rays are discarded
    safe_p = np.where((code != 0)[:, None], f32(0), np.asarray(points, f32)[:, 0:3]).astype(f32)
    rows, weights = rays(safe_p, safe_n, table, num_dirs, num_sets, bias, max_distance)
    trace_mode = S.OCCLUSION if mode == SOFT else S.NO_NORMAL
    hits = (march(rows) if march is not None else S.trace(dense, origin, step, rows, iso, max_steps, ids, block_list, trace_mode))
    return fold(hits, rows[:, 4:7], weights, n, code, mode)


def as_words(records):
    """AMBIENT records as uint32 (m, 8): every word as it is (the contract covers finite tables and lattices, so no NaN)."""
    return np.ascontiguousarray(records).view(np.uint32).reshape(-1, 8)
