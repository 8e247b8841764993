"""The definition of rm_light_probes (include/raymarcher_amd.h) in NumPy float32, sharing no code with the library: which probes and
rows are valid, the rays as (n·K, 8) rows of RmRay, their colours through shade_helpers.spec_shade — the specification of
rm_shade_rays, which the definition names —, their hit flags through trace_helpers.spec_trace — the specification of rm_trace_rays in
the mode the definition names —, the leaves and the pairwise tree.  Every array below is float32 and every operation on them one
rounded binary32 operation.  Also rm_sphere_directions' table as the header states it, in NumPy float64."""
import numpy as np

f32 = np.float32
PROBE = np.dtype([("sh", "<f4", (9, 4)), ("hits", "<i4"), ("reserved", "<i4", 3)])
assert PROBE.itemsize == 160
INVALID = -2  # RM_RAY_INVALID
MAX_DIRS, MAX_TABLE = 1024, 4096
GOLDEN, PLASTIC = 0.6180339887498949, 0.7548776662466927


# ---------------------------------------------------------------- rm_sphere_directions, in float64
def sh9(d):
    """The nine real spherical harmonics of bands 0 to 2 at unit vectors d (..., 3), float64, in the header's order."""
    d = np.asarray(d, np.float64)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    pi = np.pi
    c0, c1, c2 = np.sqrt(1 / (4 * pi)), np.sqrt(3 / (4 * pi)), np.sqrt(15 / (4 * pi))
    c20, c22 = np.sqrt(5 / (16 * pi)), np.sqrt(15 / (16 * pi))
    return np.stack([c0 + 0 * x, c1 * y, c1 * z, c1 * x, c2 * (x * y), c2 * (y * z), c20 * (3 * (z * z) - 1), c2 * (x * z), c22 * (x * x - y * y)],
                    axis=-1)


def sphere_table64(K, sets):
    """(dir (sets, K, 3), basis (sets, K, 9)) of rm_sphere_directions before the one rounding, float64."""
    k = np.arange(K, dtype=np.float64)[None, :]
    s = np.arange(sets, dtype=np.float64)[:, None]
    z = 1 - (2 * k + 1) / K + 0 * s
    r = np.sqrt(1 - z * z)
    turn = k * GOLDEN + s * PLASTIC
    phi = 2 * np.pi * (turn - np.floor(turn))
    d = np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=-1)
    return d, (4 * np.pi / K) * sh9(d)


# ---------------------------------------------------------------- the definition
def valid_positions(positions):
    with np.errstate(all="ignore"):
        return np.isfinite(np.asarray(positions, f32)[:, 0:3]).all(axis=1)


def valid_rows(table):
    """rm_shade_rays' rule for a direction: every component finite, not all three zero."""
    d = np.asarray(table, f32)[:, 0:3]
    with np.errstate(all="ignore"):
        return np.isfinite(d).all(axis=1) & (d != f32(0)).any(axis=1)


def rows_of(n, K, sets, first=0):
    """The table row of every (probe, k) → int (n, K).  first: the index of probe 0 in the call, which selects the sets."""
    return ((first + np.arange(n)) % int(sets))[:, None] * int(K) + np.arange(int(K))[None, :]


def rays(positions, table, K, sets, far, first=0):
    """The rays of the call as (n·K, 8) float32 rows of RmRay, probe-major: origin = the position, dir = the row's as given."""
    p = np.asarray(positions, f32)[:, 0:3]
    n = len(p)
    e = np.asarray(table, f32).reshape(-1, 16)[rows_of(n, K, sets, first)]  # (n, K, 16)
    out = np.zeros((n, int(K), 8), f32)
    out[:, :, 0:3], out[:, :, 3], out[:, :, 4:7] = p[:, None, :], f32(far), e[:, :, 0:3]
    return out.reshape(n * int(K), 8)


def tree(leaves):
    """The pairwise tree over axis 1 of (n, K, w), level by level, s[m] = s[2m] + s[2m + 1]."""
    s = np.asarray(leaves, f32)
    assert s.shape[1] & (s.shape[1] - 1) == 0
    with np.errstate(all="ignore"):
        while s.shape[1] > 1:
            s = s[:, 0::2] + s[:, 1::2]
    assert s.dtype == f32
    return s[:, 0]


def fold(positions, table, K, sets, colours, hit, first=0):
    """The records of the call from its rays' colours (n·K, 3 or 4) and hit flags (n·K): leaves, tree, counts → PROBE (n)."""
    n, K = len(positions), int(K)
    table = np.asarray(table, f32).reshape(-1, 16)
    which = rows_of(n, K, sets, first)
    ok_row = valid_rows(table)[which]                                        # (n, K)
    c = np.where(ok_row[:, :, None], np.asarray(colours, f32).reshape(n, K, -1)[:, :, 0:3], f32(0)).astype(f32)
    hit = ok_row & np.asarray(hit, bool).reshape(n, K)
    ch = np.concatenate([c, np.where(hit, f32(1), f32(0)).astype(f32)[:, :, None]], axis=2)  # (n, K, 4)
    basis = table[which][:, :, 4:13]                                         # (n, K, 9)
    with np.errstate(all="ignore"):
        leaves = (basis[:, :, :, None] * ch[:, :, None, :]).reshape(n, K, 36)
    assert leaves.dtype == f32
    sums = tree(leaves)
    out = np.zeros(n, PROBE)
    ok = valid_positions(positions)
    out["sh"][ok] = sums[ok].reshape(-1, 9, 4)
    out["hits"] = np.where(ok, hit.sum(axis=1), INVALID)
    return out


def probes(scene, s, res, positions, table, K, sets, far, shade=None, trace=None, first=0):
    """rm_light_probes by the definition → PROBE records (n).  scene, s, res: the tests' case (shade_helpers.case).  shade: None —
    the colours come from shade_helpers.spec_shade — or a function rays (r, 8) → colours (r, 4); trace: None — the hit flags come
    from trace_helpers.spec_trace — or a function rays (r, 8) → object ids (r): the composition through the shipped entries."""
    import shade_helpers as S
    import trace_helpers as T
    rows = rays(positions, table, K, sets, far, first)
    colours = shade(rows) if shade is not None else S.spec_shade(scene, s, rows, far, res)[0]
    ids = trace(rows) if trace is not None else T.ids_of(T.spec_trace(scene[1], scene[2], scene[5], s, rows, "no_normal"))
    return fold(positions, table, K, sets, colours, np.asarray(ids) >= 0, first)


def as_words(records):
    """PROBE records as uint32 (n, 40): every word as it is."""
    return np.ascontiguousarray(records).view(np.uint32).reshape(-1, 40)


def assert_records_equal(got, want, what):
    g, w = as_words(got), as_words(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.nonzero((g != w).any(axis=1))[0]
    if len(bad):
        i = int(bad[0])
        words = np.nonzero(g[i] != w[i])[0].tolist()
        raise AssertionError(f"{what}: {len(bad)} of {len(g)} records differ; the first is probe {i}, words {words[:8]}: got "
                             f"{g[i][words[:4]].tolist()} want {w[i][words[:4]].tolist()}; hits {g[i][36].view(np.int32)} / {w[i][36].view(np.int32)}")
