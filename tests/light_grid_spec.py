"""The definition of rm_light_grid_irradiance (include/raymarcher_amd.h, steps 1 to 9) in NumPy float32, written from the header's
text and sharing no code with the library: valid points, the cell and the trilinear weights, which corner probes take part, the
facing weight, the cosine-lobe weights of the normal, a probe's convolution and the three-level tree over the corners.  Every array
below is float32 and every operation on them one rounded binary32 operation; the five constants are float64 arithmetic rounded
once.  The pieces are functions of their own so that the tests can put them together by hand."""
import numpy as np

f32 = np.float32
PROBE = np.dtype([("sh", "<f4", (9, 4)), ("hits", "<i4"), ("reserved", "<i4", 3)])        # RmLightProbe
GRIDLIGHT = np.dtype([("e", "<f4", 4), ("weight", "<f4"), ("probes", "<i4"), ("reserved", "<i4", 2)])  # RmGridLight
assert PROBE.itemsize == 160 and GRIDLIGHT.itemsize == 32
INVALID = -2  # RM_RAY_INVALID
FACING = 1    # RM_LIGHT_GRID_FACING
MAX_DIM, MAX_PROBES = 1024, 1 << 24
K0 = f32(np.pi * np.sqrt(1 / (4 * np.pi)))
K1 = f32((2 * np.pi / 3) * np.sqrt(3 / (4 * np.pi)))
K2 = f32((np.pi / 4) * np.sqrt(15 / (4 * np.pi)))
K6 = f32((np.pi / 4) * np.sqrt(5 / (16 * np.pi)))
K8 = f32((np.pi / 4) * np.sqrt(15 / (16 * np.pi)))


def _vec(v):
    return np.asarray(v, f32).reshape(3)


def positions(origin, step, dims):
    """The probes' world positions, (nx·ny·nz, 3) float32, x fastest: origin_a + (float)index_a · step_a, unfused."""
    o, s = _vec(origin), _vec(step)
    nx, ny, nz = (int(d) for d in dims)
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    at = np.stack([i.ravel(), j.ravel(), k.ravel()], axis=1).astype(f32)
    out = o[None, :] + at * s[None, :]
    assert out.dtype == f32
    return out


def valid_points(points, normals):
    """Step 1."""
    p, n = np.asarray(points, f32)[:, 0:3], np.asarray(normals, f32)[:, 0:3]
    with np.errstate(all="ignore"):
        return np.isfinite(p).all(axis=1) & np.isfinite(n).all(axis=1) & (n != f32(0)).any(axis=1)


def cells(p, origin, step, dims):
    """Step 2 → (cell int (m, 3), f float32 (m, 3))."""
    o, s, d = _vec(origin), _vec(step), np.asarray(dims, np.int64).reshape(3)
    with np.errstate(all="ignore"):
        u = (np.asarray(p, f32) - o[None, :]) / s[None, :]
        top = (d - 1).astype(f32)[None, :]
        u = np.where(u > f32(0), u, f32(0)).astype(f32)
        u = np.where(u > top, top, u).astype(f32)
        cell = np.minimum(np.floor(u).astype(np.int64), (d - 2)[None, :])
        f = u - cell.astype(f32)
    assert f.dtype == f32
    return cell, f


def lobe(normals):
    """Step 7 → (m, 9) float32."""
    n = np.asarray(normals, f32)
    x, y, z = n[:, 0], n[:, 1], n[:, 2]
    with np.errstate(all="ignore"):
        k = np.stack([np.full_like(x, K0), K1 * y, K1 * z, K1 * x, K2 * (x * y), K2 * (y * z), K6 * (f32(3) * (z * z) - f32(1)), K2 * (x * z),
                      K8 * (x * x - y * y)], axis=1)
    assert k.dtype == f32
    return k


def convolve(sh, k):
    """Step 8's E: sh (..., 9, 4) and k (..., 9) float32 → (..., 4): k0·sh0, then + k_j·sh_j for j = 1 … 8 in order."""
    sh, k = np.asarray(sh, f32), np.asarray(k, f32)
    with np.errstate(all="ignore"):
        E = k[..., 0, None] * sh[..., 0, :]
        for j in range(1, 9):
            E = E + k[..., j, None] * sh[..., j, :]
    assert E.dtype == f32
    return E


def tree8(v):
    """((v0 + v1) + (v2 + v3)) + ((v4 + v5) + (v6 + v7)) over axis 1 of (m, 8, ...)."""
    with np.errstate(all="ignore"):
        s = ((v[:, 0] + v[:, 1]) + (v[:, 2] + v[:, 3])) + ((v[:, 4] + v[:, 5]) + (v[:, 6] + v[:, 7]))
    assert s.dtype == f32
    return s


def corners(hits, dims, origin, step, p, n, facing):
    """Steps 2 to 5 for valid points p, n (m, 3) → (index int (m, 8), valid bool (m, 8), w float32 (m, 8))."""
    o, s, d = _vec(origin), _vec(step), np.asarray(dims, np.int64).reshape(3)
    p, n = np.asarray(p, f32), np.asarray(n, f32)
    cell, f = cells(p, o, s, d)
    m = len(p)
    index, valid, w = np.zeros((m, 8), np.int64), np.zeros((m, 8), bool), np.zeros((m, 8), f32)
    with np.errstate(all="ignore"):
        for c in range(8):
            bit = np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1])
            at = cell + bit[None, :]
            index[:, c] = at[:, 0] + d[0] * (at[:, 1] + d[1] * at[:, 2])
            valid[:, c] = np.asarray(hits)[index[:, c]] >= 0
            wa = [f[:, a] if bit[a] else f32(1) - f[:, a] for a in range(3)]
            t = (wa[0] * wa[1]) * wa[2]
            if facing:
                q = o[None, :] + at.astype(f32) * s[None, :]
                dd = q - p
                length = np.sqrt((dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2])
                cosv = ((dd[:, 0] * n[:, 0] + dd[:, 1] * n[:, 1]) + dd[:, 2] * n[:, 2]) / length
                b = (cosv + f32(1)) * f32(0.5)
                face = np.where(length == f32(0), f32(1), b * b + f32(0.2)).astype(f32)
                t = t * face
            assert t.dtype == f32
            w[:, c] = np.where(valid[:, c], t, f32(0))
    return index, valid, w


def blend(valid, w, E):
    """Steps 6, 8 and 9 from the corners' validity (m, 8), weights (m, 8) and convolutions E (m, 8, 4) → GRIDLIGHT (m).  E of an
    invalid corner is not looked at."""
    m = len(w)
    out = np.zeros(m, GRIDLIGHT)
    with np.errstate(all="ignore"):
        W = tree8(w)
        count = (valid & (w > f32(0))).sum(axis=1)
        leaf = np.where(valid[:, :, None], w[:, :, None] * E, f32(0)).astype(f32)
        e = tree8(leaf) / W[:, None]
    out["weight"], out["probes"] = W, count
    out["e"] = np.where((count > 0)[:, None], e, f32(0))
    return out


def grid_light(probes, dims, origin, step, points, normals, facing):
    """rm_light_grid_irradiance by the definition → GRIDLIGHT records (n).  probes: PROBE records (nx·ny·nz)."""
    probes = np.asarray(probes)
    assert probes.dtype == PROBE and len(probes) == int(np.prod(np.asarray(dims, np.int64)))
    pts, nrm = np.asarray(points, f32)[:, 0:3], np.asarray(normals, f32)[:, 0:3]
    ok = valid_points(pts, nrm)
    out = np.zeros(len(pts), GRIDLIGHT)
    out["probes"][~ok] = INVALID
    if ok.any():
        p, n = pts[ok], nrm[ok]
        index, valid, w = corners(probes["hits"], dims, origin, step, p, n, facing)
        E = convolve(probes["sh"][index], lobe(n)[:, None, :])
        out[ok] = blend(valid, w, E)
    return out


def as_words(records):
    """GRIDLIGHT records as uint32 (n, 8): every word as it is."""
    return np.ascontiguousarray(records).view(np.uint32).reshape(-1, 8)


def assert_records_equal(got, want, what):
    g, w = as_words(got), as_words(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.nonzero((g != w).any(axis=1))[0]
    if len(bad):
        i = int(bad[0])
        words = np.nonzero(g[i] != w[i])[0].tolist()
        raise AssertionError(f"{what}: {len(bad)} of {len(g)} records differ (points {bad[:8].tolist()}); the first is point {i}, words {words}: "
                             f"got {[hex(v) for v in g[i][words]]} want {[hex(v) for v in w[i][words]]}; probes {g[i][5].view(np.int32)} / "
                             f"{w[i][5].view(np.int32)}")
