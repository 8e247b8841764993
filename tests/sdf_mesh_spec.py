"""The definition of rm_sdf_grid's lattice points and of rm_sdf_mesh (include/raymarcher_amd.h) in NumPy: a vectorised float32
transcription of the header's text that shares no code with the library.  Every array below is float32 and every operation one
float32 operation, so the results are the definition's bits."""
import numpy as np

f32 = np.float32
EDGES = ((0, 1), (2, 3), (4, 5), (6, 7), (0, 2), (1, 3), (4, 6), (5, 7), (0, 4), (1, 5), (2, 6), (3, 7))
EDGE_AXIS = (0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2)
# the four cells around the lattice edge from P along x, y, z, as offsets from P, in the order used when P is inside
QUAD_CELLS = (((0, -1, -1), (0, 0, -1), (0, 0, 0), (0, -1, 0)),
              ((-1, 0, -1), (-1, 0, 0), (0, 0, 0), (0, 0, -1)),
              ((-1, -1, 0), (0, -1, 0), (0, 0, 0), (-1, 0, 0)))


def lattice_axes(origin, step, dims):
    """The coordinates of the lattice per axis: origin + arange(n) · step, one float32 multiply and one float32 add."""
    return [f32(origin[a]) + np.arange(dims[a], dtype=f32) * f32(step[a]) for a in range(3)]


def lattice_points(origin, step, dims):
    """(nx·ny·nz, 3) float32 points in the lattice's linear order (k·ny + j)·nx + i, x fastest."""
    x, y, z = lattice_axes(origin, step, dims)
    zz, yy, xx = np.meshgrid(z, y, x, indexing="ij")
    return np.ascontiguousarray(np.stack([xx, yy, zz], axis=-1).reshape(-1, 3))


def surface_nets(dist, origin, step, iso, ids=None):
    """dist: float32 (nz, ny, nx); ids: int32 of the same shape or None → dict(vertices (n, 4) float32, vertex_object (n) int32,
    quads (m, 4) int32, cells (n, 3) int32: the (i, j, k) of each vertex's cell)."""
    dist = np.asarray(dist)
    assert dist.dtype == f32 and dist.ndim == 3
    nz, ny, nx = dist.shape
    iso = f32(iso)
    empty = dict(vertices=np.zeros((0, 4), f32), vertex_object=np.zeros(0, np.int32), quads=np.zeros((0, 4), np.int32),
                 cells=np.zeros((0, 3), np.int32))
    if min(nx, ny, nz) < 2:
        return empty
    ins = dist < iso  # a NaN is outside

    def corner(a, c):
        cx, cy, cz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        return a[cz:nz - 1 + cz, cy:ny - 1 + cy, cx:nx - 1 + cx]

    v = [corner(dist, c) for c in range(8)]
    m = [corner(ins, c) for c in range(8)]
    count = sum(x.astype(np.int32) for x in m)
    active = (count > 0) & (count < 8)
    shape = active.shape
    acc = [np.zeros(shape, f32) for _ in range(3)]
    n = np.zeros(shape, np.int32)
    with np.errstate(all="ignore"):
        for (a, b), axis in zip(EDGES, EDGE_AXIS):
            cross = m[a] != m[b]
            t = (iso - v[a]) / (v[b] - v[a])
            t = np.where((t >= 0) & (t <= 1), t, f32(0.5)).astype(f32)
            comp = [np.full(shape, f32(a & 1)), np.full(shape, f32((a >> 1) & 1)), np.full(shape, f32((a >> 2) & 1))]
            comp[axis] = t
            for k in range(3):
                acc[k] = np.where(cross, acc[k] + comp[k], acc[k]).astype(f32)
            n += cross
        inv = f32(1.0) / n.astype(f32)
        local = [(acc[k] * inv).astype(f32) for k in range(3)]
    kk, jj, ii = np.nonzero(active)  # C order: the cells' linear order (k·(ny − 1) + j)·(nx − 1) + i
    nv = len(ii)
    verts = np.zeros((nv, 4), f32)
    for k, idx in enumerate((ii, jj, kk)):
        cell = idx.astype(f32) + local[k][active]
        scaled = cell * f32(step[k])
        verts[:, k] = f32(origin[k]) + scaled
    assert verts.dtype == f32
    vobj = np.full(nv, -1, np.int32)
    if ids is not None:
        ids = np.asarray(ids)
        assert ids.dtype == np.int32 and ids.shape == dist.shape
        first = np.full(shape, -1, np.int32)
        for c in range(7, -1, -1):  # the lowest inside corner wins
            first = np.where(m[c], corner(ids, c), first)
        vobj = first[active].astype(np.int32)
    number = np.full(shape, -1, np.int64)
    number[active] = np.arange(nv)

    keys, quads = [], []
    for axis in range(3):
        lo = [1, 1, 1]
        hi = [nx - 2, ny - 2, nz - 2]  # inclusive, interior in the other two axes
        lo[axis] = 0
        if any(hi[a] < lo[a] for a in range(3)):
            continue
        sl = tuple(slice(lo[a], hi[a] + 1) for a in (2, 1, 0))
        sl_next = tuple(slice(lo[a] + (a == axis), hi[a] + 1 + (a == axis)) for a in (2, 1, 0))
        p_in, e_in = ins[sl], ins[sl_next]
        k, j, i = np.nonzero(p_in != e_in)
        inside_p = p_in[k, j, i]
        i, j, k = i + lo[0], j + lo[1], k + lo[2]
        cells = []
        for dx, dy, dz in QUAD_CELLS[axis]:
            cells.append(number[k + dz, j + dy, i + dx])
        c = np.stack(cells, axis=1)
        assert (c >= 0).all(), "a quad names a cell that is not active"
        flipped = c[:, [0, 3, 2, 1]]
        quads.append(np.where(inside_p[:, None], c, flipped))
        keys.append(((k.astype(np.int64) * ny + j) * nx + i) * 3 + axis)
    if quads:
        keys, quads = np.concatenate(keys), np.concatenate(quads)
        quads = quads[np.argsort(keys, kind="stable")]
    else:
        quads = np.zeros((0, 4), np.int64)
    return dict(vertices=verts, vertex_object=vobj, quads=quads.astype(np.int32),
                cells=np.stack([ii, jj, kk], axis=1).astype(np.int32))
