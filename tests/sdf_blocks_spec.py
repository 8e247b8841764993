"""The definitions of rm_sdf_blocks_select, rm_sdf_grid_blocks and rm_sdf_mesh_blocks (include/raymarcher_amd.h) in NumPy, sharing
no code with the library.  Everything starts from a DENSE float32 lattice of 8·m + 1 points per axis: the active blocks are read off
it, a block list's values are gathered from it, and the sparse mesh is sdf_mesh_spec.surface_nets of the dense lattice, restricted
to the listed blocks and renumbered as the header orders it."""
import numpy as np

import sdf_mesh_spec as S

f32 = np.float32


def blocks_of(dense):
    """(mx, my, mz) of a dense lattice (nz, ny, nx) of 8·m + 1 points per axis."""
    nz, ny, nx = dense.shape
    assert all((n - 1) % 8 == 0 and n >= 9 for n in (nx, ny, nz)), "a virtual lattice has 8·m + 1 points per axis"
    return (nx - 1) // 8, (ny - 1) // 8, (nz - 1) // 8


def block_values(a, bi, bj, bk):
    """The 9×9×9 values of block (bi, bj, bk) of a dense array, as [c, b, a]."""
    return a[8 * bk:8 * bk + 9, 8 * bj:8 * bj + 9, 8 * bi:8 * bi + 9]


def all_blocks(blocks):
    """Every block of the lattice in linear order (bk·my + bj)·mx + bi → int32 (n, 4)."""
    mx, my, mz = blocks
    return np.array([(bi, bj, bk, 0) for bk in range(mz) for bj in range(my) for bi in range(mx)], np.int32).reshape(-1, 4)


def active_blocks(dense, iso):
    """rm_sdf_blocks_select: the blocks whose 729 points are not all inside and not all outside, in linear order → int32 (n, 4)."""
    ins = np.asarray(dense) < f32(iso)  # a NaN is outside
    out = []
    for bi, bj, bk, _ in all_blocks(blocks_of(dense)):
        v = block_values(ins, bi, bj, bk)
        if v.any() and not v.all():
            out.append((bi, bj, bk, 0))
    return np.array(out, np.int32).reshape(-1, 4)


def blocks_with_an_active_cell(dense, iso):
    """The blocks one of whose 512 cells is active in rm_sdf_mesh's sense (corners neither all inside nor all outside), in linear
    order → int32 (n, 4).  Computed cell by cell: the other side of the equivalence the header states."""
    ins = np.asarray(dense) < f32(iso)
    nz, ny, nx = ins.shape
    count = sum(ins[cz:nz - 1 + cz, cy:ny - 1 + cy, cx:nx - 1 + cx].astype(np.int32) for cz in (0, 1) for cy in (0, 1) for cx in (0, 1))
    active = (count > 0) & (count < 8)
    out = [(bi, bj, bk, 0) for bi, bj, bk, _ in all_blocks(blocks_of(dense)) if active[8 * bk:8 * bk + 8, 8 * bj:8 * bj + 8, 8 * bi:8 * bi + 8].any()]
    return np.array(out, np.int32).reshape(-1, 4)


def first_positions(block_list, blocks):
    """The block map: int64 (mz, my, mx), the position of the first entry that names each block, −1 where none does."""
    mx, my, mz = blocks
    first = np.full((mz, my, mx), -1, np.int64)
    for n, (bi, bj, bk) in enumerate(np.asarray(block_list).reshape(-1, 4)[:, :3].tolist()):
        if 0 <= bi < mx and 0 <= bj < my and 0 <= bk < mz and first[bk, bj, bi] < 0:
            first[bk, bj, bi] = n
    return first


def listed(block_list, blocks):
    """bool (n): which entries count (are not void) — inside the lattice and the first of their equals."""
    first = first_positions(block_list, blocks)
    mx, my, mz = blocks
    return np.array([0 <= bi < mx and 0 <= bj < my and 0 <= bk < mz and first[bk, bj, bi] == n
                     for n, (bi, bj, bk) in enumerate(np.asarray(block_list).reshape(-1, 4)[:, :3].tolist())], bool).reshape(-1)


def pack_blocks(dense, block_list, fill):
    """rm_sdf_grid_blocks: (n, 9, 9, 9) of dense's dtype, entry n the values of its block as [c, b, a]; a void entry's slot is `fill`."""
    dense = np.asarray(dense)
    bl = np.asarray(block_list).reshape(-1, 4)
    out = np.full((len(bl), 9, 9, 9), fill, dense.dtype)
    for n in np.nonzero(listed(bl, blocks_of(dense)))[0]:
        out[n] = block_values(dense, *bl[n, :3])
    return out


def mesh_blocks(dense, origin, step, iso, block_list, ids=None):
    """rm_sdf_mesh_blocks → dict(vertices (n, 4) float32, vertex_object (n) int32, quads (m, 4) int32, counts (vertices, quads, open
    vertices), cells (n, 3): each vertex's global cell, dense: the dense mesh)."""
    dense = np.asarray(dense)
    blocks = blocks_of(dense)
    m = S.surface_nets(dense, origin, step, iso, ids)
    first = first_positions(block_list, blocks)
    cells = m["cells"].astype(np.int64)
    pos = first[cells[:, 2] >> 3, cells[:, 1] >> 3, cells[:, 0] >> 3]  # of every dense vertex: its block's list position, −1 unlisted
    local = ((cells[:, 2] & 7) * 8 + (cells[:, 1] & 7)) * 8 + (cells[:, 0] & 7)
    keep = np.nonzero(pos >= 0)[0]
    keep = keep[np.argsort(pos[keep] * 512 + local[keep], kind="stable")]  # by list position, then by local cell index
    number = np.full(len(cells), -1, np.int64)
    number[keep] = np.arange(len(keep))
    dq = m["quads"].astype(np.int64)
    if len(dq):
        qc = cells[dq]  # (m, 4, 3): the four cells of every dense quad
        owner = qc.max(axis=1)  # P = corner 0 of the cell with the largest index on every axis: the other three lie at offsets 0 or −1
        same = (qc == qc[:, :1, :]).all(axis=1)  # the four cells share their index on the edge's axis alone
        assert (same.sum(axis=1) == 1).all()
        axis = same.argmax(axis=1)
        stored = (number[dq] >= 0).all(axis=1)
        opos = first[owner[:, 2] >> 3, owner[:, 1] >> 3, owner[:, 0] >> 3]
        olocal = ((owner[:, 2] & 7) * 8 + (owner[:, 1] & 7)) * 8 + (owner[:, 0] & 7)
        sel = np.nonzero(stored)[0]
        sel = sel[np.argsort((opos[sel] * 512 + olocal[sel]) * 3 + axis[sel], kind="stable")]
        quads = number[dq[sel]]
        dropped = dq[~stored]
        open_vertices = int((number[np.unique(dropped)] >= 0).sum())  # the listed vertices of the dense quads that the list drops
    else:
        quads, open_vertices = np.zeros((0, 4), np.int64), 0
    return dict(vertices=m["vertices"][keep], vertex_object=m["vertex_object"][keep], quads=quads.astype(np.int32),
                counts=(len(keep), len(quads), open_vertices), cells=m["cells"][keep], dense=m)


def truncated(mesh, max_vertices, max_quads):
    """What a call with these capacities stores: the first max_vertices vertices and max_quads quads; the counts stay the full ones."""
    return dict(mesh, vertices=mesh["vertices"][:max_vertices], vertex_object=mesh["vertex_object"][:max_vertices],
                quads=mesh["quads"][:max_quads])
