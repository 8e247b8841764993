"""The block-sparse lattice's definitions without a GPU.  First the NumPy specification (tests/sdf_blocks_spec.py) against what it
must mean — the sparse mesh IS the dense mesh, renumbered, wherever the list holds every block with an active cell — on the oracle's
lattices and on hand-made ones with NaN, infinities and values equal to iso.  Then the library's block-local arithmetic
(raymarcher_amd/csrc/rm_surface_nets_blocks.h, the code the kernels call), run serially by a stand-alone CPU program under the address
and undefined-behaviour sanitizers, against that specification in every bit."""
import numpy as np
import pytest

import helpers as h
import sdf_blocks_helpers as K
import sdf_blocks_spec as B

CASE_NAMES = sorted(list(K.ORACLE_CASES) + list(K.handmade()))
SURFACE_CASES = [n for n in CASE_NAMES if not n.startswith("all_")]


def cell_tuples(mesh, quads=None):
    """Each quad as the bytes of its four global cells, in order: a name that does not depend on the numbering."""
    q = mesh["quads"] if quads is None else quads
    return [mesh["cells"][row].tobytes() for row in q]


def assert_is_the_dense_mesh(m, what):
    dense = m["dense"]
    assert m["counts"] == (len(dense["vertices"]), len(dense["quads"]), 0), what
    # vertex bits: the dense vertex of the same cell
    index = {c.tobytes(): n for n, c in enumerate(dense["cells"])}
    back = np.array([index[c.tobytes()] for c in m["cells"]], np.int64)
    assert len(np.unique(back)) == len(back) == len(dense["vertices"]), what
    h.assert_bit_equal(m["vertices"], dense["vertices"][back], f"{what}: vertices")
    assert (m["vertex_object"] == dense["vertex_object"][back]).all(), what
    # quads mapped through the cells: the dense quads, each once, corner for corner
    assert sorted(cell_tuples(m)) == sorted(cell_tuples(dense)), what


@pytest.mark.parametrize("name", CASE_NAMES)
def test_a_block_is_active_iff_one_of_its_cells_is(name):
    dense, _ids, _o, _s, iso = K.case(name)
    by_points, by_cells = B.active_blocks(dense, iso), B.blocks_with_an_active_cell(dense, iso)
    assert by_points.tobytes() == by_cells.tobytes() and by_points.shape == by_cells.shape
    if name in K.ORACLE_CASES:
        assert len(by_points) > 0, "the lattice should cross a surface"
    if name == "bulb_33":
        assert len(by_points) < np.prod(B.blocks_of(dense)), "the lattice should have blocks without surface too"
    if name.startswith("all_"):
        assert len(by_points) == 0


@pytest.mark.parametrize("name", CASE_NAMES)
def test_the_full_list_and_the_active_list_give_the_dense_mesh_renumbered(name):
    dense, ids, origin, step, iso = K.case(name)
    blocks = B.blocks_of(dense)
    full = B.mesh_blocks(dense, origin, step, iso, B.all_blocks(blocks), ids)
    assert_is_the_dense_mesh(full, f"{name}: every block")
    # the full list in linear order keeps the blocks' order, so vertex keys (block, local cell) rise
    act = B.mesh_blocks(dense, origin, step, iso, B.active_blocks(dense, iso), ids)
    assert_is_the_dense_mesh(act, f"{name}: the active blocks")
    if name in SURFACE_CASES:
        assert full["counts"][0] > 0
    empty = B.mesh_blocks(dense, origin, step, iso, np.zeros((0, 4), np.int32), ids)
    assert empty["counts"] == (0, 0, 0)


@pytest.mark.parametrize("name", sorted(K.ORACLE_CASES))
def test_removing_an_active_block_opens_the_mesh(name):
    dense, ids, origin, step, iso = K.case(name)
    act = B.active_blocks(dense, iso)
    whole = B.mesh_blocks(dense, origin, step, iso, act, ids)
    per_block = [int(((whole["cells"] >> 3) == blk[:3]).all(axis=1).sum()) for blk in act]
    r = int(np.argmax(per_block))  # the block with the most vertices: quads cross its faces
    less = B.mesh_blocks(dense, origin, step, iso, np.delete(act, r, axis=0), ids)
    assert less["counts"][2] > 0 and less["counts"][0] == whole["counts"][0] - per_block[r]
    dm = whole["dense"]
    in_removed = ((dm["cells"] >> 3) == act[r, :3]).all(axis=1)
    avoid = [t for t, q in zip(cell_tuples(dm), dm["quads"]) if not in_removed[q].any()]
    assert sorted(cell_tuples(less)) == sorted(avoid)
    # the open vertices, counted the other way: kept vertices that a quad through the removed block's cells names
    touched = np.unique(dm["quads"][in_removed[dm["quads"]].any(axis=1)])
    assert less["counts"][2] == int((~in_removed[touched]).sum())


@pytest.mark.parametrize("name", ["sphere_25", "bulb_33", "nonfinite_17x9x9", "touches_boundary_17x9x9"])
def test_a_messy_list_obeys_the_orders_and_the_first_wins_rule(name):
    dense, ids, origin, step, iso = K.case(name)
    blocks = B.blocks_of(dense)
    bl = K.messy_list(blocks)
    keep = B.listed(bl, blocks)
    assert keep.sum() == np.prod(blocks) and (~keep).sum() >= 2
    seen = {}
    for n, row in enumerate(bl[:, :3].tolist()):
        ok = all(0 <= row[a] < blocks[a] for a in range(3))
        assert keep[n] == (ok and tuple(row) not in seen), n
        if ok:
            seen.setdefault(tuple(row), n)
    m = B.mesh_blocks(dense, origin, step, iso, bl, ids)
    assert_is_the_dense_mesh(m, f"{name}: the messy list")
    pos = np.array([seen[tuple(c)] for c in (m["cells"] >> 3).tolist()], np.int64)
    local = ((m["cells"][:, 2] & 7) * 8 + (m["cells"][:, 1] & 7)) * 8 + (m["cells"][:, 0] & 7)
    assert (np.diff(pos * 512 + local) > 0).all(), "vertex order: list position, then local cell index"
    if len(m["quads"]):
        owner = m["cells"][m["quads"]].max(axis=1)
        opos = np.array([seen[tuple(c)] for c in (owner >> 3).tolist()], np.int64)
        olocal = ((owner[:, 2] & 7) * 8 + (owner[:, 1] & 7)) * 8 + (owner[:, 0] & 7)
        assert (np.diff(opos * 512 + olocal) >= 0).all(), "quad order: the owning block's list position, then P's local index"
    packed = B.pack_blocks(dense, bl, np.float32(-7.5))
    assert (packed[~keep] == np.float32(-7.5)).all()
    for n in np.nonzero(keep)[0][:5]:
        bi, bj, bk = bl[n, :3]
        assert packed[n].tobytes() == np.ascontiguousarray(dense[8 * bk:8 * bk + 9, 8 * bj:8 * bj + 9, 8 * bi:8 * bi + 9]).tobytes()


def test_capacities_truncate_without_changing_the_counts():
    dense, ids, origin, step, iso = K.case("sphere_25")
    m = B.mesh_blocks(dense, origin, step, iso, B.active_blocks(dense, iso), ids)
    nv, nq, _ = m["counts"]
    for mv, mq in ((nv, nq), (nv - 1, nq - 1), (1, 0), (0, 3)):
        t = B.truncated(m, mv, mq)
        assert t["counts"] == m["counts"]
        assert t["vertices"].tobytes() == m["vertices"][:mv].tobytes() and t["quads"].tobytes() == m["quads"][:mq].tobytes()
        assert len(t["vertex_object"]) == min(mv, nv)


@pytest.fixture(scope="module")
def cpu_program(tmp_path_factory):
    return K.build_cpu_program(tmp_path_factory.mktemp("sdf_blocks_cpu"))


def _lists(dense, iso):
    blocks = B.blocks_of(dense)
    act = B.active_blocks(dense, iso)
    out = {"full": B.all_blocks(blocks), "active": act, "messy": K.messy_list(blocks)}
    if len(act) > 1:
        out["one_removed"] = np.delete(act, len(act) // 2, axis=0)
    return out


@pytest.mark.parametrize("name", CASE_NAMES)
def test_the_shared_header_on_the_cpu_equals_the_spec_in_every_bit(cpu_program, tmp_path, name):
    dense, ids, origin, step, iso = K.case(name)
    blocks = B.blocks_of(dense)
    for label, bl in _lists(dense, iso).items():
        want = B.mesh_blocks(dense, origin, step, iso, bl, ids)
        packed = B.pack_blocks(dense, bl, np.float32(np.nan))
        packed_ids = B.pack_blocks(ids, bl, np.int32(-9)) if ids is not None else None
        got = K.run_cpu_program(cpu_program, tmp_path, packed, packed_ids, bl, blocks, origin, step, iso)
        K.assert_mesh_equal(got, want, f"{name}, {label} list")
        keep = B.listed(bl, blocks)
        active = {tuple(r) for r in B.active_blocks(dense, iso)[:, :3].tolist()}
        want_flags = np.array([(1 if tuple(r) in active else 0) if k else -1 for r, k in zip(bl[:, :3].tolist(), keep)], np.int32)
        assert (got["active"] == want_flags).all(), f"{name}, {label} list: the select rule per entry"
