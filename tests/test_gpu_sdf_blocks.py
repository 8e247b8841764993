"""rm_sdf_blocks_select, rm_sdf_grid_blocks and rm_sdf_mesh_blocks on the GPU, bit for bit: the blocks' values against rm_sdf_grid of
the same lattice gathered per block, the selection against the NumPy specification's active blocks of that lattice, the mesh against
the specification (tests/sdf_blocks_spec.py) in every word — with guard words around every output — then the Python layer."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers as h
import sdf_blocks_helpers as K
import sdf_blocks_spec as B
import sdf_helpers as V
from raymarcher_amd import abi, lib

pytestmark = pytest.mark.gpu

SCENES = ("sphere", "primitives", "menger", "bulb_plain", "bulb_moved", "julia")  # the table walk (with the sponge prologue) and both bulb classes
GRIDS = ((1, 1, 1), (2, 1, 1), (3, 2, 2))
ISO = {"sphere": 0.0, "primitives": 0.0, "menger": 0.0, "bulb_plain": 0.001, "bulb_moved": 0.001, "julia": 0.001}


def vec(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def table_only(objs, no, g):
    return h.tables_of((abi.RmCamera(), objs, no, None, 0, g))


def guards_intact(g):
    """The two guard bands of a helpers.Guarded, without its demand that every payload word was written (void slots are not)."""
    end = g.guard + g.nbytes
    return bool(g._unwritten(g.buf[:g.guard]).all()) and bool(g._unwritten(g.buf[end:]).all())


_DENSE = {}


def dense_lattice(renderer, name, blocks):
    """rm_sdf_grid on the lattice of 8·m + 1 points per axis across the table's box → (dist, ids, origin, step), computed once per
    process and read-only."""
    key = (name, tuple(blocks))
    if key not in _DENSE:
        objs, no, g, s = V.scene(name)
        dims = tuple(8 * m + 1 for m in blocks)
        origin, step = V.lattice_of(name, dims)
        dist, ids = renderer.sdf_grid(table_only(objs, no, g), s, origin, step, dims, ids=True)
        out = (dist.cpu().numpy(), ids.cpu().numpy(), origin, step)
        for a in out:
            a.setflags(write=False)
        _DENSE[key] = out
    return _DENSE[key]


# ---------------------------------------------------------------- rm_sdf_grid_blocks
def grid_blocks_call(renderer, name, origin, step, blocks, bl, ids=True):
    """rm_sdf_grid_blocks into poisoned, guarded outputs → (dist, ids or None) as arrays (n, 9, 9, 9) with the poison left where
    nothing was written; the guards are checked."""
    objs, no, g, s = V.scene(name)
    n = len(bl)
    d_bl = torch.from_numpy(np.ascontiguousarray(bl, np.int32)).to(renderer.device)
    gd = h.Guarded((n, 9, 9, 9), torch.float32, h.FLOAT_POISON, renderer.device)
    gi = h.Guarded((n, 9, 9, 9), torch.int32, h.FLOAT_POISON, renderer.device) if ids else None
    st = lib().rm_sdf_grid_blocks(objs, no, C.byref(g), C.byref(s), vec(origin), vec(step), blocks[0], blocks[1], blocks[2], ptr(d_bl), n,
                                  ptr(gd.payload), ptr(gi.payload) if ids else None, renderer._stream())
    assert st == abi.RM_OK, lib().rm_last_error().decode()
    assert lib().rm_debug_last_path() == abi.RM_PATH_SDF_GRID_BLOCKS == 19 and lib().rm_debug_last_split() == 0
    assert guards_intact(gd) and (not ids or guards_intact(gi)), "a guard band was written"
    return gd.payload.cpu().numpy(), (gi.payload.cpu().numpy() if ids else None)


def poison_of(dtype):
    g = h.Guarded((1, 1), torch.float32, h.FLOAT_POISON, "cpu")
    return g.payload.numpy().view(dtype)[0, 0]


@pytest.mark.parametrize("name", SCENES)
def test_grid_blocks_equals_the_dense_lattice_gathered_per_block(renderer, name):
    pf, pi = poison_of(np.float32), poison_of(np.int32)
    for blocks in GRIDS:
        dist, ids, origin, step = dense_lattice(renderer, name, blocks)
        every = B.all_blocks(blocks)
        lists = {"one": every[-1:], "all": every, "messy": K.messy_list(blocks)}
        if len(every) > 1:
            lists["two"] = every[[len(every) - 1, 0]]
        for label, bl in lists.items():
            got_d, got_i = grid_blocks_call(renderer, name, origin, step, blocks, bl)
            # a void entry's slot holds the poison it was given
            V.assert_bits(got_d, B.pack_blocks(dist, bl, pf), f"{name} {blocks} {label}: d_dist")
            assert (got_i == B.pack_blocks(ids, bl, pi)).all(), f"{name} {blocks} {label}: d_objectId"
            alone, _ = grid_blocks_call(renderer, name, origin, step, blocks, bl, ids=False)
            V.assert_bits(alone, got_d, f"{name} {blocks} {label}: d_dist without d_objectId")
        assert (~B.listed(lists["messy"], blocks)).sum() >= 2
    dist, _, _, _ = dense_lattice(renderer, name, GRIDS[-1])
    assert (dist < ISO[name]).any() and (dist >= ISO[name]).any(), "the lattice does not cross the surface"


# ---------------------------------------------------------------- rm_sdf_blocks_select
def select_call(renderer, name, origin, step, blocks, iso, capacity):
    objs, no, g, s = V.scene(name)
    count, check_c = h.guarded((1, 1), torch.int32, device=renderer.device)
    out = h.Guarded((capacity, 4), torch.int32, h.FLOAT_POISON, renderer.device) if capacity else None
    st = lib().rm_sdf_blocks_select(objs, no, C.byref(g), C.byref(s), vec(origin), vec(step), blocks[0], blocks[1], blocks[2], float(iso), capacity,
                                    ptr(out.payload) if capacity else None, ptr(count), renderer._stream())
    assert st == abi.RM_OK, lib().rm_last_error().decode()
    assert lib().rm_debug_last_path() == abi.RM_PATH_SDF_BLOCKS_SELECT == 18 and lib().rm_debug_last_split() == 0
    check_c()
    assert out is None or guards_intact(out), "a guard band was written"
    n = int(count.cpu().numpy().view(np.uint32)[0, 0])
    return n, (out.payload.cpu().numpy() if capacity else np.zeros((0, 4), np.int32))


def assert_select(renderer, name, blocks, iso):
    dist, _ids, origin, step = dense_lattice(renderer, name, blocks)
    want = B.active_blocks(dist, iso)
    n, _ = select_call(renderer, name, origin, step, blocks, iso, 0)
    assert n == len(want), f"{name} {blocks}: the counting call"
    total = int(np.prod(blocks))
    pi = poison_of(np.int32)
    for cap in sorted({total, len(want), max(len(want) - 1, 0), 1} - {0}):
        n, got = select_call(renderer, name, origin, step, blocks, iso, cap)
        assert n == len(want), f"{name} {blocks}: the count with capacity {cap}"
        k = min(cap, len(want))
        assert (got[:k] == want[:k]).all(), f"{name} {blocks}: the list with capacity {cap}"
        assert (got[k:] == pi).all(), f"{name} {blocks}: entries past the count were written"
    return want


@pytest.mark.parametrize("name", SCENES)
def test_select_equals_the_active_blocks_of_the_dense_lattice(renderer, name):
    for blocks in GRIDS:
        assert_select(renderer, name, blocks, ISO[name])


def test_select_across_the_scans_boundary(renderer):
    """11×10×10 = 1 100 blocks (89×81×81 points): two shares of 1024 flags, and lists on both sides of the boundary."""
    want = assert_select(renderer, "menger", (11, 10, 10), 0.0)
    lin = (want[:, 2] * 10 + want[:, 1]) * 11 + want[:, 0]
    assert (lin < 1024).any() and (lin >= 1024).any(), "the sponge reaches the lattice's last slab of blocks"


# ---------------------------------------------------------------- rm_sdf_mesh_blocks
def mesh_blocks_call(renderer, packed, packed_ids, bl, blocks, origin, step, iso, max_v, max_q, want_vobj=True, stream=None):
    """rm_sdf_mesh_blocks on host blocks into guarded outputs of exactly the capacities → (counts, vertices, vertex ids, quads)."""
    dev = renderer.device
    n = len(bl)
    d = torch.from_numpy(np.array(packed, dtype=np.float32)).to(dev)
    i = torch.from_numpy(np.array(packed_ids, dtype=np.int32)).to(dev) if packed_ids is not None else None
    d_bl = torch.from_numpy(np.ascontiguousarray(bl, np.int32)).to(dev)
    counts, check_c = h.guarded((1, 3), torch.int32, device=dev)
    v, check_v = h.guarded((max_v, 4), torch.float32, device=dev) if max_v else (None, None)
    vo, check_o = h.guarded((1, max_v), torch.int32, device=dev) if max_v and want_vobj else (None, None)
    q, check_q = h.guarded((max_q, 4), torch.int32, device=dev) if max_q else (None, None)
    path_before = lib().rm_debug_last_path()
    st = lib().rm_sdf_mesh_blocks(ptr(d), ptr(i), ptr(d_bl), n, blocks[0], blocks[1], blocks[2], vec(origin), vec(step), float(iso), max_v, max_q,
                                  ptr(v), ptr(vo), ptr(q), ptr(counts),
                                  C.c_void_p(stream.cuda_stream) if stream is not None else renderer._stream())
    assert st == abi.RM_OK, lib().rm_last_error().decode()
    if stream is not None:
        stream.synchronize()
    assert lib().rm_debug_last_path() == path_before, "rm_sdf_mesh_blocks is not a render launch"
    for check in (check_c, check_v, check_o, check_q):
        if check:
            check()
    host = lambda t, shape, dt: t.cpu().numpy().reshape(shape) if t is not None else np.zeros(shape, dt)  # noqa: E731
    return (tuple(int(x) for x in counts.cpu().numpy().view(np.uint32).reshape(-1)), host(v, (max_v, 4), np.float32),
            host(vo, (max_v,), np.int32), host(q, (max_q, 4), np.int32))


def assert_mesh_blocks(renderer, dense, ids, origin, step, iso, bl, what, stream=None):
    """The counting call, exact capacities and capacities one below the counts, all against the specification."""
    blocks = B.blocks_of(dense)
    want = B.mesh_blocks(dense, origin, step, iso, bl, ids)
    packed = B.pack_blocks(dense, bl, np.float32(np.nan))  # a void slot's values are never read: NaN would show
    packed_ids = B.pack_blocks(ids, bl, np.int32(-9)) if ids is not None else None
    nv, nq, _ = want["counts"]
    counts, _, _, _ = mesh_blocks_call(renderer, packed, packed_ids, bl, blocks, origin, step, iso, 0, 0, stream=stream)
    assert counts == want["counts"], f"{what}: the counting call {counts} against {want['counts']}"
    for mv, mq in ((nv, nq), (max(nv - 1, 0), max(nq - 1, 0))):
        if mv == 0 and mq == 0:
            continue
        counts, v, vo, q = mesh_blocks_call(renderer, packed, packed_ids, bl, blocks, origin, step, iso, mv, mq, stream=stream)
        assert counts == want["counts"], f"{what}: counts with capacities {mv}, {mq}"
        V.assert_bits(v, want["vertices"][:mv], f"{what}: vertices, capacity {mv}")
        assert (vo == want["vertex_object"][:mv]).all(), f"{what}: vertex ids, capacity {mv}"
        assert (q == want["quads"][:mq]).all(), f"{what}: quads, capacity {mq}"
    return want


def _lists(dense, iso):
    blocks = B.blocks_of(dense)
    act = B.active_blocks(dense, iso)
    out = {"full": B.all_blocks(blocks), "active": act, "messy": K.messy_list(blocks)}
    if len(act) > 1:
        out["one_removed"] = np.delete(act, len(act) // 2, axis=0)
    return out


@pytest.mark.parametrize("name", sorted(list(K.ORACLE_CASES) + list(K.handmade())))
def test_mesh_blocks_equals_the_spec_in_every_word(renderer, name):
    dense, ids, origin, step, iso = K.case(name)
    for label, bl in _lists(dense, iso).items():
        want = assert_mesh_blocks(renderer, dense, ids, origin, step, iso, bl, f"{name}, {label} list")
        if label in ("full", "active", "messy"):
            assert want["counts"][2] == 0 and want["counts"][0] == len(want["dense"]["vertices"])
        if label == "one_removed" and name in K.ORACLE_CASES:
            assert want["counts"][2] > 0
    if ids is not None:
        bl = B.active_blocks(dense, iso)
        want = B.mesh_blocks(dense, origin, step, iso, bl, ids)
        nv, nq, _ = want["counts"]
        if nv:
            packed = B.pack_blocks(dense, bl, np.float32(np.nan))
            _, _, vo, _ = mesh_blocks_call(renderer, packed, None, bl, B.blocks_of(dense), origin, step, iso, nv, 0)
            assert (vo == -1).all(), "d_vertexObject without d_objectId is −1"
            mesh_blocks_call(renderer, packed, B.pack_blocks(ids, bl, np.int32(-9)), bl, B.blocks_of(dense), origin, step, iso, nv, nq, want_vobj=False)


def test_mesh_blocks_of_a_long_list_on_two_streams_and_the_workspace(renderer):
    """1 030 entries that hold the 12 blocks of the 3×2×2 lattice among voids and duplicates: the scan over the entries crosses 1024.
    Four calls on two streams; then the workspace is released, refused under a limit, and served again."""
    dense, ids, origin, step, iso = K.case("primitives_25")
    blocks = B.blocks_of(dense)
    rng = np.random.default_rng(11)
    bl = np.empty((1030, 4), np.int32)
    bl[:, :3] = rng.integers(-2, 6, (1030, 3))  # mostly outside the lattice, the rest mostly repeats
    bl[:, 3] = 0
    every = B.all_blocks(blocks)
    places = np.sort(rng.choice(1030, len(every), replace=False))
    places[-3:] = (1024, 1027, 1029)  # entries that count beyond the scan's first round
    bl[places] = every[rng.permutation(len(every))]
    keep = B.listed(bl, blocks)
    assert keep.sum() == 12 and keep[1024:].any() and keep[:1024].any()
    s1, s2 = torch.cuda.Stream(device=renderer.device), torch.cuda.Stream(device=renderer.device)
    want = assert_mesh_blocks(renderer, dense, ids, origin, step, iso, bl, "the long list, stream 1", stream=s1)
    assert_mesh_blocks(renderer, dense, ids, origin, step, iso, bl, "the long list, stream 2", stream=s2)
    assert want["counts"][2] == 0 and want["counts"][0] == len(want["dense"]["vertices"]) > 100
    freed = C.c_ulonglong(0)
    assert lib().rm_release_workspaces(C.byref(freed)) == abi.RM_OK and freed.value > 0
    packed = torch.from_numpy(B.pack_blocks(dense, bl, np.float32(0))).to(renderer.device)
    d_bl = torch.from_numpy(bl).to(renderer.device)
    counts = torch.zeros(3, dtype=torch.int32, device=renderer.device)
    call = lambda: lib().rm_sdf_mesh_blocks(ptr(packed), None, ptr(d_bl), len(bl), *blocks, vec(origin), vec(step), float(iso), 0, 0, None, None,  # noqa: E731
                                            None, ptr(counts), renderer._stream())
    assert lib().rm_set_workspace_limit(64) == abi.RM_OK
    try:
        assert call() == abi.RM_ERR_DEVICE and "rm_set_workspace_limit" in lib().rm_last_error().decode()
        objs, no, g, s = V.scene("primitives")
        one = torch.zeros(1, dtype=torch.int32, device=renderer.device)
        st = lib().rm_sdf_blocks_select(objs, no, C.byref(g), C.byref(s), vec(origin), vec(step), 11, 10, 10, 0.0, 0, None, ptr(one), renderer._stream())
        assert st == abi.RM_ERR_DEVICE and "rm_set_workspace_limit" in lib().rm_last_error().decode()
    finally:
        lib().rm_set_workspace_limit(0)
    assert call() == abi.RM_OK and tuple(counts.tolist()) == want["counts"]
    # an empty list: three zero counts, nothing else touched
    counts.fill_(7)
    st = lib().rm_sdf_mesh_blocks(None, None, None, 0, *blocks, vec(origin), vec(step), float(iso), 0, 0, None, None, None, ptr(counts), renderer._stream())
    assert st == abi.RM_OK and counts.tolist() == [0, 0, 0]


# ---------------------------------------------------------------- the Python layer
def test_scene_mesh_sparse_equals_extract_mesh_on_its_own_padded_lattice(renderer):
    objs, no, g, s = V.scene("sphere_cube")
    t = table_only(objs, no, g)
    res, iso = 30, 0.001
    v, q, vo = (x.cpu().numpy() for x in renderer.scene_mesh_sparse(t, s, res, iso))
    origin, step, dims = renderer._scene_lattice(t, res, None)
    blocks = [(d + 6) // 8 for d in dims]
    padded = [8 * m + 1 for m in blocks]
    assert any(p > d for p, d in zip(padded, dims))
    dist, ids = renderer.sdf_grid(t, s, origin, (step,) * 3, padded, ids=True)
    dv, dq, dvo = (x.cpu().numpy() for x in renderer.extract_mesh(dist, origin, (step,) * 3, iso, ids))
    o32, s32 = np.asarray(origin, np.float32), np.full(3, step, np.float32)
    want = B.mesh_blocks(dist.cpu().numpy(), o32, s32, iso, B.active_blocks(dist.cpu().numpy(), iso), ids.cpu().numpy())
    assert want["counts"] == (len(dv), len(dq), 0)
    V.assert_bits(v, want["vertices"], "scene_mesh_sparse: vertices")
    assert (vo == want["vertex_object"]).all() and (q == want["quads"]).all()
    # and through the renumbering it is extract_mesh's mesh: the same vertices, the same quads over them
    key = lambda vs, qs: sorted(np.ascontiguousarray(vs[row]).tobytes() for row in qs)  # noqa: E731
    assert sorted(x.tobytes() for x in v) == sorted(x.tobytes() for x in dv) and key(v, q) == key(dv, dq)
    assert len(v) > 500 and V.assert_closed_oriented(q, "scene_mesh_sparse") > 0
    # the pieces: the list is the specification's, the blocks are the dense lattice's
    bl = renderer.sdf_active_blocks(t, s, origin, (step,) * 3, blocks, iso)
    assert (bl.cpu().numpy() == B.active_blocks(dist.cpu().numpy(), iso)).all()
    gb = renderer.sdf_grid_blocks(t, s, origin, (step,) * 3, blocks, bl)
    V.assert_bits(gb.cpu().numpy(), B.pack_blocks(dist.cpu().numpy(), bl.cpu().numpy(), np.float32(0)), "sdf_grid_blocks")
    v2, q2, nopen = renderer.extract_mesh_blocks(gb, bl, blocks, origin, (step,) * 3, iso)
    assert nopen == 0 and torch.equal(v2.cpu(), torch.from_numpy(v)) and (q2.cpu().numpy() == q).all()
    _, _, nopen = renderer.extract_mesh_blocks(gb[1:].contiguous(), bl[1:].contiguous(), blocks, origin, (step,) * 3, iso)
    assert nopen > 0
    with pytest.raises(ValueError):
        renderer.scene_mesh_sparse(t, s, 4098)


def test_bake_mesh_sparse_against_shade_points_on_its_vertices(renderer):
    objs, no, g, s = V.scene("sphere_cube")
    lights = (abi.RmLight * 1)(h.make_light(abi.RM_LIGHT_DIRECTIONAL, (1, 1, 1), (-0.3, -1, -0.5)))
    for i in range(no):
        for k in range(3):
            objs[i].cAmbient[k], objs[i].cDiffuse[k] = 0.3, 0.8
    t = h.tables_of((h.make_camera((0, 0, 5), (0, 0, -1), (0, 1, 0), 40.0, 8, 8), objs, no, lights, 1, g))
    res, iso = 20, 0.001
    verts, quads, obj, normal, ao, rgb = renderer.bake_mesh_sparse(t, s, res, iso)
    v0, q0, _vo0, step = renderer._scene_mesh_sparse(t, s, res, iso, None)
    assert torch.equal(quads, q0) and len(verts) == len(v0) > 100
    n_, _d, pos, oid, aos, col = renderer.shade_points(t, s, v0, colour=True, ao=True, project=2, iso=iso, max_move=0.5 * step * 3.0 ** 0.5)
    assert torch.equal(verts[:, :3], pos) and bool((verts[:, 3] == 0).all())
    assert torch.equal(obj, oid) and torch.equal(normal.view(torch.int32), n_.contiguous().view(torch.int32))
    assert torch.equal(ao.view(torch.int32), aos.view(torch.int32))
    assert torch.equal(rgb, renderer.to_rgba8(col.view(1, len(v0), 4))[0, :, 0:3])
    # the same mesh as the dense route's wherever both lattices hold the surface: the vertex sets agree
    dv, _dq, _ = renderer.scene_mesh(t, s, res, iso)
    assert sorted(x.tobytes() for x in dv.cpu().numpy()) == sorted(x.tobytes() for x in v0.cpu().numpy())
