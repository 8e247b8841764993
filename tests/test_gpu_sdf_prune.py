"""rm_sdf_blocks_select_pruned on the GPU, word for word: the list, the count and the number of candidates against the NumPy
specification (tests/sdf_prune_spec.py) of the dense lattice that rm_sdf_grid gives for the same points — into poisoned outputs
between guard words — and against rm_sdf_blocks_select itself; then the Python layer against the *_sparse methods."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers as h
import sdf_blocks_spec as B
import sdf_helpers as V
import sdf_prune_spec as P
import trace_helpers as T
from raymarcher_amd import abi, lib

pytestmark = pytest.mark.gpu

inf = float("inf")
SCENES = ("sphere", "primitives", "menger", "bulb_plain", "bulb_moved", "julia")  # the table walk (with the sponge prologue) and both bulb classes
ISO = {"sphere": 0.0, "primitives": 0.0, "menger": 0.0, "bulb_plain": 0.001, "bulb_moved": 0.001, "julia": 0.001}
CONSTANTS = ((1.0, inf), (1.0, 1.0), (0.125, inf), (0.0, 0.0), (inf, inf))
BIG = (16, 16, 16)
SMALL = ((1, 1, 1), (2, 1, 1), (3, 2, 2), (5, 4, 3))


def vec(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def guards_intact(g):
    """The two guard bands of a helpers.Guarded, without its demand that every payload word was written (entries past the count
    are not)."""
    end = g.guard + g.nbytes
    return bool(g._unwritten(g.buf[:g.guard]).all()) and bool(g._unwritten(g.buf[end:]).all())


POISON = np.array([h.FLOAT_POISON], np.uint32).view(np.int32)[0]
_DENSE = {}


def dense_lattice(renderer, name, blocks):
    """rm_sdf_grid on the lattice of 8·m + 1 points per axis across the table's box, into poisoned, guarded outputs, and the
    exhaustive list of its active blocks → (dist, origin, step, active), computed once per process and read-only."""
    key = (name, tuple(blocks))
    if key not in _DENSE:
        objs, no, g, s = V.scene(name)
        nx, ny, nz = (8 * m + 1 for m in blocks)
        origin, step = V.lattice_of(name, (nx, ny, nz))
        dist, check = h.guarded((nz, ny, nx), torch.float32, device=renderer.device)
        st = lib().rm_sdf_grid(objs, no, C.byref(g), C.byref(s), vec(origin), vec(step), nx, ny, nz, ptr(dist), None, renderer._stream())
        assert st == abi.RM_OK, lib().rm_last_error().decode()
        check()
        dist = dist.cpu().numpy()
        out = (dist, origin, step, B.active_blocks(dist, ISO[name]))
        for a in out:
            a.setflags(write=False)
        _DENSE[key] = out
    return _DENSE[key]


def pruned_call(renderer, name, origin, step, blocks, iso, l_out, l_in, capacity, stream=None):
    """rm_sdf_blocks_select_pruned into poisoned, guarded outputs → (d_count[0], d_count[1], the capacity's rows)."""
    objs, no, g, s = V.scene(name)
    count, check_c = h.guarded((1, 2), torch.int32, device=renderer.device)
    out = h.Guarded((capacity, 4), torch.int32, h.FLOAT_POISON, renderer.device) if capacity else None
    st = lib().rm_sdf_blocks_select_pruned(objs, no, C.byref(g), C.byref(s), vec(origin), vec(step), blocks[0], blocks[1], blocks[2], float(iso),
                                           l_out, l_in, capacity, ptr(out.payload) if capacity else None, ptr(count),
                                           C.c_void_p(stream.cuda_stream) if stream is not None else renderer._stream())
    assert st == abi.RM_OK, lib().rm_last_error().decode()
    if stream is not None:
        stream.synchronize()
    assert lib().rm_debug_last_path() == abi.RM_PATH_SDF_BLOCKS_SELECT_PRUNED == 20 and lib().rm_debug_last_split() == 0
    check_c()
    assert out is None or guards_intact(out), "a guard band was written"
    n, cand = (int(x) for x in count.cpu().numpy().view(np.uint32).reshape(-1))
    return n, cand, (out.payload.cpu().numpy() if capacity else np.zeros((0, 4), np.int32))


def select_call(renderer, name, origin, step, blocks, iso, capacity):
    """rm_sdf_blocks_select, the exhaustive entry → (count, rows)."""
    objs, no, g, s = V.scene(name)
    count, check_c = h.guarded((1, 1), torch.int32, device=renderer.device)
    out = h.Guarded((capacity, 4), torch.int32, h.FLOAT_POISON, renderer.device)
    st = lib().rm_sdf_blocks_select(objs, no, C.byref(g), C.byref(s), vec(origin), vec(step), blocks[0], blocks[1], blocks[2], float(iso), capacity,
                                    ptr(out.payload), ptr(count), renderer._stream())
    assert st == abi.RM_OK, lib().rm_last_error().decode()
    check_c()
    return int(count.cpu().numpy().view(np.uint32)[0, 0]), out.payload.cpu().numpy()


def assert_pruned(renderer, name, blocks, l_out, l_in, capacities=None, stream=None):
    """One call per capacity (default: one more than the exhaustive count, so the words past the list show) against the spec →
    (the spec's list, the spec's candidates, the exhaustive list)."""
    dist, origin, step, active = dense_lattice(renderer, name, blocks)
    iso = ISO[name]
    want, cand = P.pruned_blocks(dist, step, iso, l_out, l_in, active)
    what = f"{name} {blocks} ({l_out}, {l_in})"
    for cap in capacities if capacities is not None else (len(active) + 1,):
        n, c, got = pruned_call(renderer, name, origin, step, blocks, iso, l_out, l_in, cap, stream)
        assert (n, c) == (len(want), cand), f"{what}: d_count {(n, c)} against {(len(want), cand)} with capacity {cap}"
        k = min(cap, len(want))
        assert (got[:k] == want[:k]).all(), f"{what}: the list with capacity {cap}"
        assert (got[k:] == POISON).all(), f"{what}: entries past the count were written"
    return want, cand, active


# ---------------------------------------------------------------- the call against the specification
@pytest.mark.parametrize("name", SCENES)
def test_list_count_and_candidates_equal_the_spec_in_every_word(renderer, name):
    dist, origin, step, active = dense_lattice(renderer, name, BIG)
    assert len(active) > 50, "the lattice does not cross the surface"
    for l_out, l_in in CONSTANTS:
        want, cand, _ = assert_pruned(renderer, name, BIG, l_out, l_in)
        if (l_out, l_in) == (inf, inf):  # no block is discarded: the exhaustive entry's output in every word
            n, rows = select_call(renderer, name, origin, step, BIG, ISO[name], len(active) + 1)
            _, _, mine = pruned_call(renderer, name, origin, step, BIG, ISO[name], inf, inf, len(active) + 1)
            assert n == len(want) == len(active) and cand == int(np.prod(BIG)) and (rows == mine).all()
        if (l_out, l_in) == (1.0, inf):
            assert len(want) == len(active), f"{name}: (1, inf) lost {len(active) - len(want)} blocks"
            assert cand < int(np.prod(BIG))
    if name == "primitives":
        assert step[2] != step[0], "the primitives' box has anisotropic steps"
        assert len(assert_pruned(renderer, name, BIG, 0.125, inf)[0]) < len(active), "an eighth of the bound loses blocks"
    if name == "julia":
        assert len(active) - len(assert_pruned(renderer, name, BIG, 1.0, 1.0)[0]) == 4, "the four interior pockets"


@pytest.mark.parametrize("name", ("sphere", "menger", "bulb_plain"))
def test_counting_call_and_capacities_around_the_count(renderer, name):
    dist, origin, step, active = dense_lattice(renderer, name, (3, 2, 2))
    for l_out, l_in in ((1.0, inf), (0.125, inf)):
        want, _, _ = assert_pruned(renderer, name, (3, 2, 2), l_out, l_in, capacities=(0,))
        assert len(want) >= 2
        assert_pruned(renderer, name, (3, 2, 2), l_out, l_in, capacities=(len(want), len(want) - 1, 1, 12))


@pytest.mark.parametrize("name", SCENES)
def test_tiny_and_ragged_lattices(renderer, name):
    for blocks in SMALL:
        want, cand, active = assert_pruned(renderer, name, blocks, 0.125, inf)
        assert_pruned(renderer, name, blocks, 1.0, inf)
        if name == "sphere" and blocks == (5, 4, 3):
            assert len(active) - len(want) == 4, "the spec predicts four lost blocks of the 5×4×3 sphere at an eighth of the bound"


def test_across_the_scans_boundary_and_more_than_1024_candidates(renderer):
    """11×10×10 = 1 100 blocks: two shares of 1024 flags in both compactions, lists on both sides of the boundary; and the 16³
    sponge, whose candidates fill more than one share of the candidate list."""
    for l_out, l_in in ((1.0, inf), (0.125, inf), (inf, inf)):
        want, cand, _ = assert_pruned(renderer, "menger", (11, 10, 10), l_out, l_in)
        lin = (want[:, 2] * 10 + want[:, 1]) * 11 + want[:, 0]
        assert (lin < 1024).any() and (lin >= 1024).any(), "the sponge reaches the lattice's last slab of blocks"
    assert cand == 1100
    _, cand, _ = assert_pruned(renderer, "menger", BIG, 1.0, inf)
    assert 1024 < cand < 4096


def test_two_streams(renderer):
    s1, s2 = torch.cuda.Stream(device=renderer.device), torch.cuda.Stream(device=renderer.device)
    dense_lattice(renderer, "primitives", BIG), dense_lattice(renderer, "bulb_moved", BIG)
    torch.cuda.synchronize(renderer.device)
    for _ in range(2):
        assert_pruned(renderer, "primitives", BIG, 1.0, inf, stream=s1)
        assert_pruned(renderer, "bulb_moved", BIG, 1.0, 1.0, stream=s2)
        assert_pruned(renderer, "primitives", (3, 2, 2), 0.125, inf, stream=s2)
        assert_pruned(renderer, "bulb_moved", (5, 4, 3), 1.0, inf, stream=s1)


def test_workspace_limit_refuses_cleanly_and_a_retry_succeeds(renderer):
    dist, origin, step, active = dense_lattice(renderer, "primitives", (11, 10, 10))
    want, cand = P.pruned_blocks(dist, step, 0.0, 1.0, inf, active)
    objs, no, g, s = V.scene("primitives")
    count = torch.zeros(2, dtype=torch.int32, device=renderer.device)
    call = lambda: lib().rm_sdf_blocks_select_pruned(objs, no, C.byref(g), C.byref(s), vec(origin), vec(step), 11, 10, 10, 0.0, 1.0, inf, 0, None,  # noqa: E731
                                                     ptr(count), renderer._stream())
    torch.cuda.synchronize(renderer.device)
    assert lib().rm_release_workspaces(None) == abi.RM_OK
    need = 4 * 12 * 11 * 11 + 8 * 1100 + 8 * 3  # 4 B per corner, 8 B per block, the scan's words of two shares
    assert lib().rm_set_workspace_limit(need - 1) == abi.RM_OK
    try:
        assert call() == abi.RM_ERR_DEVICE and "rm_set_workspace_limit" in lib().rm_last_error().decode()
        torch.cuda.synchronize(renderer.device)  # HIP's error state is clean
        assert count.tolist() == [0, 0], "a refused call wrote its count"
    finally:
        lib().rm_set_workspace_limit(0)
    assert call() == abi.RM_OK and count.tolist() == [len(want), cand]


# ---------------------------------------------------------------- the Python layer
def table_only(objs, no, g):
    return h.tables_of((abi.RmCamera(), objs, no, None, 0, g))


def test_sdf_active_blocks_pruned_against_sdf_active_blocks(renderer):
    dist, origin, step, active = dense_lattice(renderer, "julia", BIG)
    objs, no, g, s = V.scene("julia")
    t = table_only(objs, no, g)
    exhaustive = renderer.sdf_active_blocks(t, s, origin, step, BIG, 0.001).cpu().numpy()
    assert (exhaustive == active).all()
    bl, cand = renderer.sdf_active_blocks_pruned(t, s, origin, step, BIG, 0.001)  # the defaults: (4, None)
    assert (bl.cpu().numpy() == active).all() and cand == P.pruned_blocks(dist, step, 0.001, 4.0, inf, active)[1] < 4096
    bl, cand = renderer.sdf_active_blocks_pruned(t, s, origin, step, BIG, 0.001, outside=None, inside=None)
    assert (bl.cpu().numpy() == active).all() and cand == 4096
    bl, cand = renderer.sdf_active_blocks_pruned(t, s, origin, step, BIG, 0.001, 1.0, 1.0)
    want, wc = P.pruned_blocks(dist, step, 0.001, 1.0, 1.0, active)
    assert (bl.cpu().numpy() == want).all() and cand == wc and len(want) == len(active) - 4
    with pytest.raises(Exception, match="lipschitz"):
        renderer.sdf_active_blocks_pruned(t, s, origin, step, BIG, 0.001, outside=-1.0)


@pytest.mark.parametrize("name", ("sphere_cube", "bulb_plain"))
def test_scene_mesh_pruned_equals_scene_mesh_sparse_in_every_word(renderer, name):
    objs, no, g, s = V.scene(name)
    t = table_only(objs, no, g)
    sparse = renderer.scene_mesh_sparse(t, s, 129, 0.001)
    pruned = renderer.scene_mesh_pruned(t, s, 129, 0.001)
    assert len(sparse[0]) > 1000
    for a, b, what in zip(pruned, sparse, ("vertices", "quads", "vertex objects")):
        assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{name}: {what}"


def test_bake_mesh_pruned_equals_bake_mesh_sparse_in_every_word(renderer):
    objs, no, g, s = V.scene("sphere_cube")
    lights = (abi.RmLight * 1)(h.make_light(abi.RM_LIGHT_DIRECTIONAL, (1, 1, 1), (-0.3, -1, -0.5)))
    for i in range(no):
        for k in range(3):
            objs[i].cAmbient[k], objs[i].cDiffuse[k] = 0.3, 0.8
    t = h.tables_of((h.make_camera((0, 0, 5), (0, 0, -1), (0, 1, 0), 40.0, 8, 8), objs, no, lights, 1, g))
    sparse = renderer.bake_mesh_sparse(t, s, 20, 0.001)
    pruned = renderer.bake_mesh_pruned(t, s, 20, 0.001, outside=1.0, inside=1.0)
    assert len(sparse) == len(pruned) == 6 and len(sparse[0]) > 100
    for a, b in zip(pruned, sparse):
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def test_scene_field_pruned_traces_as_scene_field_sparse_does(renderer):
    objs, no, g, s = V.scene("bulb_plain")
    t = table_only(objs, no, g)
    sparse = renderer.scene_field_sparse(t, s, 129, 0.001)
    pruned = renderer.scene_field_pruned(t, s, 129, 0.001)
    for a, b in zip(pruned[:3], sparse[:3]):
        assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert tuple(pruned[3]) == tuple(sparse[3]) and (np.asarray(pruned[4]) == np.asarray(sparse[4])).all() and pruned[5] == sparse[5]
    rays = T.seeded_rays(np.random.default_rng(5), 600, radius=1.5)
    hits = []
    for dist, obj, bl, blocks, origin, step in (sparse, pruned):
        with renderer.lattice_field_blocks(dist, bl, blocks, origin, step, obj) as field:
            out = torch.empty((600, 8), dtype=torch.float32, device=renderer.device)
            field.trace(rays, out=out)
            torch.cuda.synchronize(renderer.device)
            hits.append(out.cpu().numpy())
    V.assert_bits(hits[1], hits[0], "the trace through the pruned field")
    assert (hits[0][:, 7].view(np.int32) >= 0).sum() > 50, "the rays meet the surface"
