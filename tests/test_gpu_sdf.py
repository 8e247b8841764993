"""rm_sdf_grid and rm_sdf_mesh on the GPU, bit for bit: the lattice against the oracle's sdScene and against rm_probe_sdscene at the
same points, the mesh against the NumPy specification (tests/sdf_mesh_spec.py) — vertices, ids, quads and counts — with guard words
around every output; then the capacities, two streams, the workspace, and the Python layer."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import helpers as h
import sdf_helpers as V
import sdf_mesh_spec as S
from raymarcher_amd import abi, lib, mesh_bounds, write_ply
from raymarcher_amd.render import Scene

pytestmark = pytest.mark.gpu

# every brick of 4×4×4 (and of 8×8×1) partial along every axis; one point; a thin lattice; whole and partial bricks side by side
GRID_DIMS = ((5, 7, 9), (1, 1, 1), (1, 9, 4), (17, 16, 3))
GRID_SCENES = ("primitives", "menger", "sierpinski", "julia", "bulb_plain", "bulb_moved", "bulb_power6")


def vec(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def table_only(objs, no, g):
    """SceneTables of an object table alone: no camera, no lights."""
    return h.tables_of((abi.RmCamera(), objs, no, None, 0, g))


def grid_call(renderer, name, origin, step, dims, ids=True):
    """rm_sdf_grid into guarded, poisoned outputs → (dist, ids or None) as arrays; the guards and the coverage are checked."""
    objs, no, g, s = V.scene(name)
    nx, ny, nz = dims
    dist, check_d = h.guarded((nz, ny, nx), torch.float32, device=renderer.device)
    obj, check_i = h.guarded((nz, ny, nx), torch.int32, device=renderer.device) if ids else (None, None)
    st = lib().rm_sdf_grid(objs, no, C.byref(g), C.byref(s), vec(origin), vec(step), nx, ny, nz, ptr(dist), ptr(obj), renderer._stream())
    assert st == abi.RM_OK, lib().rm_last_error().decode()
    assert lib().rm_debug_last_path() == abi.RM_PATH_SDF_GRID == 16 and lib().rm_debug_last_split() == 0
    check_d()
    if ids:
        check_i()
    return dist.cpu().numpy(), (obj.cpu().numpy() if ids else None)


@pytest.mark.parametrize("name", GRID_SCENES)
def test_grid_equals_the_oracle_and_the_probe_in_every_bit(renderer, name):
    objs, no, g, s = V.scene(name)
    plain = lib().rm_debug_bulb_plain(objs, no, C.byref(g))
    assert plain == (1 if name == "bulb_plain" else 0)
    for dims in GRID_DIMS:
        ref_d, ref_i, origin, step = V.oracle_lattice(name, dims)
        got_d, got_i = grid_call(renderer, name, origin, step, dims)
        V.assert_bits(got_d, ref_d, f"{name} {dims}: d_dist against the oracle")
        assert (got_i == ref_i).all(), f"{name} {dims}: d_objectId against the oracle"
        pts = torch.from_numpy(S.lattice_points(origin, step, dims)).to(renderer.device)
        probe = renderer.probe_sdscene(table_only(objs, no, g), s, pts).cpu().numpy()
        nx, ny, nz = dims
        V.assert_bits(got_d, np.ascontiguousarray(probe[:, 0]).reshape(nz, ny, nx), f"{name} {dims}: d_dist against rm_probe_sdscene")
        assert (got_i == probe[:, 1].astype(np.int32).reshape(nz, ny, nx)).all(), f"{name} {dims}: ids against rm_probe_sdscene"
        alone, _ = grid_call(renderer, name, origin, step, dims, ids=False)
        V.assert_bits(alone, got_d, f"{name} {dims}: d_dist without d_objectId")
    ref_d, ref_i, _, _ = V.oracle_lattice(name, GRID_DIMS[0])
    assert ref_d.min() < 0.001 < ref_d.max(), "the lattice does not cross a surface"
    if name == "primitives":
        assert len(np.unique(ref_i)) >= 7, "the lattice sees too few of the primitives"


def test_grid_python_layer_and_timing(renderer):
    objs, no, g, s = V.scene("primitives")
    dims = (17, 16, 3)
    ref_d, ref_i, origin, step = V.oracle_lattice("primitives", dims)
    t = table_only(objs, no, g)
    dist, ids = renderer.sdf_grid(t, s, origin, step, dims, ids=True)
    assert tuple(dist.shape) == (3, 16, 17) and dist.dtype == torch.float32 and ids.dtype == torch.int32
    V.assert_bits(dist.cpu().numpy(), ref_d, "Renderer.sdf_grid")
    assert (ids.cpu().numpy() == ref_i).all()
    only = renderer.sdf_grid(t, s, origin, step, dims)
    assert torch.equal(only, dist)
    lib().rm_set_timing(1)
    try:
        renderer.sdf_grid(t, s, origin, step, dims)
        torch.cuda.synchronize()
        total, stages, n = C.c_double(), (C.c_double * 4)(), C.c_int()
        assert lib().rm_get_stage_timing(C.byref(total), stages, C.byref(n)) == abi.RM_OK
        assert n.value == 1 and stages[0] == 0.0 and stages[1] == total.value > 0.0
    finally:
        lib().rm_set_timing(0)


# ---------------------------------------------------------------- rm_sdf_mesh
def mesh_call(renderer, dist, ids, origin, step, iso, max_v, max_q, want_vobj=True, stream=None):
    """rm_sdf_mesh on a host lattice into guarded outputs of exactly the capacities → (counts, vertices, vertex ids, quads)."""
    dev = renderer.device
    nz, ny, nx = dist.shape
    d = torch.from_numpy(np.array(dist, dtype=np.float32)).to(dev)
    i = torch.from_numpy(np.array(ids, dtype=np.int32)).to(dev) if ids is not None else None
    counts, check_c = h.guarded((1, 2), torch.int32, device=dev)
    v, check_v = h.guarded((max_v, 4), torch.float32, device=dev) if max_v else (None, None)
    vo, check_o = h.guarded((1, max_v), torch.int32, device=dev) if max_v and want_vobj else (None, None)
    q, check_q = h.guarded((max_q, 4), torch.int32, device=dev) if max_q else (None, None)
    path_before = lib().rm_debug_last_path()
    st = lib().rm_sdf_mesh(ptr(d), ptr(i), nx, ny, nz, vec(origin), vec(step), float(iso), max_v, max_q, ptr(v), ptr(vo), ptr(q), ptr(counts),
                           C.c_void_p(stream.cuda_stream) if stream is not None else renderer._stream())
    assert st == abi.RM_OK, lib().rm_last_error().decode()
    if stream is not None:
        stream.synchronize()
    assert lib().rm_debug_last_path() == path_before, "rm_sdf_mesh is not a render launch"
    for check in (check_c, check_v, check_o, check_q):
        if check:
            check()
    host = lambda t, shape, dt: t.cpu().numpy().reshape(shape) if t is not None else np.zeros(shape, dt)  # noqa: E731
    return (tuple(int(x) for x in counts.cpu().numpy().view(np.uint32).reshape(-1)), host(v, (max_v, 4), np.float32),
            host(vo, (max_v,), np.int32), host(q, (max_q, 4), np.int32))


def assert_mesh(renderer, dist, ids, origin, step, iso, what):
    """The counting call, exact capacities and capacities one below the counts, all against the specification."""
    want = S.surface_nets(dist, origin, step, iso, ids)
    nv, nq = len(want["vertices"]), len(want["quads"])
    counts, _, _, _ = mesh_call(renderer, dist, ids, origin, step, iso, 0, 0)
    assert counts == (nv, nq), f"{what}: the counting call"
    if nv == 0:
        return want
    for mv, mq in ((nv, nq), (nv - 1, max(nq - 1, 0))):
        counts, v, vo, q = mesh_call(renderer, dist, ids, origin, step, iso, mv, mq)
        assert counts == (nv, nq), f"{what}: counts with capacities {mv}, {mq}"
        V.assert_bits(v, want["vertices"][:mv], f"{what}: vertices, capacity {mv}")
        assert (vo == want["vertex_object"][:mv]).all(), f"{what}: vertex ids, capacity {mv}"
        assert (q == want["quads"][:mq]).all(), f"{what}: quads, capacity {mq}"
    return want


@pytest.mark.parametrize("name,dims,iso", [("sphere", (12, 12, 12), 0.0), ("sphere_cube", (21, 11, 11), 0.0), ("sphere", (12, 12, 12), 0.07),
                                           ("bulb_plain", (24, 24, 24), 0.001), ("sphere", (33, 35, 70), 0.0)])
def test_mesh_of_oracle_lattices_equals_the_spec(renderer, name, dims, iso):
    dist, ids, origin, step = V.oracle_lattice(name, dims)
    want = assert_mesh(renderer, dist, ids, origin, step, iso, f"{name} {dims} iso {iso}")
    assert len(want["vertices"]) > 50
    if dims == (33, 35, 70):
        # 80850 points are 79 workgroups' shares of 1024: the offsets carry across workgroups, and vertices lie in many shares
        cell = (want["cells"][:, 2] * 35 + want["cells"][:, 1]) * 33 + want["cells"][:, 0]
        assert len(np.unique(cell // 1024)) > 20
    if name == "bulb_plain":
        assert (dist < iso).sum() > 100, "the lattice holds too few points inside the bulb"


def test_mesh_of_more_than_1024_shares_carries_the_scan_into_its_second_round(renderer):
    """mesh_scan_kernel scans 1024 shares per round and carries both totals into the next.  128 × 128 × 72 points are 1152 shares of
    1024: a sphere of radius 0.55 around the middle of the box has active cells on both sides of share 1024, so the vertices and
    quads numbered behind it are right only with the carry."""
    nx, ny, nz = 128, 128, 72
    origin, step = np.array([-1.0, -1.0, -0.5], np.float32), np.array([2 / 127, 2 / 127, 1 / 71], np.float32)
    x, y, z = (origin[a] + np.arange(n, dtype=np.float32) * step[a] for a, n in enumerate((nx, ny, nz)))
    dist = np.sqrt(z[:, None, None] ** 2 + y[None, :, None] ** 2 + x[None, None, :] ** 2) - np.float32(0.55)
    assert dist.dtype == np.float32 and dist.shape == (nz, ny, nx) and dist.size == 1152 * 1024
    ids = (np.arange(dist.size, dtype=np.int32) % 7).reshape(dist.shape)
    want = assert_mesh(renderer, dist, ids, origin, step, 0.0, "128 × 128 × 72 sphere")
    assert (len(want["vertices"]), len(want["quads"])) == (22976, 22856)
    share = ((want["cells"][:, 2] * ny + want["cells"][:, 1]) * nx + want["cells"][:, 0]) // 1024
    assert ((share < 1024).sum(), (share >= 1024).sum()) == (20736, 2240), "active cells on both sides of the scan's second round"


@pytest.mark.parametrize("name", sorted(V.handmade()))
def test_mesh_of_handmade_lattices_equals_the_spec(renderer, name):
    dist, ids, origin, step, iso = V.handmade()[name]
    want = assert_mesh(renderer, dist, ids, origin, step, iso, name)
    if name.startswith("all_"):
        assert len(want["vertices"]) == 0 and len(want["quads"]) == 0
    if ids is not None and len(want["vertices"]):
        _, _, vo, _ = mesh_call(renderer, dist, None, origin, step, iso, len(want["vertices"]), 0)
        assert (vo == -1).all(), "d_vertexObject without d_objectId is −1"
        mesh_call(renderer, dist, ids, origin, step, iso, len(want["vertices"]), len(want["quads"]), want_vobj=False)


def test_mesh_of_a_lattice_with_a_dimension_of_one_is_empty(renderer):
    for dims in ((1, 6, 5), (6, 1, 5), (6, 5, 1), (1, 1, 1)):
        nx, ny, nz = dims
        dist = np.full((nz, ny, nx), -1.0, np.float32)
        dist[::2] = 1.0
        counts, _, _, _ = mesh_call(renderer, dist, None, (0, 0, 0), (1, 1, 1), 0.0, 0, 0)
        assert counts == (0, 0), dims
        # capacities it has no use for: the counts are stored, the arrays stay as they were
        d = torch.from_numpy(dist).to(renderer.device)
        v, q = torch.full((3, 4), 7.0, device=renderer.device), torch.full((2, 4), 7, dtype=torch.int32, device=renderer.device)
        counts = torch.full((2,), 7, dtype=torch.int32, device=renderer.device)
        st = lib().rm_sdf_mesh(ptr(d), None, nx, ny, nz, vec((0, 0, 0)), vec((1, 1, 1)), 0.0, 3, 2, ptr(v), None, ptr(q), ptr(counts),
                               renderer._stream())
        assert st == abi.RM_OK and counts.tolist() == [0, 0] and bool((v == 7).all()) and bool((q == 7).all()), dims


def test_two_streams_give_identical_meshes_and_the_workspace_is_released(renderer):
    dist, ids, origin, step = V.oracle_lattice("sphere_cube", (21, 11, 11))
    want = S.surface_nets(dist, origin, step, 0.0, ids)
    nv, nq = len(want["vertices"]), len(want["quads"])
    s1, s2 = torch.cuda.Stream(device=renderer.device), torch.cuda.Stream(device=renderer.device)
    a = mesh_call(renderer, dist, ids, origin, step, 0.0, nv, nq, stream=s1)
    b = mesh_call(renderer, dist, ids, origin, step, 0.0, nv, nq, stream=s2)
    assert a[0] == b[0] == (nv, nq)
    for x, y, w in zip(a[1:], b[1:], (want["vertices"], want["vertex_object"], want["quads"])):
        assert x.tobytes() == y.tobytes() == w.tobytes()
    freed = C.c_ulonglong(0)
    assert lib().rm_release_workspaces(C.byref(freed)) == abi.RM_OK
    assert freed.value > 0
    # a lattice over a set workspace limit is refused with RM_ERR_DEVICE, and served again once the limit is lifted
    assert lib().rm_set_workspace_limit(64) == abi.RM_OK
    try:
        d = torch.from_numpy(np.array(dist, dtype=np.float32)).to(renderer.device)
        counts = torch.zeros(2, dtype=torch.int32, device=renderer.device)
        st = lib().rm_sdf_mesh(ptr(d), None, 21, 11, 11, vec(origin), vec(step), 0.0, 0, 0, None, None, None, ptr(counts), renderer._stream())
        assert st == abi.RM_ERR_DEVICE and "rm_set_workspace_limit" in lib().rm_last_error().decode()
    finally:
        lib().rm_set_workspace_limit(0)
    assert mesh_call(renderer, dist, ids, origin, step, 0.0, 0, 0)[0] == (nv, nq)


# ---------------------------------------------------------------- the Python layer
def test_extract_mesh_equals_the_two_c_calls(renderer):
    objs, no, g, s = V.scene("sphere_cube")
    dims = (21, 11, 11)
    ref_d, ref_i, origin, step = V.oracle_lattice("sphere_cube", dims)
    t = table_only(objs, no, g)
    dist, ids = renderer.sdf_grid(t, s, origin, step, dims, ids=True)
    v, q, vo = renderer.extract_mesh(dist, origin, step, 0.0, ids)
    want = S.surface_nets(ref_d, origin, step, 0.0, ref_i)
    counts, cv, cvo, cq = mesh_call(renderer, ref_d, ref_i, origin, step, 0.0, len(want["vertices"]), len(want["quads"]))
    V.assert_bits(v.cpu().numpy(), cv, "extract_mesh: vertices")
    assert (vo.cpu().numpy() == cvo).all() and (q.cpu().numpy() == cq).all()
    assert counts == (len(v), len(q))
    v2, q2 = renderer.extract_mesh(dist, origin, step)
    assert torch.equal(v2, v) and torch.equal(q2, q)
    empty = renderer.extract_mesh(torch.ones_like(dist), origin, step)
    assert tuple(empty[0].shape) == (0, 4) and tuple(empty[1].shape) == (0, 4)


def _scene_distance(t, s, pts):
    out = np.empty((len(pts), 4), np.float32)
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    assert h.oracle().rmo_probe_sdscene(t.objects, t.num_objects, C.byref(t.globals_), C.byref(s), h.fptr(pts), h.fptr(out), len(pts)) == 0
    return out[:, 0].astype(np.float64)


def test_scene_mesh_of_a_scenefile_round_trips_through_write_ply(renderer, tmp_path):
    """recursive_sphere_2.json: a sphere of radius 3 with six of radius 1.5 on it, one closed surface.  A vertex shares its cell with
    a point of the surface {d = 0.001} and a union of spheres' distance changes by at most 1 per unit length, so the oracle's
    distance at a vertex is within a cell's diagonal of 0.001."""
    t = Scene(path=os.path.join(h.ROOT, "tests", "golden", "scenes", "simple", "recursive_sphere_2.json")).tables(64, 36)
    s = abi.default_settings()
    assert t.num_objects == 7
    v, q, vo = (x.cpu().numpy() for x in renderer.scene_mesh(t, s, 24))
    assert len(v) > 500 and set(np.unique(vo)) == set(range(7))
    edges = V.assert_closed_oriented(q, "recursive_sphere_2.json")
    assert len(v) - edges + len(q) == 2 and V.signed_volume(v, q) > 0
    lo, hi = mesh_bounds(t)
    step = float((hi - lo).max()) / (24 - 3)
    assert np.abs(_scene_distance(t, s, v[:, :3]) - 0.001).max() < step * np.sqrt(3.0)
    colours = np.clip(v[:, :3] * 20 + 128, 0, 255).astype(np.uint8)
    path = write_ply(tmp_path / "spheres.ply", v, q, colours)
    gv, gc, gq = V.read_ply(path)
    V.assert_bits(gv, np.ascontiguousarray(v[:, :3]), "PLY vertices")
    assert (gq == q).all() and (gc == colours).all()
    # the caller's bounds: the top sphere alone (centre (0, 4.5, 0), radius 1.5) is cut open where it joins the large one
    v2, q2, vo2 = (x.cpu().numpy() for x in renderer.scene_mesh(t, s, 16, bounds=((-1.6, 3.2, -1.6), (1.6, 6.1, 1.6))))
    assert len(v2) > 50 and V.signed_volume(v2, q2) != 0 and v2[:, 1].min() > 2.9
    with pytest.raises(ValueError):
        renderer.scene_mesh(t, s, 3)
