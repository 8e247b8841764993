"""rm_sdf_grid, rm_sdf_mesh and rm_write_ply without a GPU: the header declares them and the library exports them under the unchanged
ABI version, every refusal returns its status before the first HIP call — with pointers that would fault if read — in the order the
header states, and rm_write_ply, a host function, writes what a few lines of Python read back."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

import abi_helpers as ah
import helpers as h
import scene_builders as SB
import sdf_helpers as V
from abi_helpers import BAD_ORIGINS, BAD_STEPS, CAPACITY, FAKE, HEADER, HP, inf, nan, refused, vec3
from raymarcher_amd import abi, lib
from raymarcher_amd._lib import SIGNATURES

UNSUPPORTED, IO = abi.RM_ERR_UNSUPPORTED, abi.RM_ERR_IO


# ---------------------------------------------------------------- the ABI surface
def test_header_declares_and_library_exports_the_three_symbols():
    assert ah.params("rm_sdf_grid") == [
        "const RmObject *objs", "int numObjects", "const RmGlobals *g", "const RmSettings *s",
        "const float origin[3]", "const float step[3]", "int nx", "int ny", "int nz", "float *d_dist",
        "int32_t *d_objectId", "void *stream"]
    assert ah.params("rm_sdf_mesh") == [
        "const float *d_dist", "const int32_t *d_objectId", "int nx", "int ny", "int nz",
        "const float origin[3]", "const float step[3]", "float iso", "int maxVertices", "int maxQuads",
        "float *d_vertices", "int32_t *d_vertexObject", "int32_t *d_quads", "uint32_t *d_counts",
        "void *stream"]
    assert ah.params("rm_write_ply") == [
        "const char *path", "const float *vertices4", "int numVertices", "const int32_t *quads4",
        "int numQuads", "const uint8_t *rgb"]
    ah.assert_exported(["rm_sdf_grid", "rm_sdf_mesh", "rm_write_ply"])
    for name in ("rm_sdf_grid", "rm_sdf_mesh", "rm_write_ply"):
        assert name in SIGNATURES and SIGNATURES[name][0] is C.c_int
    assert len(SIGNATURES["rm_sdf_grid"][1]) == 12 and len(SIGNATURES["rm_sdf_mesh"][1]) == 15 and len(SIGNATURES["rm_write_ply"][1]) == 6


def test_abi_version_stays_and_the_header_carries_the_definitions():
    ah.assert_abi_version()
    assert re.search(r"#define\s+RM_MAX_LATTICE_DIM\s+4096\b", HEADER) and abi.RM_MAX_LATTICE_DIM == 4096 and abi.RM_PATH_SDF_GRID == 16
    assert re.search(r"16 = a launch of rm_sdf_grid", HEADER), "rm_debug_last_path's comment does not document 16"
    for name, words in (("rm_sdf_grid", ("never fused", "frag:1406-1430", "rm_probe_sdscene", "a 64-bit index", "before any HIP call",
                                         "rm_debug_last_path() = 16", "4×4×4", "does not depend on which other points", "symbol lookup")),
                        ("rm_sdf_mesh", ("inside(v) = v < iso", "a NaN is outside", "t = 0.5f unless (t >= 0 && t <= 1)", "(c0, c3, c2, c1)",
                                         "first inside corner", "the counting call", "FULL number", "before any HIP call",
                                         "rm_set_workspace_limit", "rm_release_workspaces"))):
        ah.assert_comment_has(name, words)


def test_python_signatures():
    import raymarcher_amd
    from raymarcher_amd.render import Renderer, mesh_bounds, write_ply
    assert list(inspect.signature(Renderer.sdf_grid).parameters) == ["self", "tables", "settings", "origin", "step", "dims", "ids"]
    sig = inspect.signature(Renderer.extract_mesh)
    assert list(sig.parameters) == ["self", "grid", "origin", "step", "iso", "ids"] and sig.parameters["iso"].default == 0.0
    sig = inspect.signature(Renderer.scene_mesh)
    assert list(sig.parameters) == ["self", "tables", "settings", "resolution", "iso", "bounds"] and sig.parameters["iso"].default == 0.001
    assert list(inspect.signature(mesh_bounds).parameters) == ["tables", "margin"]
    assert list(inspect.signature(write_ply).parameters) == ["path", "vertices", "quads", "colours"]
    assert raymarcher_amd.mesh_bounds is mesh_bounds and raymarcher_amd.write_ply is write_ply


def test_mesh_bounds_hold_the_surface_or_raise():
    from raymarcher_amd import mesh_bounds
    from raymarcher_amd.render import SceneTables
    for name in ("sphere", "sphere_cube", "primitives", "bulb_plain", "menger"):
        objs, no, g, s = V.scene(name)
        t = SceneTables(abi.RmCamera(), objs, no, None, 0, g)
        lo, hi = mesh_bounds(t)
        assert lo.dtype == np.float32 and lo.shape == hi.shape == (3,) and (lo < hi).all()
        # the oracle's sdScene on a shell just outside the bounds is above the hit threshold: no surface out there
        rng = np.random.default_rng(3)
        pts = rng.uniform(-1, 1, (400, 3))
        pts /= np.abs(pts).max(axis=1, keepdims=True)  # on the surface of the cube [−1, 1]³
        pts = ((lo + hi) / 2 + pts * (hi - lo) / 2 * 1.0001).astype(np.float32)
        out = np.empty((len(pts), 4), np.float32)
        assert h.oracle().rmo_probe_sdscene(objs, no, C.byref(g), C.byref(s), h.fptr(pts), h.fptr(out), len(pts)) == 0
        assert (out[:, 0] > 0.001).all(), name
        wide_lo, wide_hi = mesh_bounds(t, 0.25)
        assert np.allclose(wide_lo, lo - 0.25) and np.allclose(wide_hi, hi + 0.25)
    for name in ("sierpinski",):
        objs, no, g, s = V.scene(name)
        with pytest.raises(ValueError):
            mesh_bounds(SceneTables(abi.RmCamera(), objs, no, None, 0, g))
    with pytest.raises(ValueError):
        mesh_bounds(SceneTables(abi.RmCamera(), None, 0, None, 0, h.make_globals()))


# ---------------------------------------------------------------- rm_sdf_grid's refusals, in the header's order
def grid(objs, no, g, s="default", origin=(0, 0, 0), step=(0.1, 0.1, 0.1), dims=(8, 8, 8), dist=FAKE, ids=FAKE):
    s = abi.default_settings() if s == "default" else s
    return lib().rm_sdf_grid(objs, no, C.byref(g) if g is not None else None, C.byref(s) if s is not None else None,
                             vec3(origin), vec3(step),
                             dims[0], dims[1], dims[2], dist, ids, None)


# a baked lattice may have a dimension of 1: these differ from the sampled lattices' shared table
BAD_DIMS = ((0, 8, 8), (8, -1, 8), (8, 8, 0), (4097, 1, 1), (1, 4097, 1), (1, 1, 2 ** 31 - 1), (-2 ** 31, 8, 8))
TOO_MANY = ((2048, 2048, 512), (4096, 4096, 128), (4096, 4096, 4096), (1291, 1291, 1291))  # 2^31 points and more


def test_grid_pointers_and_lattice():
    objs, no, g = SB.three_primitives_table()
    assert refused(grid(objs, no, None), text="null g, s, origin or step")
    assert refused(grid(objs, no, g, s=None), text="null g, s, origin or step")
    assert refused(grid(objs, no, g, origin=None), text="null g, s, origin or step")
    assert refused(grid(objs, no, g, step=None), text="null g, s, origin or step")
    assert refused(grid(None, no, g), text="null object table")
    assert refused(grid(objs, -1, g), text="null object table")
    assert refused(grid(None, no, None), text="null g, s")  # the pointers come before the table
    for o in BAD_ORIGINS:
        assert refused(grid(objs, no, g, origin=o), text="origin must be finite"), o
        assert refused(grid(None, no, g, origin=o), text="null object table"), o  # the table comes before the lattice
    for st in BAD_STEPS:
        assert refused(grid(objs, no, g, step=st), text="step must be finite and greater than 0"), st
        assert refused(grid(objs, no, g, origin=(nan, 0, 0), step=st), text="origin"), st
    for d in BAD_DIMS:
        assert refused(grid(objs, no, g, dims=d), text="lattice dimension"), d
        assert refused(grid(objs, no, g, step=(0, 1, 1), dims=d), text="step"), d
    for d in TOO_MANY:
        assert refused(grid(objs, no, g, dims=d), text="INT_MAX"), d
    # just under 2^31 points and the largest single dimensions are lattices: they get as far as the output
    for d in ((4096, 4096, 127), (1, 1, 1), (4096, 1, 1), (1, 1, 4096), (2048, 2048, 511)):
        assert refused(grid(objs, no, g, dims=d, dist=None), text="null d_dist"), d


def test_grid_unsupported_table_and_outputs():
    objs, no, g = SB.three_primitives_table()
    for feat in (abi.RM_FEAT_TERRAIN, abi.RM_FEAT_CLOUD, abi.RM_FEAT_SEA, abi.RM_FEAT_SEA | abi.RM_FEAT_PERLIN_BUMP):
        assert refused(grid(objs, no, g, s=abi.default_settings(features=feat)), "TERRAIN / CLOUD / SEA", want=UNSUPPORTED), feat
        # the lattice comes before the layers, the layers before the 2-D mode
        assert refused(grid(objs, no, g, s=abi.default_settings(features=feat), dims=(0, 1, 1)), text="lattice dimension"), feat
        assert refused(grid(objs, no, h.make_globals(two_d=1), s=abi.default_settings(features=feat)), "TERRAIN", want=UNSUPPORTED), feat
    assert refused(grid(objs, no, h.make_globals(two_d=1)), "isTwoD", want=UNSUPPORTED)
    many, nm = h.table([h.make_object(abi.RM_SPHERE) for _ in range(abi.RM_MAX_OBJECTS + 1)])
    assert refused(grid(many, nm, g), "RM_MAX_OBJECTS", want=CAPACITY)
    assert refused(grid(many, nm, h.make_globals(two_d=1)), "isTwoD", want=UNSUPPORTED)  # the 2-D mode comes before the table
    assert refused(grid(many, nm, g, dist=None), "RM_MAX_OBJECTS", want=CAPACITY)        # and the table before the output
    assert refused(grid(many, abi.RM_MAX_OBJECTS, g, dist=None), text="null d_dist")
    for field in ("fractalIters", "mengerLevels", "maxSteps"):
        assert refused(grid(objs, no, g, s=abi.default_settings(**{field: -1})), text="loop bound"), field
    objs[1].type = abi.RM_CUSTOM
    assert refused(grid(objs, no, g), "object 1", want=UNSUPPORTED) and "CUSTOM" in lib().rm_last_error().decode()
    objs[1].type = 99
    assert refused(grid(objs, no, g, dist=None), "object 1", want=UNSUPPORTED)
    objs[1].type = abi.RM_CUBE
    assert refused(grid(objs, no, g, dist=None), text="null d_dist")
    assert refused(grid(None, 0, g, dist=None), text="null d_dist")  # an empty table needs no pointer
    # host memory is not device memory: the only check that asks the HIP runtime
    assert refused(grid(objs, no, g, dist=HP, ids=None), text="d_dist")
    assert refused(grid(objs, no, g, dist=HP, ids=HP), text="is not device-accessible")


# ---------------------------------------------------------------- rm_sdf_mesh's refusals, in the header's order
def mesh(dims=(8, 8, 8), origin=(0, 0, 0), step=(0.1, 0.1, 0.1), iso=0.0, max_v=10, max_q=10, dist=FAKE, ids=FAKE, verts=FAKE, vobj=FAKE,
         quads=FAKE, counts=FAKE):
    return lib().rm_sdf_mesh(dist, ids, dims[0], dims[1], dims[2], vec3(origin), vec3(step), iso, max_v, max_q, verts, vobj, quads, counts, None)


def test_mesh_refusals_in_order():
    assert refused(mesh(origin=None), text="null origin or step")
    assert refused(mesh(step=None), text="null origin or step")
    for o in BAD_ORIGINS:
        assert refused(mesh(origin=o), text="origin must be finite"), o
    for st in BAD_STEPS:
        assert refused(mesh(step=st), text="step must be finite and greater than 0"), st
        assert refused(mesh(origin=(0, nan, 0), step=st), text="origin"), st
    for d in BAD_DIMS:
        assert refused(mesh(dims=d), text="lattice dimension"), d
        assert refused(mesh(dims=d, step=(1, 1, nan)), text="step"), d
    for d in TOO_MANY:
        assert refused(mesh(dims=d), text="INT_MAX"), d
    for iso in (nan, inf, -inf):
        assert refused(mesh(iso=iso), text="iso must be finite"), iso
        assert refused(mesh(iso=iso, dims=(0, 1, 1)), text="lattice dimension"), iso  # the lattice comes before iso
        assert refused(mesh(iso=iso, max_v=-1), text="iso"), iso                      # iso before the capacities
    assert refused(mesh(max_v=-1), text="negative capacity")
    assert refused(mesh(max_q=-5), text="negative capacity")
    assert refused(mesh(max_q=-2 ** 31, verts=None), text="negative capacity")        # the capacities before the outputs
    assert refused(mesh(verts=None), text="null d_vertices or d_quads")
    assert refused(mesh(quads=None), text="null d_vertices or d_quads")
    assert refused(mesh(verts=None, dist=None), text="null d_vertices or d_quads")     # the outputs before d_dist and d_counts
    assert refused(mesh(dist=None), text="null d_dist or d_counts")
    assert refused(mesh(counts=None), text="null d_dist or d_counts")
    # the counting call takes null outputs, a capacity of 0 takes a null array, d_vertexObject and d_objectId may be null: each of
    # these gets as far as the device-memory check of an array that is host memory
    assert refused(mesh(max_v=0, max_q=0, verts=None, vobj=None, quads=None, ids=None, dist=HP), text="d_dist is not device-accessible")
    assert refused(mesh(max_v=0, verts=None, vobj=None, ids=None, dist=HP), text="d_dist is not device-accessible")
    assert refused(mesh(max_q=0, quads=None, dist=HP), text="d_dist is not device-accessible")
    # a lattice with a dimension of 1 is a lattice: it is checked like any other
    assert refused(mesh(dims=(1, 8, 8), dist=None), text="null d_dist or d_counts")
    assert refused(mesh(dims=(8, 1, 8), dist=HP, max_v=0, max_q=0, verts=None, quads=None), text="d_dist is not device-accessible")


# ---------------------------------------------------------------- rm_write_ply
def _write(path, v, q, rgb=None, nv=None, nq=None):
    p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None  # noqa: E731
    return lib().rm_write_ply(str(path).encode() if path is not None else None, p(v), len(v) if nv is None else nv, p(q),
                              len(q) if nq is None else nq, p(rgb))


def test_write_ply_round_trip(tmp_path):
    rng = np.random.default_rng(5)
    v = rng.normal(size=(37, 4)).astype(np.float32)
    v[3, 0], v[4, 1], v[5, 2] = np.float32(-0.0), np.float32(1e-42), np.float32(3e38)
    q = rng.integers(0, 37, (53, 4)).astype(np.int32)
    rgb = rng.integers(0, 256, (37, 3)).astype(np.uint8)
    for colours in (None, rgb):
        path = tmp_path / ("c.ply" if colours is not None else "p.ply")
        assert _write(path, v, q, colours) == abi.RM_OK
        gv, gc, gq = V.read_ply(path)
        V.assert_bits(gv, v[:, :3], "vertices")
        assert (gq == q).all() and gq.dtype == np.int32
        assert (gc is None) if colours is None else (gc == rgb).all()
    # the Python wrapper writes the same bytes; an empty mesh is a file with two empty elements
    from raymarcher_amd import write_ply
    write_ply(tmp_path / "w.ply", v, q, rgb)
    assert open(tmp_path / "w.ply", "rb").read() == open(tmp_path / "c.ply", "rb").read()
    assert _write(tmp_path / "e.ply", None, None, nv=0, nq=0) == abi.RM_OK
    gv, gc, gq = V.read_ply(tmp_path / "e.ply")
    assert gv.shape == (0, 3) and gq.shape == (0, 4)


def test_write_ply_refusals(tmp_path):
    v = np.zeros((4, 4), np.float32)
    q = np.array([[0, 1, 2, 3]], np.int32)
    ok = tmp_path / "ok.ply"
    assert refused(_write(None, v, q), text="bad ply arguments")
    assert refused(_write(ok, None, q, nv=4), text="bad ply arguments")
    assert refused(_write(ok, v, None, nq=1), text="bad ply arguments")
    assert refused(_write(ok, v, q, nv=-1), text="bad ply arguments")
    assert refused(_write(ok, v, q, nq=-1), text="bad ply arguments")
    for bad in (4, -1, 2 ** 31 - 1):
        q2 = q.copy()
        q2[0, 2] = bad
        assert refused(_write(ok, v, q2), text="names a vertex outside"), bad
    assert not ok.exists(), "a refused call created the file"
    assert refused(_write(tmp_path / "no_such_directory" / "m.ply", v, q), "cannot open", want=IO)
    assert refused(_write(tmp_path, v, q), "cannot open", want=IO)  # a directory
    with pytest.raises(Exception):
        from raymarcher_amd import write_ply
        write_ply(ok, v, q, np.zeros((3, 3), np.uint8))
