"""rm_shade_points and rm_write_ply_ex without a GPU: the header declares them and the library exports them under the unchanged ABI
version, the comment carries the definition, every argument error returns its status, in the documented order, before the first HIP
call — with pointers that would fault if read — and rm_write_ply_ex, a host function, writes what a few lines of NumPy read back."""
import ctypes as C
import inspect
import re

import numpy as np

import abi_helpers as ah
import helpers as h
import scene_builders as SB
from abi_helpers import CAPACITY, FAKE, HEADER, HP, INT_MAX, INVALID, fake, refused
from abi_helpers import inf as INF
from raymarcher_amd import abi, lib, write_ply, write_ply_ex
from raymarcher_amd._lib import SIGNATURES
from scene_builders import three_primitives_lit as _scene

UNSUPPORTED = abi.RM_ERR_UNSUPPORTED


# ---------------------------------------------------------------- the symbols and the written definition
def test_header_declares_and_library_exports_the_symbols():
    assert ah.params("rm_shade_points") == [
        "const float *d_points", "const float *d_view", "int numPoints", "const RmPointsSettings *ps", "const RmObject *objs",
        "int numObjects", "const RmLight *lights", "int numLights", "const RmGlobals *g", "const RmSettings *s", "const RmResources *res",
        "RmSurfacePoint *d_surface", "float *d_ao", "float *d_rgba", "void *stream"]
    assert ah.params("rm_points_settings_default", "void") == ["RmPointsSettings *ps"]
    assert ah.params("rm_write_ply_ex") == [
        "const char *path", "const float *vertices4", "int numVertices", "const int32_t *quads4",
        "int numQuads", "const uint8_t *rgb", "const float *normals4"]
    ah.assert_exported(["rm_shade_points", "rm_points_settings_default", "rm_write_ply_ex"])
    for name in ("rm_shade_points", "rm_points_settings_default", "rm_write_ply_ex"):
        assert name in SIGNATURES, name
    assert len(SIGNATURES["rm_shade_points"][1]) == 15 and len(SIGNATURES["rm_write_ply_ex"][1]) == 7
    assert abi.RM_PATH_SHADE_POINTS == 17 and abi.RM_MAX_PROJECT_STEPS == 16
    assert re.search(r"#define\s+RM_MAX_PROJECT_STEPS\s+16\b", HEADER)
    ah.assert_abi_version()


def test_struct_sizes_and_layouts():
    assert C.sizeof(abi.RmSurfacePoint) == 32 == C.sizeof(abi.RmRayHit) and C.sizeof(abi.RmPointsSettings) == 16
    assert [(f, getattr(abi.RmSurfacePoint, f).offset) for f, _ in abi.RmSurfacePoint._fields_] == [
        ("normal", 0), ("distance", 12), ("position", 16), ("objectId", 28)]
    assert [(f, getattr(abi.RmPointsSettings, f).offset) for f, _ in abi.RmPointsSettings._fields_] == [
        ("far", 0), ("iso", 4), ("maxMove", 8), ("projectSteps", 12)]
    assert re.search(r"typedef struct RmSurfacePoint \{ float normal\[3\]; float distance; float position\[3\]; int32_t objectId; \}", HEADER)
    assert re.search(r"typedef struct RmPointsSettings \{ float far; float iso; float maxMove; int32_t projectSteps; \}", HEADER)


def test_points_settings_default():
    ps = abi.RmPointsSettings(-1.0, -1.0, -1.0, -1)
    lib().rm_points_settings_default(C.byref(ps))
    assert ps.far == 100.0 and ps.iso == np.float32(0.001) and ps.maxMove == INF and ps.projectSteps == 0
    lib().rm_points_settings_default(None)  # a null pointer is left alone


def test_header_comment_carries_the_definition():
    ah.assert_comment_has("RmSurfacePoint", (
        "bit for bit", "Invalid point", "RM_RAY_INVALID", "evaluates nothing", "cannot refuse them", "frag:1406-1430",
        "frag:1436-1444", "never bumped", "madd(N, −e, p)", "maxMove·maxMove", "keeps the last accepted p", "UB3",
        "frag:1679-1691", "frag:1729-1740", "whatever s->enableAmbientOcclusion says", "frag:2337-2375", "frag:1842-1933",
        "frag:2354-2365", "−N", "No reflection and no refraction", "1 + 4 evaluations", "5 per projection step",
        "does not depend on which points", "same bits whichever", "before any HIP call", "rm_debug_last_path() = 17",
        "symbol lookup"))
    assert re.search(r"17 = a launch of rm_shade_points", HEADER), "rm_debug_last_path's comment does not document 17"


def test_python_signatures():
    from raymarcher_amd.render import Renderer
    sig = inspect.signature(Renderer.shade_points)
    assert list(sig.parameters) == ["self", "tables", "settings", "points", "view", "far", "colour", "ao", "project", "iso", "max_move"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert d["view"] is None and d["far"] is None and d["colour"] is True and d["ao"] is False and d["project"] == 0
    assert d["iso"] == 0.001 and d["max_move"] == INF
    sig = inspect.signature(Renderer.bake_mesh)
    assert list(sig.parameters) == ["self", "tables", "settings", "resolution", "iso", "bounds", "project", "ao", "colour"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert d["iso"] == 0.001 and d["bounds"] is None and d["project"] == 2 and d["ao"] is True and d["colour"] is True
    assert list(inspect.signature(write_ply_ex).parameters) == ["path", "vertices", "quads", "colours", "normals"]
    assert list(inspect.signature(write_ply).parameters) == ["path", "vertices", "quads", "colours"], "write_ply keeps its signature"


# ---------------------------------------------------------------- refusals, all without a device
DEFAULT = object()


def call(objs, no, lights, nl, g, s=DEFAULT, n=100, ps=DEFAULT, res=None, points=FAKE, view=None, surface=None, ao=None, rgba=FAKE,
         **ps_over):
    s = abi.default_settings() if s is DEFAULT else s
    if ps is DEFAULT:
        ps = abi.RmPointsSettings()
        lib().rm_points_settings_default(C.byref(ps))
        for k, v in ps_over.items():
            setattr(ps, k, v)
    return lib().rm_shade_points(points, view, n, C.byref(ps) if ps is not None else None, objs, no, lights, nl,
                                 C.byref(g) if g is not None else None, C.byref(s) if s is not None else None,
                                 C.byref(res) if res is not None else None, surface, ao, rgba, None)


ARRAYS = "null d_points"  # the first check behind the scene's: a call that gets this far passed everything before it


def test_counts_and_scene_pointers():
    objs, no, lights, nl, g = _scene()
    assert refused(call(objs, no, lights, nl, g, n=-1), text="numPoints")
    assert refused(call(objs, no, lights, nl, g, n=-INT_MAX), text="numPoints")
    # numPoints == 0: RM_OK with null everything, nothing is read
    assert call(objs, no, lights, nl, g, n=0, points=None, rgba=None) == abi.RM_OK
    assert call(None, 5, None, -3, None, s=None, ps=None, n=0, points=None, rgba=None) == abi.RM_OK
    # every positive int fits one grid: INT_MAX points get as far as the scene pointers
    assert refused(call(objs, no, lights, nl, None, n=INT_MAX), text="null ps")
    assert refused(call(objs, no, lights, nl, g, ps=None), text="null ps")
    assert refused(call(objs, no, lights, nl, g, s=None), text="null ps")
    assert refused(call(None, no, lights, nl, g), text="null ps")
    assert refused(call(objs, no, None, nl, g), text="null ps")
    assert refused(call(objs, -1, lights, nl, g), text="null ps")
    assert refused(call(objs, no, lights, -1, g), text="null ps")
    # without d_rgba no light is read: a null light table passes, a negative count does not
    assert refused(call(objs, no, None, nl, g, rgba=None, surface=FAKE, points=None), text=ARRAYS)
    assert refused(call(objs, no, None, -1, g, rgba=None, surface=FAKE), text="null ps")
    # empty tables need no pointers
    assert refused(call(None, 0, None, 0, g, points=None), text=ARRAYS)


def test_point_settings_in_order():
    objs, no, lights, nl, g = _scene()
    for far in (float("nan"), -1.0, -1e-30, INF, -INF):
        assert refused(call(objs, no, lights, nl, g, far=far), text="far"), far
    for far in (0.0, -0.0, 1e-30, 3.0e38):
        assert refused(call(objs, no, lights, nl, g, far=far, points=None), text=ARRAYS), far
    for iso in (float("nan"), INF, -INF):
        assert refused(call(objs, no, lights, nl, g, iso=iso), text="iso"), iso
    for iso in (0.0, -0.5, 1e30):
        assert refused(call(objs, no, lights, nl, g, iso=iso, points=None), text=ARRAYS), iso
    for mm in (float("nan"), -1.0, -1e-30, -INF):
        assert refused(call(objs, no, lights, nl, g, maxMove=mm), text="maxMove"), mm
    for mm in (0.0, -0.0, 1e-30, INF):
        assert refused(call(objs, no, lights, nl, g, maxMove=mm, points=None), text=ARRAYS), mm
    for steps in (-1, abi.RM_MAX_PROJECT_STEPS + 1, INT_MAX):
        assert refused(call(objs, no, lights, nl, g, projectSteps=steps), text="projectSteps"), steps
    for steps in (0, 1, abi.RM_MAX_PROJECT_STEPS):
        assert refused(call(objs, no, lights, nl, g, projectSteps=steps, points=None), text=ARRAYS), steps
    assert refused(call(objs, no, lights, nl, g, rgba=None), text="all null")
    for out in ("surface", "ao", "rgba"):
        assert refused(call(objs, no, lights, nl, g, points=None, **{"rgba": None, out: FAKE}), text=ARRAYS), out
    # the order: the pointers, far, iso, maxMove, projectSteps, the outputs, then the layers
    bad = dict(far=-1.0, iso=INF, maxMove=-1.0, projectSteps=-1)
    sea = abi.default_settings(features=abi.RM_FEAT_SEA)
    assert refused(call(objs, no, lights, nl, None, rgba=None, s=sea, **bad), text="null ps")
    assert refused(call(objs, no, lights, nl, g, rgba=None, s=sea, **bad), text="far")
    del bad["far"]
    assert refused(call(objs, no, lights, nl, g, rgba=None, s=sea, **bad), text="iso")
    del bad["iso"]
    assert refused(call(objs, no, lights, nl, g, rgba=None, s=sea, **bad), text="maxMove")
    del bad["maxMove"]
    assert refused(call(objs, no, lights, nl, g, rgba=None, s=sea, **bad), text="projectSteps")
    assert refused(call(objs, no, lights, nl, g, rgba=None, s=sea), text="all null")
    assert refused(call(objs, no, lights, nl, g, s=sea), "TERRAIN / CLOUD / SEA", want=UNSUPPORTED)


def test_layers_capacity_loop_bounds_and_types_in_order():
    objs, no, lights, nl, g = _scene()
    for feat in (abi.RM_FEAT_TERRAIN, abi.RM_FEAT_CLOUD, abi.RM_FEAT_SEA, abi.RM_FEAT_TERRAIN | abi.RM_FEAT_PERLIN_BUMP):
        assert refused(call(objs, no, lights, nl, g, s=abi.default_settings(features=feat)), "TERRAIN / CLOUD / SEA", want=UNSUPPORTED), feat
    for feat in (0, abi.RM_FEAT_SKY_BACKGROUND, abi.RM_FEAT_DARK_BACKGROUND, abi.RM_FEAT_REFERENCE_DEFAULT):
        assert refused(call(objs, no, lights, nl, g, s=abi.default_settings(features=feat), points=None), text=ARRAYS), feat
    assert refused(call(objs, no, lights, nl, h.make_globals(two_d=1)), "isTwoD", want=UNSUPPORTED)
    many = (abi.RmObject * (abi.RM_MAX_OBJECTS + 1))(*[h.make_object(abi.RM_SPHERE) for _ in range(abi.RM_MAX_OBJECTS + 1)])
    lots = (abi.RmLight * (abi.RM_MAX_LIGHTS + 1))(*[h.make_light(abi.RM_LIGHT_POINT) for _ in range(abi.RM_MAX_LIGHTS + 1)])
    for outs in (dict(), dict(rgba=None, surface=FAKE), dict(rgba=None, ao=FAKE)):  # with and without the colour
        assert refused(call(many, abi.RM_MAX_OBJECTS + 1, lights, nl, g, **outs), "RM_MAX_OBJECTS", want=CAPACITY), outs
        assert refused(call(many, abi.RM_MAX_OBJECTS, lights, nl, g, points=None, **outs), text=ARRAYS), outs
        for field in ("maxSteps", "fractalIters", "mengerLevels"):
            assert refused(call(objs, no, lights, nl, g, s=abi.default_settings(**{field: -1}), **outs), text="loop bound"), field
        # the layers come before the capacity, the capacity before the loop bounds, the loop bounds before the types
        assert refused(call(many, abi.RM_MAX_OBJECTS + 1, lights, nl, g, s=abi.default_settings(features=abi.RM_FEAT_CLOUD), **outs),
                       "TERRAIN", want=UNSUPPORTED)
        assert refused(call(many, abi.RM_MAX_OBJECTS + 1, lights, nl, g, s=abi.default_settings(maxSteps=-1), **outs), want=CAPACITY)
        objs[1].type = abi.RM_CUSTOM
        assert refused(call(objs, no, lights, nl, g, s=abi.default_settings(maxSteps=-1), **outs), text="loop bound")
        assert refused(call(objs, no, lights, nl, g, **outs), "object 1", want=UNSUPPORTED)
        assert "CUSTOM" in lib().rm_last_error().decode()
        objs[1].type = abi.RM_CUBE
    # what only the colour reads is only checked with it: the light table's size and types, numReflection
    assert refused(call(objs, no, lots, abi.RM_MAX_LIGHTS + 1, g), "RM_MAX_LIGHTS", want=CAPACITY)
    assert refused(call(objs, no, lots, abi.RM_MAX_LIGHTS + 1, g, rgba=None, surface=FAKE, points=None), text=ARRAYS)
    assert refused(call(objs, no, lights, nl, g, s=abi.default_settings(numReflection=-1)), text="loop bound")
    lights[1].type = 7
    assert refused(call(objs, no, lights, nl, g), "light 1", want=UNSUPPORTED)
    assert refused(call(objs, no, lights, nl, g, rgba=None, ao=FAKE, points=None), text=ARRAYS)


def test_samplers_are_asked_for_only_with_the_colour():
    """Every sampler a feature, an object or a light reads must be supplied when d_rgba is: rm_render_res's statuses and texts.
    Without d_rgba no sampler is read and none is asked for.  Supplied pixel pointers are fake and never read."""
    objs, no, lights, nl, g = _scene()
    tex = abi.RmTexture(0x2000, 4, 4)
    night = abi.default_settings(features=abi.RM_FEAT_NIGHTSKY_BACKGROUND)
    assert refused(call(objs, no, lights, nl, g, s=night), "noise", want=UNSUPPORTED)
    assert refused(call(objs, no, lights, nl, g, s=night, rgba=None, surface=FAKE, points=None), text=ARRAYS)
    res = abi.RmResources()
    res.noise = tex
    assert refused(call(objs, no, lights, nl, g, s=night, res=res, points=None), text=ARRAYS)
    box = abi.default_settings(enableSkyBox=1)
    assert refused(call(objs, no, lights, nl, g, s=box), "enableSkyBox", want=UNSUPPORTED)
    assert refused(call(objs, no, lights, nl, g, s=box, rgba=None, ao=FAKE, points=None), text=ARRAYS)
    objs[0].texLoc = 0
    assert refused(call(objs, no, lights, nl, g), "texLoc", want=UNSUPPORTED)
    assert refused(call(objs, no, lights, nl, g, rgba=None, surface=FAKE, points=None), text=ARRAYS)
    res = abi.RmResources()
    arr = (abi.RmTexture * 1)(tex)
    res.textures, res.numTextures = arr, 1
    assert refused(call(objs, no, lights, nl, g, res=res, points=None), text=ARRAYS)
    objs[0].texLoc = -1
    res.numTextures = abi.RM_MAX_TEXTURES + 1
    assert refused(call(objs, no, lights, nl, g, res=res), "RM_MAX_TEXTURES", want=CAPACITY)
    scene = SB.area_light_scene(8, 8)
    assert refused(call(*scene[1:6]), "LTC", want=UNSUPPORTED)
    assert refused(call(*scene[1:6], rgba=None, surface=FAKE, points=None), text=ARRAYS)
    res = abi.RmResources()
    res.ltc1, res.ltc2 = 0x3000, 0x4000
    assert refused(call(*scene[1:6], res=res, points=None), text=ARRAYS)


def test_the_five_arrays():
    objs, no, lights, nl, g = _scene()
    assert refused(call(objs, no, lights, nl, g, points=None), text=ARRAYS)
    for off in (4, 8, 12, 1):
        bad = fake(0x1000 + off)
        for name in ("points", "view", "surface", "rgba"):
            assert refused(call(objs, no, lights, nl, g, **{name: bad}), text="16-byte aligned"), (name, off)
    for off in (1, 2, 3):
        assert refused(call(objs, no, lights, nl, g, ao=fake(0x1000 + off)), text="4-byte aligned"), off
    # the arrays come behind everything about the scene
    objs[0].type = abi.RM_CUSTOM
    assert refused(call(objs, no, lights, nl, g, points=None), "object 0", want=UNSUPPORTED)
    objs[0].type = abi.RM_SPHERE
    # host memory is not device memory: the only check that asks the HIP runtime, and the last
    assert refused(call(objs, no, lights, nl, g, points=HP, rgba=HP), text="d_points")


# ---------------------------------------------------------------- rm_write_ply_ex
def _mesh():
    rng = np.random.default_rng(2)
    v = rng.normal(size=(7, 4)).astype(np.float32)
    q = rng.integers(0, 7, (5, 4)).astype(np.int32)
    n = rng.normal(size=(7, 4)).astype(np.float32)
    c = rng.integers(0, 256, (7, 3)).astype(np.uint8)
    return v, q, n, c


def _read_ply(path):
    """A few lines of NumPy for what rm_write_ply_ex writes → (header lines, the vertex records, the face records)."""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    head = raw[:end].decode().splitlines()
    nv = int(next(ln for ln in head if ln.startswith("element vertex")).split()[-1])
    nq = int(next(ln for ln in head if ln.startswith("element face")).split()[-1])
    kinds = {"float": "<f4", "uchar": "u1"}
    props = [ln.split() for ln in head if ln.startswith("property") and "list" not in ln]
    vt = np.dtype([(p[2], kinds[p[1]]) for p in props])
    verts = np.frombuffer(raw, dtype=vt, count=nv, offset=end)
    faces = np.frombuffer(raw, dtype=np.dtype([("n", "u1"), ("i", "<i4", 4)]), count=nq, offset=end + nv * vt.itemsize)
    assert end + nv * vt.itemsize + nq * 17 == len(raw), "nothing behind the faces"
    return head, verts, faces


def _ply_ex(path, v, q, c, n):
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
    return lib().rm_write_ply_ex(str(path).encode(), p(v), len(v), p(q), len(q), p(c), p(n))


def test_write_ply_ex_reads_back(tmp_path):
    v, q, n, c = _mesh()
    for colours in (c, None):
        path = tmp_path / "m.ply"
        assert _ply_ex(path, v, q, colours, n) == abi.RM_OK
        head, verts, faces = _read_ply(path)
        names = ["x", "y", "z", "nx", "ny", "nz"] + (["red", "green", "blue"] if colours is not None else [])
        assert list(verts.dtype.names) == names, "the normals follow z, ahead of the colour"
        for k, name in enumerate(("x", "y", "z")):
            h.assert_bit_equal(verts[name], v[:, k], name)
            h.assert_bit_equal(verts["n" + name], n[:, k], "n" + name)
        if colours is not None:
            assert (np.stack([verts["red"], verts["green"], verts["blue"]], 1) == c).all()
        assert (faces["n"] == 4).all() and (faces["i"] == q).all()


def test_write_ply_ex_without_normals_is_write_ply_byte_for_byte(tmp_path):
    v, q, _, c = _mesh()
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
    for colours in (c, None):
        a, b = tmp_path / "a.ply", tmp_path / "b.ply"
        assert lib().rm_write_ply(str(a).encode(), p(v), len(v), p(q), len(q), p(colours)) == abi.RM_OK
        assert _ply_ex(b, v, q, colours, None) == abi.RM_OK
        assert open(a, "rb").read() == open(b, "rb").read()
    # and the Python layer: write_ply_ex without normals goes the old way, with normals of three or four floats the new one
    v3n = np.ascontiguousarray(_mesh()[2][:, :3])
    write_ply(tmp_path / "c.ply", v, q)
    assert open(tmp_path / "c.ply", "rb").read() == open(tmp_path / "a.ply", "rb").read()
    write_ply_ex(tmp_path / "d.ply", v, q, colours=c, normals=v3n)
    write_ply_ex(tmp_path / "e.ply", v, q)
    assert open(tmp_path / "e.ply", "rb").read() == open(tmp_path / "a.ply", "rb").read()
    _, verts, _ = _read_ply(tmp_path / "d.ply")
    h.assert_bit_equal(verts["ny"], v3n[:, 1], "ny through write_ply")


def test_write_ply_ex_refusals(tmp_path):
    v, q, n, c = _mesh()
    path = tmp_path / "never.ply"
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    L = lib()
    assert L.rm_write_ply_ex(None, p(v), 7, p(q), 5, None, p(n)) == INVALID
    assert L.rm_write_ply_ex(str(path).encode(), p(v), -1, p(q), 5, None, p(n)) == INVALID
    assert L.rm_write_ply_ex(str(path).encode(), None, 7, p(q), 5, None, p(n)) == INVALID
    q2 = q.copy()
    q2[3, 2] = 7
    assert L.rm_write_ply_ex(str(path).encode(), p(v), 7, p(q2), 5, None, p(n)) == INVALID and not path.exists()
    assert L.rm_write_ply_ex(str(tmp_path / "no" / "dir.ply").encode(), p(v), 7, p(q), 5, None, p(n)) == abi.RM_ERR_IO
    assert L.rm_write_ply_ex(str(path).encode(), None, 0, None, 0, None, None) == abi.RM_OK and path.exists()
