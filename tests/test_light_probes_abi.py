"""rm_light_probes and rm_sphere_directions without a GPU: the header declares them and the library exports them under the unchanged
ABI version, the structs have 64 and 160 bytes, every argument error returns its status, in the documented order, before the first
HIP call — with pointers that would fault if read —, and the Python layer has its functions.  The table's content is in
tests/test_light_probes_spec.py, what needs the device in tests/test_gpu_light_probes.py."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

import abi_helpers as ah
import helpers as h
from abi_helpers import CAPACITY, FAKE, HEADER, HP, INT_MAX, fake, refused
from raymarcher_amd import abi, lib, sh_irradiance, sphere_directions
from raymarcher_amd._lib import SIGNATURES
from scene_builders import three_primitives_lit as _scene

UNSUPPORTED = abi.RM_ERR_UNSUPPORTED
f32 = np.float32


# ---------------------------------------------------------------- the symbols and the written definition
def test_header_declares_and_library_exports_the_symbols():
    assert ah.params("rm_sphere_directions") == ["int numDirs", "int numSets", "RmProbeDir *out"]
    assert ah.params("rm_light_probes") == [
        "const float *d_positions", "int numProbes", "const RmProbeDir *d_dirs", "int numDirs", "int numSets", "float far",
        "const RmObject *objs", "int numObjects", "const RmLight *lights", "int numLights", "const RmGlobals *g", "const RmSettings *s",
        "const RmResources *res", "RmLightProbe *d_out", "void *stream"]
    Ptr = C.POINTER
    assert SIGNATURES["rm_light_probes"] == (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float, Ptr(abi.RmObject), C.c_int,
                                                       Ptr(abi.RmLight), C.c_int, Ptr(abi.RmGlobals), Ptr(abi.RmSettings), Ptr(abi.RmResources),
                                                       C.c_void_p, C.c_void_p])
    assert SIGNATURES["rm_sphere_directions"] == (C.c_int, [C.c_int, C.c_int, C.c_void_p])
    ah.assert_exported(["rm_light_probes", "rm_sphere_directions"])
    assert not [n for n in ah.declared_functions() if n.startswith("rm_probe_") and "light" in n], "rm_probe_* is the test probes' prefix"


def test_abi_version_stays_and_the_structs_have_64_and_160_bytes():
    ah.assert_abi_version()
    assert C.sizeof(abi.RmProbeDir) == 64 and C.sizeof(abi.RmLightProbe) == 160
    assert [f[0] for f in abi.RmProbeDir._fields_] == ["dir", "reserved", "basis", "pad"]
    assert abi.RmProbeDir.reserved.offset == 12 and abi.RmProbeDir.basis.offset == 16 and abi.RmProbeDir.pad.offset == 52
    assert [f[0] for f in abi.RmLightProbe._fields_] == ["sh", "hits", "reserved"]
    assert abi.RmLightProbe.hits.offset == 144 and abi.RmLightProbe.reserved.offset == 148
    assert re.search(r"typedef struct RmProbeDir\s+\{ float dir\[3\]; float reserved; float basis\[9\]; float pad\[3\]; \} RmProbeDir;\s*/\* 64 bytes \*/",
                     HEADER)
    assert re.search(r"typedef struct RmLightProbe \{ float sh\[9\]\[4\]; int32_t hits; int32_t reserved\[3\]; \} RmLightProbe;\s*/\* 160 bytes \*/",
                     HEADER)
    for name, value in (("RM_MAX_PROBE_DIRS", "1024"), ("RM_MAX_PROBE_TABLE", "4096")):
        assert re.search(rf"#define\s+{name}\s+{value}\b", HEADER), name
    assert (abi.RM_MAX_PROBE_DIRS, abi.RM_MAX_PROBE_TABLE, abi.RM_PATH_LIGHT_PROBES) == (1024, 4096, 21)


def test_header_comment_carries_the_definition():
    ah.assert_comment_has("RmProbeDir", (
        "(i mod numSets)·numDirs + k", "used as given", "RM_TRACE_CLOSEST | RM_TRACE_NO_NORMAL", "tMax = far", "objectId >= 0",
        "evaluates nothing", "h = hit ? 1.0f : 0.0f", "e.basis[j]·c.r", "ONE binary32 multiplication, unfused", "s[m] = s[2m] + s[2m + 1]",
        "rm_field_ambient's tree", "hits = RM_RAY_INVALID", "are not read", "stored as zeros", "does not depend on which other probes",
        "finite tables", "sky visibility", "z = 1 − (2k + 1) / numDirs", "0.6180339887498949", "0.7548776662466927", "rounded once",
        "sqrt(1/4π)", "sqrt(3/4π)", "sqrt(15/4π)", "sqrt(5/16π)", "sqrt(15/16π)", "any table of their own", "before any HIP call",
        "Then numProbes == 0: RM_OK", "above INT_MAX", "rm_debug_last_path() = 21", "nothing is allocated", "symbol lookup"))
    assert re.search(r"21 = a launch of rm_light_probes", HEADER), "rm_debug_last_path's comment does not document 21"


def test_python_signatures():
    from raymarcher_amd.render import Renderer
    sig = inspect.signature(sphere_directions)
    assert list(sig.parameters) == ["num_dirs", "num_sets"] and sig.parameters["num_sets"].default == 1
    sig = inspect.signature(Renderer.light_probes)
    assert list(sig.parameters) == ["self", "tables", "settings", "positions", "directions", "sets", "far", "table", "out"]
    assert [sig.parameters[k].default for k in ("directions", "sets", "far", "table", "out")] == [256, 1, None, None, None]
    assert list(inspect.signature(sh_irradiance).parameters) == ["sh", "normals"]
    # existing signatures are as they were
    assert list(inspect.signature(Renderer.shade_rays).parameters) == ["self", "tables", "settings", "rays", "far", "bright", "out", "out_bright"]
    from raymarcher_amd import RaymarcherError
    with pytest.raises(RaymarcherError):
        sphere_directions(3)
    with pytest.raises(RaymarcherError):
        sphere_directions(1024, 5)
    t = sphere_directions(8, 3)
    assert t.shape == (24, 16) and t.dtype == f32


# ---------------------------------------------------------------- rm_sphere_directions' refusals
BAD_DIRS = (0, -1, 3, 6, 12, 24, 96, 1023, 1025, 2048, 4096, 2 ** 31 - 1, -2 ** 31)
GOOD_SHAPES = ((1, 1), (1, 4096), (2, 2048), (16, 256), (64, 64), (256, 16), (1024, 4), (1024, 1), (128, 8))
BAD_SETS = ((1, 0), (1, -1), (1, 4097), (1024, 5), (16, 257), (64, 65), (2, 2 ** 30), (4, 2 ** 31 - 1), (1, -2 ** 31))


def test_sphere_directions_refusals():
    buf = np.zeros((4096, 16), f32)
    out = C.c_void_p(buf.ctypes.data)
    for k in BAD_DIRS:
        assert refused(lib().rm_sphere_directions(k, 1, out), "numDirs must be a power of two"), k
        assert refused(lib().rm_sphere_directions(k, 0, None), "numDirs"), k  # numDirs comes first
    for k, s in BAD_SETS:
        assert refused(lib().rm_sphere_directions(k, s, out), "numSets"), (k, s)
        assert refused(lib().rm_sphere_directions(k, s, None), "numSets"), (k, s)  # and numSets before out
    assert (buf == 0).all()
    for k, s in GOOD_SHAPES:
        assert refused(lib().rm_sphere_directions(k, s, None), "null out"), (k, s)
        assert lib().rm_sphere_directions(k, s, out) == abi.RM_OK, (k, s)


# ---------------------------------------------------------------- rm_light_probes' refusals, all without a device
DEFAULT = object()


def call(objs, no, lights, nl, g, s=DEFAULT, n=100, K=16, sets=1, far=100.0, res=None, pos=FAKE, dirs=FAKE, out=FAKE):
    s = abi.default_settings() if s is DEFAULT else s
    return lib().rm_light_probes(pos, n, dirs, K, sets, far, objs, no, lights, nl, C.byref(g) if g is not None else None,
                                 C.byref(s) if s is not None else None, C.byref(res) if res is not None else None, out, None)


ARRAYS = "null d_positions, d_dirs or d_out"  # the first check behind the scene's: a call that gets this far passed everything before it


def test_the_order_of_the_checks():
    """Every check fails at the start; each step mends one, and the earliest check still violated answers."""
    objs, no, lights, nl, g = _scene()
    many = (abi.RmObject * (abi.RM_MAX_OBJECTS + 1))(*[h.make_object(abi.RM_SPHERE) for _ in range(abi.RM_MAX_OBJECTS + 1)])
    two_d = h.make_globals(two_d=1)
    sea = abi.default_settings(features=abi.RM_FEAT_SEA)

    def run(a):
        return call(a["objs"], a["no"], lights, nl, a["g"], s=a["s"], n=a["n"], K=a["K"], sets=a["sets"], far=a["far"], pos=a["pos"],
                    dirs=a["dirs"], out=a["out"])

    start = dict(n=-1, K=3, sets=0, far=float("nan"), objs=many, no=abi.RM_MAX_OBJECTS + 1, g=None, s=sea, pos=None, dirs=fake(0x1004), out=HP)
    ah.walk(run, start, [
        ({}, ah.INVALID, "negative numProbes"),
        ({"n": INT_MAX}, ah.INVALID, "numDirs must be a power of two"),
        ({"K": 1024}, ah.INVALID, "numSets"),
        ({"sets": 5}, ah.INVALID, "numSets"),
        ({"sets": 4}, ah.INVALID, "INT_MAX"),
        ({"n": INT_MAX // 1024}, ah.INVALID, "null scene pointer"),
        ({"g": two_d}, ah.INVALID, "far"),
        ({"far": 100.0}, UNSUPPORTED, "TERRAIN / CLOUD / SEA"),
        ({"s": abi.default_settings()}, UNSUPPORTED, "isTwoD"),
        ({"g": g}, CAPACITY, "RM_MAX_OBJECTS"),
        ({"objs": objs, "no": no}, ah.INVALID, ARRAYS),
        ({"pos": HP}, ah.INVALID, "16-byte aligned"),
        ({"dirs": HP}, ah.INVALID, "d_positions is not device-accessible"),  # host memory is not device memory: the only check that asks the HIP runtime, and the last
    ])


def test_counts_and_the_table():
    objs, no, lights, nl, g = _scene()
    for n in (-1, -INT_MAX, -2 ** 31):
        assert refused(call(objs, no, lights, nl, g, n=n), "negative numProbes"), n
        assert refused(call(objs, no, lights, nl, g, n=n, K=3, sets=0), "negative numProbes"), n
    for k in BAD_DIRS:
        assert refused(call(objs, no, lights, nl, g, K=k), "numDirs must be a power of two"), k
        assert refused(call(objs, no, lights, nl, g, K=k, sets=0, n=0), "numDirs must be a power of two"), k  # before the empty call
    for k, s in BAD_SETS:
        assert refused(call(objs, no, lights, nl, g, K=k, sets=s), "numSets"), (k, s)
        assert refused(call(objs, no, lights, nl, g, K=k, sets=s, n=0, pos=None), "numSets"), (k, s)
    # numProbes == 0: RM_OK with null everything, nothing is read
    for k, s in GOOD_SHAPES:
        assert call(None, 5, None, -3, None, s=None, n=0, K=k, sets=s, far=float("nan"), pos=None, dirs=None, out=None) == abi.RM_OK
    # the rays of a call fit an int
    for n, k in ((INT_MAX, 2), (INT_MAX // 2 + 1, 2), (INT_MAX // 1024 + 1, 1024), (2 ** 21, 1024)):
        assert refused(call(objs, no, lights, nl, g, n=n, K=k), "INT_MAX"), (n, k)
        assert refused(call(objs, no, lights, nl, None, n=n, K=k, far=-1.0), "INT_MAX"), (n, k)  # before the scene pointers
    for n, k in ((INT_MAX, 1), (INT_MAX // 2, 2), (INT_MAX // 1024, 1024)):
        assert refused(call(objs, no, lights, nl, g, n=n, K=k, pos=None), ARRAYS), (n, k)


def test_scene_pointers_far_layers_and_the_scene():
    objs, no, lights, nl, g = _scene()
    assert refused(call(objs, no, lights, nl, None), "null scene pointer")
    assert refused(call(objs, no, lights, nl, g, s=None), "null scene pointer")
    assert refused(call(None, no, lights, nl, g), "null scene pointer")
    assert refused(call(objs, no, None, nl, g), "null scene pointer")
    assert refused(call(objs, -1, lights, nl, g), "null scene pointer")
    assert refused(call(objs, no, lights, -1, g), "null scene pointer")
    assert refused(call(None, 0, None, 0, g, pos=None), ARRAYS)  # empty tables need no pointers
    for far in (float("nan"), -1.0, -1e-30, float("inf"), float("-inf")):
        assert refused(call(objs, no, lights, nl, g, far=far), "far must be finite and not negative"), far
    for far in (0.0, -0.0, 1e-30, 3.0e38):
        assert refused(call(objs, no, lights, nl, g, far=far, dirs=None), ARRAYS), far
    assert refused(call(objs, no, lights, nl, g, s=abi.default_settings(features=abi.RM_FEAT_SEA), far=-1.0), "far")
    for feat in (abi.RM_FEAT_TERRAIN, abi.RM_FEAT_CLOUD, abi.RM_FEAT_SEA, abi.RM_FEAT_TERRAIN | abi.RM_FEAT_PERLIN_BUMP):
        assert refused(call(objs, no, lights, nl, g, s=abi.default_settings(features=feat)), "TERRAIN / CLOUD / SEA", want=UNSUPPORTED), feat
    for feat in (0, abi.RM_FEAT_SKY_BACKGROUND, abi.RM_FEAT_DARK_BACKGROUND, abi.RM_FEAT_REFERENCE_DEFAULT):
        assert refused(call(objs, no, lights, nl, g, s=abi.default_settings(features=feat), out=None), ARRAYS), feat
    assert refused(call(objs, no, lights, nl, h.make_globals(two_d=1)), "isTwoD", want=UNSUPPORTED)
    # validate_scene: rm_render_res's statuses and texts
    lots = (abi.RmLight * (abi.RM_MAX_LIGHTS + 1))(*[h.make_light(abi.RM_LIGHT_POINT) for _ in range(abi.RM_MAX_LIGHTS + 1)])
    assert refused(call(objs, no, lots, abi.RM_MAX_LIGHTS + 1, g), "RM_MAX_LIGHTS", want=CAPACITY)
    for field in ("maxSteps", "fractalIters", "mengerLevels", "numReflection"):
        assert refused(call(objs, no, lights, nl, g, s=abi.default_settings(**{field: -1})), "loop bound"), field
    night = abi.default_settings(features=abi.RM_FEAT_NIGHTSKY_BACKGROUND)
    assert refused(call(objs, no, lights, nl, g, s=night), "noise", want=UNSUPPORTED)
    res = abi.RmResources()
    res.noise = abi.RmTexture(0x2000, 4, 4)
    assert refused(call(objs, no, lights, nl, g, s=night, res=res, pos=None), ARRAYS)
    assert refused(call(objs, no, lights, nl, g, s=abi.default_settings(enableSkyBox=1)), "enableSkyBox", want=UNSUPPORTED)
    objs[1].type = abi.RM_CUSTOM
    assert refused(call(objs, no, lights, nl, g, pos=None), "object 1", want=UNSUPPORTED)  # the scene comes before the arrays


def test_the_three_arrays():
    objs, no, lights, nl, g = _scene()
    for kw in ({"pos": None}, {"dirs": None}, {"out": None}):
        assert refused(call(objs, no, lights, nl, g, **kw), ARRAYS), kw
    for off in (4, 8, 12, 1):
        bad = fake(0x1000 + off)
        for key in ("pos", "dirs", "out"):
            assert refused(call(objs, no, lights, nl, g, **{key: bad}), "16-byte aligned"), (key, off)
    assert refused(call(objs, no, lights, nl, g, pos=None, dirs=fake(0x1004)), ARRAYS)  # null before misaligned
    # host memory is not device memory: the only check that asks the HIP runtime, and the last
    assert refused(call(objs, no, lights, nl, g, pos=HP, dirs=HP, out=HP), "d_positions")
