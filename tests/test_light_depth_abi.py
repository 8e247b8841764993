"""rm_probe_depth_weights, rm_light_probes_depth and rm_light_grid_irradiance_visible without a GPU: the header declares them and the
library exports them under the unchanged ABI version, the record has 512 bytes, abi.py and _lib.py mirror the header, the header's
comment carries the three definitions, every argument error returns its status in the documented order before the first HIP call —
with pointers that would fault if read —, and the Python layer has its names while the existing ones keep their signatures.  The
arithmetic is in tests/test_light_depth_spec.py, what needs the device in tests/test_gpu_light_depth.py."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

import abi_helpers as ah
import helpers as h
from abi_helpers import CAPACITY, FAKE, HEADER, HP, INT_MAX, fake, refused
from raymarcher_amd import abi, lib, probe_depth_weights, sphere_directions
from raymarcher_amd._lib import SIGNATURES
from scene_builders import three_primitives_lit as _scene

UNSUPPORTED = abi.RM_ERR_UNSUPPORTED
f32 = np.float32
inf, nan = float("inf"), float("nan")
NAMES = ["rm_probe_depth_weights", "rm_light_probes_depth", "rm_light_grid_irradiance_visible"]


# ---------------------------------------------------------------- the symbols and the written definitions
def test_header_declares_and_library_exports_the_symbols():
    assert ah.params("rm_probe_depth_weights") == ["const RmProbeDir *dirs", "int numDirs", "int numSets", "float sharpness", "float *out"]
    assert ah.params("rm_light_probes_depth") == [
        "const float *d_positions", "int numProbes", "const RmProbeDir *d_dirs", "const float *d_weights", "int numDirs", "int numSets",
        "float maxDistance", "const RmObject *objs", "int numObjects", "const RmGlobals *g", "const RmSettings *s", "RmProbeDepth *d_out",
        "void *stream"]
    assert ah.params("rm_light_grid_irradiance_visible") == [
        "const RmLightProbe *d_probes", "const RmProbeDepth *d_depth", "const int dims[3]", "const float origin[3]", "const float step[3]",
        "const float *d_points", "const float *d_normals", "int numPoints", "uint32_t flags", "float normalBias", "RmGridLight *d_out",
        "void *stream"]
    Ptr = C.POINTER
    assert SIGNATURES["rm_probe_depth_weights"] == (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p])
    assert SIGNATURES["rm_light_probes_depth"] == (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float,
                                                             Ptr(abi.RmObject), C.c_int, Ptr(abi.RmGlobals), Ptr(abi.RmSettings), C.c_void_p,
                                                             C.c_void_p])
    assert SIGNATURES["rm_light_grid_irradiance_visible"] == (C.c_int, [C.c_void_p, C.c_void_p, Ptr(C.c_int), Ptr(C.c_float), Ptr(C.c_float),
                                                                        C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_float, C.c_void_p,
                                                                        C.c_void_p])
    ah.assert_exported(NAMES)


def test_abi_version_stays_and_the_record_has_512_bytes():
    ah.assert_abi_version()
    assert C.sizeof(abi.RmProbeDepth) == 512 and [f[0] for f in abi.RmProbeDepth._fields_] == ["moments"]
    assert abi.RmProbeDepth.moments.offset == 0 and abi.RmProbeDepth.moments.size == 64 * 2 * 4
    assert re.search(r"typedef struct RmProbeDepth \{ float moments\[64\]\[2\]; \} RmProbeDepth;\s*/\* 512 bytes", HEADER)
    for name, value in (("RM_PROBE_DEPTH_TEXELS", "64"), ("RM_LIGHT_GRID_VIS_FLOOR", r"1\.0e-6f")):
        assert re.search(rf"#define\s+{name}\s+{value}(?!\w)", HEADER), name
    assert (abi.RM_PROBE_DEPTH_TEXELS, abi.RM_LIGHT_GRID_VIS_FLOOR, abi.RM_PATH_LIGHT_PROBES_DEPTH) == (64, 1.0e-6, 22)
    assert C.sizeof(abi.RmLightProbe) == 160 and C.sizeof(abi.RmGridLight) == 32 and C.sizeof(abi.RmProbeDir) == 64, "the records beside it"


def test_header_comment_carries_the_definitions():
    ah.assert_comment_has("RmProbeDepth", (
        "Majercik et al. 2019", "x = tx + 8·ty", "((tx + 0.5)/8)·2 − 1", "Z = 1 − |u| − |v|", "(1 − |v|)·sign(u)", "sign(±0) = +1",
        # the weights
        "host only", "pow(max(0, dot), sharpness)", "pow(0, 0) = 1", "ascending k", "rounded ONCE", "largest dot", "ties to the lowest k",
        "no texel is ever empty", "takes no part in sums", "as rm_sphere_directions does",
        # the bake
        "(i mod numSets)·numDirs + k", "RM_TRACE_CLOSEST | RM_TRACE_NO_NORMAL", "tMax = maxDistance", "maxDistance on a miss", "r_k = +0",
        "evaluates nothing", "T_k(w[k][x]·r_k)", "T_k(w[k][x]·(r_k·r_k))", "ONE binary32 multiplication", "s[m] = s[2m] + s[2m + 1]",
        "512 bytes of zeros", "does not depend on which probes share its call", "finite weights", "maxDistance in the place of far",
        "not greater than 0", "Then numProbes == 0: RM_OK", "above INT_MAX", "rm_debug_last_path() = 22", "lane x becomes texel x",
        "same operands in the same pairs", "nothing is allocated",
        # the lookup
        "q = p + normalBias·n", "r = sqrt((vx·vx + vy·vy) + vz·vz)", "r == 0 gives vis = 1", "l1 = (|vx| + |vy|) + |vz|",
        "((1 − |oy|)·sign(ox), (1 − |ox|)·sign(oy))", "u_a = o_a·4 + 3.5", "i_a = min((int)floor(u_a), 6)",
        "m = (a·(1 − fx) + b·fx)·(1 − fy) + (c·(1 − fx) + d·fx)·fy", "wrap is NOT followed", "r <= m gives vis = 1", "var = |m2 − m·m|",
        "den = var + dd·dd", "1 for den == 0", "vis = max((c·c)·c, RM_LIGHT_GRID_VIS_FLOOR)", "w_c = (t_c·face)·vis",
        "neither sh nor depth words are read", "IN EVERY WORD", "normalBias behind the step", "rm_debug_last_path() keeps its value",
        "symbol lookup"))
    assert re.search(r"22 = a launch of rm_light_probes_depth", HEADER), "rm_debug_last_path's comment does not document 22"


def test_python_names():
    from raymarcher_amd import LightGrid
    from raymarcher_amd.render import Renderer
    sig = inspect.signature(probe_depth_weights)
    assert list(sig.parameters) == ["table", "sets", "sharpness"] and (sig.parameters["sets"].default, sig.parameters["sharpness"].default) == (1, 50.0)
    sig = inspect.signature(Renderer.light_probes_depth)
    assert list(sig.parameters) == ["self", "tables", "settings", "positions", "directions", "sets", "max_distance", "table", "weights",
                                    "sharpness", "out"]
    assert [sig.parameters[k].default for k in ("directions", "sets", "max_distance", "table", "weights", "sharpness", "out")] == \
        [256, 1, None, None, None, 50.0, None]
    sig = inspect.signature(LightGrid.irradiance_visible)
    assert list(sig.parameters) == ["self", "points", "normals", "facing", "out", "visible", "normal_bias"]
    assert [sig.parameters[k].default for k in ("facing", "out", "visible", "normal_bias")] == [True, None, None, None]
    sig = inspect.signature(LightGrid.light_gbuffer_visible)
    assert list(sig.parameters) == ["self", "normal_depth", "position", "facing", "visible", "normal_bias"]
    assert list(inspect.signature(LightGrid.set_depth).parameters) == ["self", "depth", "normal_bias"]
    sig = inspect.signature(Renderer.light_grid_visible)
    assert list(sig.parameters) == ["self", "tables", "settings", "dims", "bounds", "directions", "sets", "far", "mask_inside", "visibility", "sharpness"]
    assert sig.parameters["visibility"].default is True
    # the names that were there keep their signatures: a grid without depth is what it was
    assert list(inspect.signature(LightGrid.__init__).parameters) == ["self", "renderer", "probes", "origin", "step", "dims"]
    assert list(inspect.signature(LightGrid.irradiance).parameters) == ["self", "points", "normals", "facing", "out"]
    assert list(inspect.signature(Renderer.light_grid).parameters)[-1] == "mask_inside"
    # the wrapper: shapes, and the library's refusals as exceptions
    from raymarcher_amd import RaymarcherError
    w = probe_depth_weights(sphere_directions(8, 3), sets=3)
    assert w.shape == (24, 64) and w.dtype == f32
    with pytest.raises(ValueError):
        probe_depth_weights(np.zeros((8, 15), f32))
    with pytest.raises(ValueError):
        probe_depth_weights(sphere_directions(8, 1), sets=3)
    with pytest.raises(RaymarcherError):
        probe_depth_weights(sphere_directions(8, 1), sharpness=-1.0)
    with pytest.raises(RaymarcherError):
        probe_depth_weights(np.zeros((3, 16), f32))


# ---------------------------------------------------------------- rm_probe_depth_weights' refusals
BAD_DIRS = (0, -1, 3, 6, 12, 24, 96, 1023, 1025, 2048, 4096, 2 ** 31 - 1, -2 ** 31)
GOOD_SHAPES = ((1, 1), (1, 4096), (2, 2048), (16, 256), (64, 64), (256, 16), (1024, 4), (1024, 1), (128, 8))
BAD_SETS = ((1, 0), (1, -1), (1, 4097), (1024, 5), (16, 257), (64, 65), (2, 2 ** 30), (4, 2 ** 31 - 1), (1, -2 ** 31))


def test_depth_weights_refusals():
    table = sphere_directions(1, 4096)
    buf = np.zeros((4096, 64), f32)
    dirs, out = C.c_void_p(table.ctypes.data), C.c_void_p(buf.ctypes.data)
    W = lib().rm_probe_depth_weights
    for k in BAD_DIRS:
        assert refused(W(dirs, k, 1, 50.0, out), "numDirs must be a power of two"), k
        assert refused(W(None, k, 0, nan, None), "numDirs"), k  # numDirs comes first
    for k, s in BAD_SETS:
        assert refused(W(dirs, k, s, 50.0, out), "numSets"), (k, s)
        assert refused(W(None, k, s, -1.0, None), "numSets"), (k, s)  # and numSets before the pointers and the sharpness
    for k, s in GOOD_SHAPES:
        assert refused(W(None, k, s, 50.0, out), "null dirs or out"), (k, s)
        assert refused(W(dirs, k, s, nan, None), "null dirs or out"), (k, s)  # the pointers before the sharpness
        for sharp in (nan, inf, -inf, -1.0, -1e-30):
            assert refused(W(dirs, k, s, sharp, out), "sharpness must be finite and not negative"), (k, s, sharp)
    assert (buf == 0).all(), "a refused call wrote"
    for sharp in (0.0, -0.0, 1e-30, 50.0, 3.0e38):
        assert W(dirs, 16, 4, sharp, out) == abi.RM_OK, sharp


# ---------------------------------------------------------------- rm_light_probes_depth's refusals, all without a device
DEFAULT = object()
ARRAYS = "null d_positions, d_dirs, d_weights or d_out"  # the first check behind the scene's


def bake(objs, no, g, s=DEFAULT, n=100, K=16, sets=1, dist=2.0, pos=FAKE, dirs=FAKE, wts=FAKE, out=FAKE):
    s = abi.default_settings() if s is DEFAULT else s
    return lib().rm_light_probes_depth(pos, n, dirs, wts, K, sets, dist, objs, no, C.byref(g) if g is not None else None,
                                       C.byref(s) if s is not None else None, out, None)


def test_the_order_of_the_bakes_checks():
    """Every check fails at the start; each step mends one, and the earliest check still violated answers."""
    objs, no, _, _, g = _scene()
    many = (abi.RmObject * (abi.RM_MAX_OBJECTS + 1))(*[h.make_object(abi.RM_SPHERE) for _ in range(abi.RM_MAX_OBJECTS + 1)])
    two_d = h.make_globals(two_d=1)
    sea = abi.default_settings(features=abi.RM_FEAT_SEA)

    def run(a):
        return bake(a["objs"], a["no"], a["g"], s=a["s"], n=a["n"], K=a["K"], sets=a["sets"], dist=a["dist"], pos=a["pos"], dirs=a["dirs"],
                    wts=a["wts"], out=a["out"])

    start = dict(n=-1, K=3, sets=0, dist=0.0, objs=many, no=abi.RM_MAX_OBJECTS + 1, g=None, s=sea, pos=None, dirs=fake(0x1004), wts=HP, out=HP)
    ah.walk(run, start, [
        ({}, ah.INVALID, "negative numProbes"),
        ({"n": INT_MAX}, ah.INVALID, "numDirs must be a power of two"),
        ({"K": 1024}, ah.INVALID, "numSets"),
        ({"sets": 5}, ah.INVALID, "numSets"),
        ({"sets": 4}, ah.INVALID, "INT_MAX"),
        ({"n": INT_MAX // 1024}, ah.INVALID, "null scene pointer"),
        ({"g": two_d}, ah.INVALID, "maxDistance"),
        ({"dist": 1e-30}, UNSUPPORTED, "TERRAIN / CLOUD / SEA"),
        ({"s": abi.default_settings()}, UNSUPPORTED, "isTwoD"),
        ({"g": g}, CAPACITY, "RM_MAX_OBJECTS"),
        ({"objs": objs, "no": no}, ah.INVALID, ARRAYS),
        ({"pos": HP}, ah.INVALID, "16-byte aligned"),
        ({"dirs": HP}, ah.INVALID, "d_positions is not device-accessible"),  # the only check that asks the HIP runtime, and the last
    ])


def test_the_bakes_counts_table_distance_and_scene():
    objs, no, _, _, g = _scene()
    for n in (-1, -INT_MAX, -2 ** 31):
        assert refused(bake(objs, no, g, n=n), "negative numProbes"), n
        assert refused(bake(objs, no, g, n=n, K=3, sets=0), "negative numProbes"), n
    for k in BAD_DIRS:
        assert refused(bake(objs, no, g, K=k), "numDirs must be a power of two"), k
        assert refused(bake(objs, no, g, K=k, sets=0, n=0), "numDirs must be a power of two"), k  # before the empty call
    for k, s in BAD_SETS:
        assert refused(bake(objs, no, g, K=k, sets=s), "numSets"), (k, s)
        assert refused(bake(objs, no, g, K=k, sets=s, n=0, pos=None), "numSets"), (k, s)
    for k, s in GOOD_SHAPES:  # numProbes == 0: RM_OK with null everything, nothing is read
        assert bake(None, 5, None, s=None, n=0, K=k, sets=s, dist=nan, pos=None, dirs=None, wts=None, out=None) == abi.RM_OK
    for n, k in ((INT_MAX, 2), (INT_MAX // 1024 + 1, 1024), (2 ** 21, 1024)):
        assert refused(bake(objs, no, g, n=n, K=k), "INT_MAX"), (n, k)
        assert refused(bake(objs, no, None, n=n, K=k, dist=-1.0), "INT_MAX"), (n, k)  # before the scene pointers
    for n, k in ((INT_MAX, 1), (INT_MAX // 1024, 1024)):
        assert refused(bake(objs, no, g, n=n, K=k, pos=None), ARRAYS), (n, k)
    assert refused(bake(objs, no, None), "null scene pointer") and refused(bake(objs, no, g, s=None), "null scene pointer")
    assert refused(bake(None, no, g), "null scene pointer") and refused(bake(objs, -1, g), "null scene pointer")
    assert refused(bake(None, 0, g, pos=None), ARRAYS)  # an empty table needs no pointer
    for dist in (nan, inf, -inf, 0.0, -0.0, -1.0, -1e-30):
        assert refused(bake(objs, no, g, dist=dist), "maxDistance must be finite and greater than 0"), dist
        assert refused(bake(objs, no, g, dist=dist, s=abi.default_settings(features=abi.RM_FEAT_SEA)), "maxDistance"), dist  # before the layers
    for dist in (1e-45, 1e-30, 1.0, 3.0e38):
        assert refused(bake(objs, no, g, dist=dist, wts=None), ARRAYS), dist
    for feat in (abi.RM_FEAT_TERRAIN, abi.RM_FEAT_CLOUD, abi.RM_FEAT_SEA, abi.RM_FEAT_TERRAIN | abi.RM_FEAT_PERLIN_BUMP):
        assert refused(bake(objs, no, g, s=abi.default_settings(features=feat)), "TERRAIN / CLOUD / SEA", want=UNSUPPORTED), feat
    assert refused(bake(objs, no, h.make_globals(two_d=1)), "isTwoD", want=UNSUPPORTED)
    # lights and samplers are no arguments: settings that would need them are no concern of a march
    assert refused(bake(objs, no, g, s=abi.default_settings(enableSkyBox=1), out=None), ARRAYS)
    objs[1].type = abi.RM_CUSTOM
    assert refused(bake(objs, no, g, pos=None), "object 1", want=UNSUPPORTED)  # the table comes before the arrays


def test_the_bakes_four_arrays():
    objs, no, _, _, g = _scene()
    for key in ("pos", "dirs", "wts", "out"):
        assert refused(bake(objs, no, g, **{key: None}), ARRAYS), key
        for off in (4, 8, 12, 1):
            assert refused(bake(objs, no, g, **{key: fake(0x1000 + off)}), "16-byte aligned"), (key, off)
    assert refused(bake(objs, no, g, pos=None, wts=fake(0x1004)), ARRAYS)  # null before misaligned
    assert refused(bake(objs, no, g, pos=HP, dirs=HP, wts=HP, out=HP), "d_positions")  # host memory is not device memory


# ---------------------------------------------------------------- rm_light_grid_irradiance_visible's refusals, all without a device
GOOD = dict(n=100, dims=(4, 3, 2), origin=(0.0, 0.0, 0.0), step=(1.0, 1.0, 1.0), flags=1, bias=0.1, probes=FAKE, depth=FAKE, pts=FAKE, nrm=FAKE,
            out=FAKE)
LOOK_ARRAYS = "null d_probes, d_depth, d_points, d_normals or d_out"


def look(**over):
    a = dict(GOOD, **over)
    dims = (C.c_int * 3)(*a["dims"]) if a["dims"] is not None else None
    return lib().rm_light_grid_irradiance_visible(a["probes"], a["depth"], dims, ah.vec3(a["origin"]), ah.vec3(a["step"]), a["pts"], a["nrm"],
                                                  a["n"], a["flags"], a["bias"], a["out"], None)


def test_the_order_of_the_lookups_checks():
    start = dict(n=-1, dims=None, origin=(nan, 0, 0), step=(0.0, 1, 1), bias=nan, flags=6, probes=None, depth=fake(0x1008), pts=fake(0x1004),
                 nrm=HP, out=HP)
    ah.walk(lambda a: look(**a), start, [
        ({}, ah.INVALID, "negative numPoints"),
        ({"n": INT_MAX}, ah.INVALID, "null dims, origin or step"),
        ({"dims": (1, 1024, 1024)}, ah.INVALID, "grid dimension"),
        ({"dims": (1024, 1024, 1024)}, ah.INVALID, "RM_MAX_LIGHT_GRID_PROBES"),
        ({"dims": (1024, 1024, 16)}, ah.INVALID, "origin must be finite"),
        ({"origin": (0, -3e38, 0)}, ah.INVALID, "step must be finite and greater than 0"),
        ({"step": (1e-30, 1, 3e38)}, ah.INVALID, "normalBias must be finite"),
        ({"bias": -3e38}, ah.INVALID, "flag bits"),
        ({"flags": 1}, ah.INVALID, LOOK_ARRAYS),
        ({"probes": HP}, ah.INVALID, "16-byte aligned"),
        ({"depth": HP}, ah.INVALID, "16-byte aligned"),
        ({"pts": HP}, ah.INVALID, "d_probes is not device-accessible"),  # the only check that asks the HIP runtime, and the last
    ])


def test_the_lookups_grid_bias_and_arrays():
    for n in (-1, -2 ** 31):
        assert refused(look(n=n, dims=None, bias=nan), "negative numPoints"), n
    for key in ("dims", "origin", "step"):
        assert refused(look(**{key: None}), "null dims, origin or step"), key
    for d in ((1, 2, 2), (2, 0, 2), (1025, 2, 2), (2, 2, -1)):
        assert refused(look(dims=d, n=0, bias=inf), "grid dimension"), d
    for d in ((1024, 1024, 17), (257, 256, 256)):
        assert refused(look(dims=d, n=0), "RM_MAX_LIGHT_GRID_PROBES"), d
    for o in ah.BAD_ORIGINS:
        assert refused(look(origin=o, bias=nan), "origin must be finite"), o
    for st in ah.BAD_STEPS:
        assert refused(look(step=st, bias=nan), "step must be finite and greater than 0"), st
    for bias in (nan, inf, -inf):
        assert refused(look(bias=bias), "normalBias must be finite"), bias
        assert refused(look(bias=bias, flags=2, n=0, probes=None), "normalBias"), bias  # before the flags and the empty call
    for flags in (2, 3, 0x80000000, 0xFFFFFFFE):
        assert refused(look(flags=flags, n=0, depth=None), "flag bits other than RM_LIGHT_GRID_FACING"), flags
    for bias in (0.0, -0.0, -1.0, 1e-45, 3.0e38):  # numPoints == 0: RM_OK with null arrays, nothing is read
        assert look(n=0, bias=bias, probes=None, depth=None, pts=None, nrm=None, out=None) == abi.RM_OK, bias
        assert refused(look(bias=bias, out=None), LOOK_ARRAYS), bias
    for key in ("probes", "depth", "pts", "nrm", "out"):
        assert refused(look(**{key: None}), LOOK_ARRAYS), key
        for off in (4, 8, 12, 1):
            assert refused(look(**{key: fake(0x1000 + off)}), "16-byte aligned"), (key, off)
    assert refused(look(pts=None, depth=fake(0x1004)), LOOK_ARRAYS)  # null before misaligned
    assert refused(look(probes=HP, depth=HP, pts=HP, nrm=HP, out=HP), "d_probes")
