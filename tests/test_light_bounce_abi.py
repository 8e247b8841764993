"""rm_shade_rays_indirect and rm_light_probes_indirect without a GPU: the header declares them and the library exports them under
the unchanged ABI version, RmLightGridRef in abi.py has the header's layout, the header's comment carries the definition, every
argument error returns its status in the documented order before the first HIP call — with pointers that would fault if read —,
and the Python layer has its names while the pinned ones keep their signatures.  The arithmetic is in
tests/test_light_bounce_spec.py, what needs the device in tests/test_gpu_light_bounce.py."""
import ctypes as C
import inspect
import re

import numpy as np

import abi_helpers as ah
import helpers as h
from abi_helpers import CAPACITY, FAKE, HEADER, HP, INT_MAX, fake, refused
from raymarcher_amd import abi, lib
from raymarcher_amd._lib import SIGNATURES
from scene_builders import three_primitives_lit as _scene

UNSUPPORTED = abi.RM_ERR_UNSUPPORTED
inf, nan = float("inf"), float("nan")
NAMES = ["rm_shade_rays_indirect", "rm_light_probes_indirect"]


# ---------------------------------------------------------------- the symbols and the written definition
def test_header_declares_and_library_exports_the_symbols():
    assert ah.params("rm_shade_rays_indirect") == [
        "const RmRay *d_rays", "int numRays", "float far", "const RmObject *objs", "int numObjects", "const RmLight *lights", "int numLights",
        "const RmGlobals *g", "const RmSettings *s", "const RmResources *res", "const RmLightGridRef *grid", "float *d_rgba", "void *stream"]
    assert ah.params("rm_light_probes_indirect") == [
        "const float *d_positions", "int numProbes", "const RmProbeDir *d_dirs", "int numDirs", "int numSets", "float far",
        "const RmObject *objs", "int numObjects", "const RmLight *lights", "int numLights", "const RmGlobals *g", "const RmSettings *s",
        "const RmResources *res", "const RmLightGridRef *grid", "RmLightProbe *d_out", "void *stream"]
    # rm_shade_rays' and rm_light_probes' arguments, with the grid behind res and no bright output
    assert [p for p in ah.params("rm_shade_rays_indirect") if "grid" not in p] == [p for p in ah.params("rm_shade_rays") if "d_bright" not in p]
    assert [p for p in ah.params("rm_light_probes_indirect") if "grid" not in p] == ah.params("rm_light_probes")
    Ptr = C.POINTER
    assert SIGNATURES["rm_shade_rays_indirect"] == (C.c_int, [C.c_void_p, C.c_int, C.c_float, Ptr(abi.RmObject), C.c_int, Ptr(abi.RmLight),
                                                              C.c_int, Ptr(abi.RmGlobals), Ptr(abi.RmSettings), Ptr(abi.RmResources),
                                                              Ptr(abi.RmLightGridRef), C.c_void_p, C.c_void_p])
    assert SIGNATURES["rm_light_probes_indirect"] == (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float, Ptr(abi.RmObject),
                                                                C.c_int, Ptr(abi.RmLight), C.c_int, Ptr(abi.RmGlobals), Ptr(abi.RmSettings),
                                                                Ptr(abi.RmResources), Ptr(abi.RmLightGridRef), C.c_void_p, C.c_void_p])
    ah.assert_exported(NAMES)


def test_abi_version_stays_and_the_grid_struct_has_the_headers_layout():
    ah.assert_abi_version()
    m = re.search(r"typedef struct RmLightGridRef \{(.*?)\} RmLightGridRef;", ah.HEADER_CODE, flags=re.S)
    assert m and re.search(r"\} RmLightGridRef;\s*/\* 64 bytes", HEADER)
    fields = [re.sub(r"\s+", " ", f.strip()) for f in m.group(1).split(";") if f.strip()]
    assert fields == ["const RmLightProbe *d_probes", "const RmProbeDepth *d_depth", "int dims[3]", "float origin[3]", "float step[3]",
                      "float strength", "uint32_t flags", "float normalBias"]
    R = abi.RmLightGridRef
    assert [f[0] for f in R._fields_] == ["d_probes", "d_depth", "dims", "origin", "step", "strength", "flags", "normalBias"]
    assert C.sizeof(R) == 64 and C.alignment(R) == 8
    assert [(getattr(R, n).offset, getattr(R, n).size) for n, _ in R._fields_] == [(0, 8), (8, 8), (16, 12), (28, 12), (40, 12), (52, 4), (56, 4),
                                                                                   (60, 4)]
    assert re.search(r"#define\s+RM_INV_PI\s+\(\(float\)0\.31830988618379067\)", HEADER)
    assert np.float32(abi.RM_INV_PI) == np.float32(1 / np.pi) and float(np.float32(abi.RM_INV_PI)) == abi.RM_INV_PI
    assert (abi.RM_PATH_SHADE_RAYS_INDIRECT, abi.RM_PATH_LIGHT_PROBES_INDIRECT) == (23, 24)


def test_header_comment_carries_the_definition():
    ah.assert_comment_has("RmLightGridRef", (
        "albedo · E_grid(hit, normal) / π", "ONE host struct", "copied before the call returns", "d_depth the grid's RmProbeDepth records or NULL",
        "colour is what rm_shade_rays stores for the ray, in every word", "rm_trace_rays(RM_TRACE_CLOSEST)", "tMax = far",
        "NO TERM", "no addition is performed, not even of +0", "the ray is invalid", "the primary march misses", "isEmissive", "probes <= 0",
        "rm_light_grid_irradiance_visible stores at (p, n)", "rm_light_grid_irradiance's where it is NULL", "word for word",
        "ec[ch] = e[ch] > 0 ? e[ch] : +0", "NaN become +0", "strength · RM_INV_PI", "one multiplication, on the host",
        "the value render() puts into mat.dif", "x[ch]  = (dif[ch] · ec[ch]) · k", "ind = c · (x · 8)", "bulbTrapColor(trap.y, trap.z, trap.w)",
        "ind = c · x", "cosine palette of trap.z", "every other type ind = x", "UB3's rule", "out.rgb = colour.rgb + ind",
        "one addition per channel", "alpha is colour's", "ONE binary32 operation as written", "PRIMARY HIT ONLY",
        "reflection and refraction bounces get none", "ambient occlusion does not multiply it", "There is no bright output",
        "rm_debug_last_path() = 23", "rm_debug_last_path() = 24", "numRays == 0 is RM_OK", "a null grid", "a non-finite normalBias",
        "d_depth may be NULL", "a non-finite strength", "last, an array that is not device memory", "RM_ERR_UNSUPPORTED",
        "the hit flag, the leaves", "in every word", "overlaps the grid's probe records", "a bake must not read the grid it writes",
        "nothing is allocated", "symbol lookup"))
    assert re.search(r"23 = a launch of rm_shade_rays_indirect, 24 = a launch of rm_light_probes_indirect", HEADER)


def test_python_names():
    from raymarcher_amd import LightGrid
    from raymarcher_amd.render import Renderer
    sig = inspect.signature(Renderer.shade_rays_indirect)
    assert list(sig.parameters) == ["self", "tables", "settings", "rays", "grid", "far", "strength", "facing", "visible", "normal_bias", "out"]
    assert [sig.parameters[k].default for k in ("far", "strength", "facing", "visible", "normal_bias", "out")] == [None, 1.0, True, None, None, None]
    sig = inspect.signature(Renderer.light_probes_indirect)
    assert list(sig.parameters) == ["self", "tables", "settings", "positions", "grid", "directions", "sets", "far", "table", "strength", "facing",
                                    "visible", "normal_bias", "out"]
    assert [sig.parameters[k].default for k in ("directions", "sets", "far", "table", "strength", "out")] == [256, 1, None, None, 1.0, None]
    sig = inspect.signature(Renderer.light_grid_bounces)
    assert list(sig.parameters) == ["self", "tables", "settings", "dims", "bounces", "bounds", "directions", "sets", "far", "mask_inside",
                                    "visibility", "strength"]
    assert [sig.parameters[k].default for k in ("bounces", "bounds", "directions", "sets", "far", "mask_inside", "visibility", "strength")] == \
        [2, None, 256, 1, None, 0.0, True, 1.0]
    sig = inspect.signature(Renderer.render_lit)
    assert list(sig.parameters) == ["self", "tables", "settings", "W", "H", "grid", "cameras", "strength"]
    assert list(inspect.signature(LightGrid.ref).parameters) == ["self", "strength", "facing", "visible", "normal_bias"]
    # the names that were there keep their signatures
    assert list(inspect.signature(Renderer.render_indirect).parameters) == ["self", "tables", "settings", "W", "H", "grid", "cameras", "strength"]
    assert list(inspect.signature(Renderer.shade_rays).parameters) == ["self", "tables", "settings", "rays", "far", "bright", "out", "out_bright"]
    assert list(inspect.signature(Renderer.light_probes).parameters) == ["self", "tables", "settings", "positions", "directions", "sets", "far",
                                                                         "table", "out"]


# ---------------------------------------------------------------- the refusals, all without a device
DEFAULT = object()
GRID = dict(probes=0x1000, depth=0x2000, dims=(4, 3, 2), origin=(0.0, 0.0, 0.0), step=(1.0, 1.0, 1.0), strength=1.0, flags=1, bias=0.1)


def grid_ref(**over):
    a = dict(GRID, **over)
    return abi.RmLightGridRef(a["probes"], a["depth"], (C.c_int32 * 3)(*a["dims"]), (C.c_float * 3)(*a["origin"]), (C.c_float * 3)(*a["step"]),
                              a["strength"], a["flags"], a["bias"])


def _ref_arg(grid):
    return None if grid is None else C.byref(grid_ref(**grid))


def shade(objs, no, lights, nl, g, s=DEFAULT, n=100, far=100.0, res=None, rays=FAKE, rgba=FAKE, grid=DEFAULT):
    s = abi.default_settings() if s is DEFAULT else s
    return lib().rm_shade_rays_indirect(rays, n, far, objs, no, lights, nl, C.byref(g) if g is not None else None,
                                        C.byref(s) if s is not None else None, C.byref(res) if res is not None else None,
                                        _ref_arg({} if grid is DEFAULT else grid), rgba, None)


def bake(objs, no, lights, nl, g, s=DEFAULT, n=100, K=16, sets=1, far=100.0, pos=FAKE, dirs=FAKE, out=FAKE, grid=DEFAULT):
    s = abi.default_settings() if s is DEFAULT else s
    return lib().rm_light_probes_indirect(pos, n, dirs, K, sets, far, objs, no, lights, nl, C.byref(g) if g is not None else None,
                                          C.byref(s) if s is not None else None, None, _ref_arg({} if grid is DEFAULT else grid), out, None)


BAD_GRID = dict(dims=(1, 1024, 1024), origin=(nan, 0, 0), step=(0.0, 1, 1), bias=nan, flags=6, probes=None, depth=0x2008, strength=nan)
GRID_STEPS = [  # each mends one field of BAD_GRID; the earliest check still violated answers
    ("dims", (1, 1024, 1024), "grid dimension"),
    ("dims", (1024, 1024, 1024), "RM_MAX_LIGHT_GRID_PROBES"),
    ("dims", (1024, 1024, 16), "origin must be finite"),
    ("origin", (0, -3e38, 0), "step must be finite and greater than 0"),
    ("step", (1e-30, 1, 3e38), "normalBias must be finite"),
    ("bias", -3e38, "flag bits"),
    ("flags", 1, "null d_probes"),
    ("probes", 0x1004, "16-byte aligned"),
    ("probes", 0x1000, "16-byte aligned"),
    ("depth", None, "strength must be finite"),
]


def test_the_order_of_the_shade_calls_checks():
    """Every check fails at the start; each step mends one, and the earliest check still violated answers: rm_shade_rays' own, the
    grid's in rm_light_grid_irradiance_visible's order with a null d_depth allowed, the strength, the device-memory checks."""
    objs, no, lights, nl, g = _scene()
    many = (abi.RmObject * (abi.RM_MAX_OBJECTS + 1))(*[h.make_object(abi.RM_SPHERE) for _ in range(abi.RM_MAX_OBJECTS + 1)])
    sea = abi.default_settings(features=abi.RM_FEAT_SEA)

    def run(a):
        return shade(a["objs"], a["no"], lights, nl, a["g"], s=a["s"], n=a["n"], far=a["far"], rays=a["rays"], rgba=a["rgba"], grid=a["grid"])

    start = dict(n=-1, objs=many, no=abi.RM_MAX_OBJECTS + 1, g=None, s=sea, far=-1.0, rays=None, rgba=fake(0x1004), grid=None)
    steps = [
        ({}, ah.INVALID, "negative numRays"),
        ({"n": INT_MAX}, ah.INVALID, "null scene pointer"),
        ({"g": h.make_globals(two_d=1)}, ah.INVALID, "far must be finite"),
        ({"far": 0.0}, UNSUPPORTED, "TERRAIN / CLOUD / SEA"),
        ({"s": abi.default_settings()}, UNSUPPORTED, "isTwoD"),
        ({"g": g}, CAPACITY, "RM_MAX_OBJECTS"),
        ({"objs": objs, "no": no}, ah.INVALID, "null d_rays or d_rgba"),
        ({"rays": HP}, ah.INVALID, "16-byte aligned"),
        ({"rgba": HP}, ah.INVALID, "null grid"),
    ]
    grid = dict(BAD_GRID)
    for key, value, word in GRID_STEPS:
        grid = dict(grid, **{key: value})
        steps.append(({"grid": grid}, ah.INVALID, word))
    steps.append(({"grid": dict(grid, strength=-3e38)}, ah.INVALID, "d_rays is not device-accessible"))  # the first check that asks the HIP runtime
    ah.walk(run, start, steps)


def test_the_order_of_the_bakes_checks():
    objs, no, lights, nl, g = _scene()
    sea = abi.default_settings(features=abi.RM_FEAT_SEA)

    def run(a):
        return bake(objs, no, lights, nl, a["g"], s=a["s"], n=a["n"], K=a["K"], sets=a["sets"], far=a["far"], pos=a["pos"], dirs=a["dirs"],
                    out=a["out"], grid=a["grid"])

    start = dict(n=-1, K=3, sets=0, far=nan, g=None, s=sea, pos=None, dirs=fake(0x1004), out=fake(0x1000), grid=None)
    steps = [
        ({}, ah.INVALID, "negative numProbes"),
        ({"n": INT_MAX}, ah.INVALID, "numDirs must be a power of two"),
        ({"K": 1024}, ah.INVALID, "numSets"),
        ({"sets": 4}, ah.INVALID, "INT_MAX"),
        ({"n": 24}, ah.INVALID, "null scene pointer"),
        ({"g": g}, ah.INVALID, "far must be finite"),
        ({"far": 3e38}, UNSUPPORTED, "TERRAIN / CLOUD / SEA"),
        ({"s": abi.default_settings()}, ah.INVALID, "null d_positions, d_dirs or d_out"),
        ({"pos": HP}, ah.INVALID, "16-byte aligned"),
        ({"dirs": HP}, ah.INVALID, "null grid"),
    ]
    grid = dict(BAD_GRID)
    for key, value, word in GRID_STEPS:
        grid = dict(grid, **{key: value})
        steps.append(({"grid": grid}, ah.INVALID, word))
    # the grid of (1024, 1024, 16) probes at 0x1000 spans 2.5 GiB: d_out at 0x1000 lies in it
    good = dict(grid, strength=0.5)
    steps.append(({"grid": good}, ah.INVALID, "overlaps the grid's probe records"))
    steps.append(({"grid": dict(good, dims=(2, 2, 2), probes=0x1000 + 24 * 160)}, ah.INVALID, "d_positions is not device-accessible"))
    ah.walk(run, start, steps)


def test_the_grid_strength_and_the_empty_calls():
    objs, no, lights, nl, g = _scene()
    for call in (lambda **kw: shade(objs, no, lights, nl, g, rays=HP, rgba=HP, **kw), lambda **kw: bake(objs, no, lights, nl, g, pos=HP, dirs=HP, out=HP, **kw)):
        assert refused(call(grid=None), "null grid")
        for d in ((1, 2, 2), (2, 0, 2), (1025, 2, 2), (2, 2, -1)):
            assert refused(call(grid=dict(dims=d, strength=nan)), "grid dimension"), d
        for d in ((1024, 1024, 17), (257, 256, 256)):
            assert refused(call(grid=dict(dims=d)), "RM_MAX_LIGHT_GRID_PROBES"), d
        for o in ah.BAD_ORIGINS:
            assert refused(call(grid=dict(origin=o, bias=nan)), "origin must be finite"), o
        for st in ah.BAD_STEPS:
            assert refused(call(grid=dict(step=st, bias=nan)), "step must be finite and greater than 0"), st
        for bias in (nan, inf, -inf):
            assert refused(call(grid=dict(bias=bias, flags=2, depth=None)), "normalBias must be finite"), bias  # checked without depth records too
        for flags in (2, 3, 0x80000000, 0xFFFFFFFE):
            assert refused(call(grid=dict(flags=flags, probes=None)), "flag bits other than RM_LIGHT_GRID_FACING"), flags
        assert refused(call(grid=dict(probes=None, strength=inf)), "null d_probes")
        for key in ("probes", "depth"):
            for off in (4, 8, 12, 1):
                assert refused(call(grid=dict({key: 0x1000 + off}, strength=nan)), "16-byte aligned"), (key, off)
        for strength in (nan, inf, -inf):
            assert refused(call(grid=dict(strength=strength)), "strength must be finite"), strength
        for strength in (0.0, -0.0, -1.0, 1e-45, 3e38):  # any finite strength, with and without depth records: on to the device checks
            for depth in (0x2000, None):
                assert refused(call(grid=dict(strength=strength, depth=depth)), "not device-accessible"), (strength, depth)
    # a call of no ray or no probe is RM_OK before the grid is looked at, as for rm_shade_rays and rm_light_probes: nothing is read
    assert shade(None, 5, None, -3, None, s=None, n=0, far=nan, rays=None, rgba=None, grid=None) == abi.RM_OK
    assert bake(None, 5, None, -3, None, s=None, n=0, far=nan, pos=None, dirs=None, out=None, grid=None) == abi.RM_OK
    assert refused(bake(objs, no, lights, nl, g, n=0, K=3, grid=None), "numDirs must be a power of two")  # the table's shape comes first
    # the scene comes before the grid
    assert refused(shade(objs, no, lights, nl, g, s=abi.default_settings(features=abi.RM_FEAT_CLOUD), grid=None), "TERRAIN / CLOUD / SEA", want=UNSUPPORTED)
    assert refused(bake(objs, no, lights, nl, g, s=abi.default_settings(features=abi.RM_FEAT_TERRAIN), grid=None), "TERRAIN / CLOUD / SEA", want=UNSUPPORTED)


def test_the_bakes_overlap_refusal():
    """[d_out, d_out + n·160) against the grid's dims[0]·dims[1]·dims[2] records of 160 bytes: any byte in common is refused, before
    the device is asked; buffers that only touch are not."""
    objs, no, lights, nl, g = _scene()
    n, count = 10, 4 * 3 * 2
    base = 0x100000

    def run(out, probes=base):
        return bake(objs, no, lights, nl, g, n=n, pos=HP, dirs=HP, out=fake(out), grid=dict(probes=probes))

    for out in (base, base + 160, base + (count - 1) * 160, base - (n - 1) * 160, base - 160 * n + 16):
        assert refused(run(out), "overlaps the grid's probe records"), hex(out)
    for out in (base + count * 160, base - n * 160, base + (1 << 30)):
        assert refused(run(out), "not device-accessible"), hex(out)
