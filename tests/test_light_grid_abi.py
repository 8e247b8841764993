"""rm_light_grid_irradiance without a GPU: the header declares it and the library exports it under the unchanged ABI version, the
record has 32 bytes, abi.py and _lib.py mirror the header, the header's comment carries the contract, every argument error returns
its status in the documented order before the first HIP call — with pointers that would fault if read —, and the Python layer has
its names.  The arithmetic is in tests/test_light_grid_spec.py, what needs the device in tests/test_gpu_light_grid.py."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

import abi_helpers as ah
from abi_helpers import FAKE, HEADER, HP, INT_MAX, fake, refused
from raymarcher_amd import abi, lib
from raymarcher_amd._lib import SIGNATURES

f32 = np.float32
inf, nan = float("inf"), float("nan")


# ---------------------------------------------------------------- the symbol and the written definition
def test_header_declares_and_library_exports_the_symbol():
    assert ah.params("rm_light_grid_irradiance") == [
        "const RmLightProbe *d_probes", "const int dims[3]", "const float origin[3]", "const float step[3]", "const float *d_points",
        "const float *d_normals", "int numPoints", "uint32_t flags", "RmGridLight *d_out", "void *stream"]
    Ptr = C.POINTER
    assert SIGNATURES["rm_light_grid_irradiance"] == (C.c_int, [C.c_void_p, Ptr(C.c_int), Ptr(C.c_float), Ptr(C.c_float), C.c_void_p, C.c_void_p,
                                                                C.c_int, C.c_uint32, C.c_void_p, C.c_void_p])
    ah.assert_exported(["rm_light_grid_irradiance"])
    assert not [n for n in ah.declared_functions() if n.startswith("rm_probe_") and "grid" in n], "rm_probe_* is the test probes' prefix"


def test_abi_version_stays_and_the_record_has_32_bytes():
    ah.assert_abi_version()
    assert C.sizeof(abi.RmGridLight) == 32
    assert [f[0] for f in abi.RmGridLight._fields_] == ["e", "weight", "probes", "reserved"]
    assert (abi.RmGridLight.e.offset, abi.RmGridLight.weight.offset, abi.RmGridLight.probes.offset, abi.RmGridLight.reserved.offset) == (0, 16, 20, 24)
    assert re.search(r"typedef struct RmGridLight \{ float e\[4\]; float weight; int32_t probes; int32_t reserved\[2\]; \} RmGridLight;\s*/\* 32 bytes \*/",
                     HEADER)
    for name, value in (("RM_LIGHT_GRID_FACING", "1u"), ("RM_MAX_LIGHT_GRID_DIM", "1024"), ("RM_MAX_LIGHT_GRID_PROBES", r"\(1 << 24\)")):
        assert re.search(rf"#define\s+{name}\s+{value}(?!\w)", HEADER), name
    assert (abi.RM_LIGHT_GRID_FACING, abi.RM_MAX_LIGHT_GRID_DIM, abi.RM_MAX_LIGHT_GRID_PROBES) == (1, 1024, 1 << 24)
    assert C.sizeof(abi.RmLightProbe) == 160 and abi.RmLightProbe.hits.offset == 144, "the records the entry consumes"


def test_header_comment_carries_the_contract():
    ah.assert_comment_has("RmGridLight", (
        "exactly as rm_light_probes stores them", "i + dims[0]·(j + dims[1]·k)", "origin_a + (float)index_a·step_a", "unfused",
        "Byte offsets are 64-bit", "ONE binary32 operation", "correctly rounded", "probes = RM_RAY_INVALID", "NOT normalised",
        "u_a = (p_a − origin_a) / step_a", "not greater than 0 becomes +0", "an infinite u_a clamps like any other", "takes the border's light",
        "cell_a = min((int)floor(u_a), dims_a − 2)", "f_a = u_a − (float)cell_a", "c = cx + 2·cy + 4·cz", "t_c = (wx·wy)·wz",
        "valid iff its hits >= 0", "only hits is read", "Majercik et al. 2019", "len == 0 gives face = 1",
        "cosv = ((dx·nx + dy·ny) + dz·nz) / len", "b = (cosv + 1)·0.5", "face = b·b + 0.2", "none of this is evaluated",
        "W = ((w0 + w1) + (w2 + w3)) + ((w4 + w5) + (w6 + w7))", "valid corners with w_c > 0", "probes == 0", "rounded once",
        "K0 = π·sqrt(1/4π)", "K1 = (2π/3)·sqrt(3/4π)", "K2 = (π/4)·sqrt(15/4π)", "K6 = (π/4)·sqrt(5/16π)", "K8 = (π/4)·sqrt(15/16π)",
        "k6 = K6·(3·(z·z) − 1)", "k8 = K8·(x·x − y·y)", "E_c[ch] = k0·sh[0][ch]", "e[ch] = T(w_c·E_c[ch]) / W", "leaf is +0", "not clamped",
        "sky visibility", "does not depend on which points share its call", "finite probe records", "before any HIP call",
        "Then numPoints == 0: RM_OK", "rm_debug_last_path() keeps its value", "nothing is allocated", "two 16-byte", "symbol lookup"))


def test_python_names():
    from raymarcher_amd import LightGrid, light_grid_positions
    from raymarcher_amd.render import Renderer
    assert list(inspect.signature(light_grid_positions).parameters) == ["origin", "step", "dims"]
    sig = inspect.signature(LightGrid.__init__)
    assert list(sig.parameters) == ["self", "renderer", "probes", "origin", "step", "dims"]
    sig = inspect.signature(LightGrid.irradiance)
    assert list(sig.parameters) == ["self", "points", "normals", "facing", "out"]
    assert sig.parameters["facing"].default is True and sig.parameters["out"].default is None
    sig = inspect.signature(LightGrid.light_gbuffer)
    assert list(sig.parameters) == ["self", "normal_depth", "position", "facing"] and sig.parameters["facing"].default is True
    sig = inspect.signature(Renderer.light_grid)
    assert list(sig.parameters) == ["self", "tables", "settings", "dims", "bounds", "directions", "sets", "far", "mask_inside"]
    assert [sig.parameters[k].default for k in ("bounds", "directions", "sets", "far", "mask_inside")] == [None, 256, 1, None, 0.0]
    sig = inspect.signature(Renderer.render_indirect)
    assert list(sig.parameters) == ["self", "tables", "settings", "W", "H", "grid", "cameras", "strength"]
    assert sig.parameters["cameras"].default is None and sig.parameters["strength"].default == 1.0
    assert "textures" in Renderer.render_indirect.__doc__ and "trap" in Renderer.render_indirect.__doc__
    # the positions are the entry's formula, x fastest, in float32
    o, s = np.array([-1.5, 0.1, 2.0], f32), np.array([0.3, 0.7, 1.1], f32)
    got = light_grid_positions(o, s, (3, 2, 4))
    assert got.shape == (24, 4) and got.dtype == f32 and (got[:, 3] == 0).all()
    for index in (0, 1, 3, 7, 23):
        i, j, k = index % 3, (index // 3) % 2, index // 6
        want = np.array([o[0] + f32(i) * s[0], o[1] + f32(j) * s[1], o[2] + f32(k) * s[2]], f32)
        assert (got[index, 0:3].view(np.uint32) == want.view(np.uint32)).all(), index
    with pytest.raises(ValueError):
        light_grid_positions(o, s, (1, 2, 2))


# ---------------------------------------------------------------- the refusals, all without a device
GOOD = dict(n=100, dims=(4, 3, 2), origin=(0.0, 0.0, 0.0), step=(1.0, 1.0, 1.0), flags=1, probes=FAKE, pts=FAKE, nrm=FAKE, out=FAKE)
ARRAYS = "null d_probes, d_points, d_normals or d_out"  # the first check behind numPoints == 0: a call that gets this far passed all before it


def call(**over):
    a = dict(GOOD, **over)
    dims = (C.c_int * 3)(*a["dims"]) if a["dims"] is not None else None
    return lib().rm_light_grid_irradiance(a["probes"], dims, ah.vec3(a["origin"]), ah.vec3(a["step"]), a["pts"], a["nrm"], a["n"], a["flags"],
                                          a["out"], None)


BAD_DIMS = ((1, 2, 2), (2, 0, 2), (2, 2, -1), (1025, 2, 2), (2, 2, 2 ** 31 - 1), (-2 ** 31, 2, 2), (1, 1, 1))
BIG_DIMS = ((1024, 1024, 17), (1024, 1024, 1024), (257, 256, 256), (1024, 129, 128))  # every axis in range, more than 2^24 probes
GOOD_DIMS = ((2, 2, 2), (1024, 2, 2), (2, 1024, 2), (2, 2, 1024), (256, 256, 256), (1024, 1024, 16), (1024, 128, 128))


def test_the_order_of_the_checks():
    """Every check fails at the start; each step mends one, and the earliest check still violated answers."""
    start = dict(n=-1, dims=None, origin=(nan, 0, 0), step=(0.0, 1, 1), flags=6, probes=None, pts=fake(0x1004), nrm=HP, out=HP)
    ah.walk(lambda a: call(**a), start, [
        ({}, ah.INVALID, "negative numPoints"),
        ({"n": INT_MAX}, ah.INVALID, "null dims, origin or step"),
        ({"dims": (1, 1024, 1024)}, ah.INVALID, "grid dimension"),
        ({"dims": (1024, 1024, 1024)}, ah.INVALID, "RM_MAX_LIGHT_GRID_PROBES"),
        ({"dims": (1024, 1024, 16)}, ah.INVALID, "origin must be finite"),
        ({"origin": (0, -3e38, 0)}, ah.INVALID, "step must be finite and greater than 0"),
        ({"step": (1e-30, 1, 3e38)}, ah.INVALID, "flag bits"),
        ({"flags": 1}, ah.INVALID, ARRAYS),
        ({"probes": HP}, ah.INVALID, "16-byte aligned"),
        ({"pts": HP}, ah.INVALID, "d_probes is not device-accessible"),  # host memory is not device memory: the only check that asks the HIP runtime, and the last
    ])


def test_counts_and_the_grid():
    for n in (-1, -INT_MAX, -2 ** 31):
        assert refused(call(n=n), "negative numPoints"), n
        assert refused(call(n=n, dims=None, flags=2), "negative numPoints"), n
    assert refused(call(dims=None), "null dims, origin or step")
    assert refused(call(origin=None), "null dims, origin or step") and refused(call(step=None), "null dims, origin or step")
    assert refused(call(origin=None, n=0, dims=(1, 1, 1)), "null dims, origin or step")  # before the dimensions and the empty call
    for d in BAD_DIMS:
        assert refused(call(dims=d), "grid dimension must be 2 … RM_MAX_LIGHT_GRID_DIM"), d
        assert refused(call(dims=d, origin=(nan, 0, 0), n=0), "grid dimension"), d  # before the origin and the empty call
    for d in BIG_DIMS:
        assert refused(call(dims=d), "RM_MAX_LIGHT_GRID_PROBES"), d
        assert refused(call(dims=d, step=(0, 1, 1), n=0), "RM_MAX_LIGHT_GRID_PROBES"), d
    for o in ah.BAD_ORIGINS:
        assert refused(call(origin=o), "origin must be finite"), o
        assert refused(call(origin=o, step=(-1, 1, 1), n=0), "origin"), o
    for st in ah.BAD_STEPS:
        assert refused(call(step=st), "step must be finite and greater than 0"), st
        assert refused(call(step=st, flags=2, n=0), "step"), st
    for flags in (2, 3, 4, 0x80000000, 0xFFFFFFFF, 0xFFFFFFFE):
        assert refused(call(flags=flags), "flag bits other than RM_LIGHT_GRID_FACING"), flags
        assert refused(call(flags=flags, n=0, probes=None), "flag bits"), flags  # before the empty call
    # numPoints == 0: RM_OK with null arrays, nothing is read
    for d in GOOD_DIMS:
        for flags in (0, 1):
            assert call(n=0, dims=d, flags=flags, probes=None, pts=None, nrm=None, out=None) == abi.RM_OK, (d, flags)
            assert call(n=0, dims=d, flags=flags, probes=fake(0x1004), pts=fake(0x1008), nrm=fake(1), out=fake(3)) == abi.RM_OK, (d, flags)
    # every valid grid and every int numPoints gets as far as the arrays
    for d in GOOD_DIMS:
        assert refused(call(dims=d, out=None), ARRAYS), d
    for n in (1, 255, 256, 257, INT_MAX):
        assert refused(call(n=n, pts=None), ARRAYS), n
    for o, st in (((-3e38, 3e38, -0.0), (1e-38, 3e38, 1.0)), ((0.0, 0.0, 0.0), (1e-45, 1.0, 1.0))):
        assert refused(call(origin=o, step=st, nrm=None), ARRAYS), (o, st)


def test_the_four_arrays():
    for key in ("probes", "pts", "nrm", "out"):
        assert refused(call(**{key: None}), ARRAYS), key
    for off in (4, 8, 12, 1):
        bad = fake(0x1000 + off)
        for key in ("probes", "pts", "nrm", "out"):
            assert refused(call(**{key: bad}), "16-byte aligned"), (key, off)
    assert refused(call(pts=None, probes=fake(0x1004)), ARRAYS)  # null before misaligned
    # host memory is not device memory: the only check that asks the HIP runtime, and the last
    assert refused(call(probes=HP, pts=HP, nrm=HP, out=HP), "d_probes")
