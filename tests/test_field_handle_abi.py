"""RmField handles without a GPU: the header declares the five entry points and the library exports them under the unchanged ABI
version, the Python layer has its methods, and every refusal of the two creates returns its status before the first HIP call — with
pointers that would fault if read — in the order the header states, leaving *field NULL.  What needs a live handle is in
tests/test_gpu_field_handle.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np

from raymarcher_amd import abi, lib
from raymarcher_amd._lib import LIB_PATH, SIGNATURES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "raymarcher_amd.h")).read()
INVALID = abi.RM_ERR_INVALID_ARGUMENT
FAKE = C.c_void_p(0x1000)  # never dereferenced: every call that gets it fails its checks first
inf, nan = float("inf"), float("nan")
NAMES = {"rm_field_create": 8, "rm_field_create_blocks": 11, "rm_field_destroy": 1, "rm_field_sample": 5, "rm_field_trace": 8}
HOST = np.zeros(4096, dtype=np.float32)
HP = C.c_void_p(HOST.ctypes.data)  # aligned host memory: it gets as far as the device-memory check
assert HOST.ctypes.data % 16 == 0


def _params(name):
    body = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    m = re.search(r"\b(?:int|void)\s+" + name + r"\s*\(([^)]*)\)", body)
    assert m, f"include/raymarcher_amd.h does not declare {name}"
    return [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]


def test_header_declares_and_library_exports_the_symbols():
    lattice = ["const float origin[3]", "const float step[3]"]
    assert _params("rm_field_create") == ["const float *d_dist", "const int32_t *d_objectId", "int nx", "int ny", "int nz"] + lattice + ["RmField **field"]
    assert _params("rm_field_create_blocks") == (["const float *d_dist", "const int32_t *d_objectId", "const int32_t *d_blocks", "int numBlocks",
                                                  "int mx", "int my", "int mz"] + lattice + ["void *stream", "RmField **field"])
    assert _params("rm_field_destroy") == ["RmField *field"]
    assert _params("rm_field_sample") == ["const RmField *field", "const float *d_points", "int numPoints", "RmFieldSample *d_samples", "void *stream"]
    assert _params("rm_field_trace") == ["const RmField *field", "const RmRay *d_rays", "int numRays", "float iso", "int maxSteps", "unsigned mode",
                                         "RmRayHit *d_hits", "void *stream"]
    assert HEADER.index("typedef struct RmField RmField;") > HEADER.index("int rm_sdf_trace_blocks(")
    lib()
    L = C.CDLL(LIB_PATH)
    for name, n in NAMES.items():
        assert hasattr(L, name), f"the library does not export {name}"
        assert name in SIGNATURES and len(SIGNATURES[name][1]) == n == len(_params(name))
        assert SIGNATURES[name][0] is (None if name == "rm_field_destroy" else C.c_int)


def test_abi_version_stays_and_the_header_carries_the_definition():
    assert abi.RM_ABI_VERSION == 5 and lib().rm_abi_version() == 5
    assert re.search(r"#define\s+RM_ABI_VERSION\s+5\b", HEADER)
    assert re.search(r"#define\s+RM_FIELD_PENUMBRA_K\s+8\.0f", HEADER) and abi.RM_FIELD_PENUMBRA_K == 8.0
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*typedef struct RmField RmField;", HEADER, flags=re.S)
    assert m, "no comment in front of RmField"
    text = re.sub(r"\s*\n\s*\*\s?", " ", m.group(1))
    for w in ("counts samples only", "borrows", "consumes d_blocks", "not the kWsBlocks workspace", "rm_set_workspace_limit", "q < res ? q : res",
              "best effort", "another device current", "a ray that never sampled stores 1", "at most mx + my + mz long",
              "equal in every word", "*field = NULL on every failure", "Then a count of 0: RM_OK", "rm_debug_last_path() keeps its value"):
        assert w in text, f"the header's definition lacks: {w}"


def test_python_signatures():
    from raymarcher_amd import LatticeField
    from raymarcher_amd.render import Renderer
    sig = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert sig(Renderer.lattice_field) == ["self", "grid", "origin", "step", "ids"]
    assert sig(Renderer.lattice_field_blocks) == ["self", "grid_blocks", "block_list", "blocks", "origin", "step", "ids"]
    assert sig(Renderer.scene_field) == sig(Renderer.scene_field_sparse)
    assert inspect.signature(Renderer.scene_field).parameters["iso"].default == 0.001
    assert sig(LatticeField.sample) == ["self", "points"]
    assert sig(LatticeField.trace) == ["self", "rays", "iso", "max_steps", "mode", "normals", "out"]
    p = inspect.signature(LatticeField.trace).parameters
    assert (p["iso"].default, p["max_steps"].default, p["mode"].default, p["normals"].default, p["out"].default) == (0.001, 256, "closest", True, None)
    for name in ("close", "__enter__", "__exit__", "__del__"):
        assert callable(getattr(LatticeField, name))


def refused(status, text=None):
    msg = lib().rm_last_error().decode()
    return status == INVALID and len(msg) > 0 and (text is None or text in msg)


def vec(v):
    return (C.c_float * 3)(*v) if v is not None else None


SENTINEL = 0xDEAD0


def create(dist=FAKE, ids=FAKE, dims=(4, 3, 2), origin=(0, 0, 0), step=(0.1, 0.1, 0.1), field=True):
    """(status, whether *field is NULL afterwards)"""
    h = C.c_void_p(SENTINEL)
    st = lib().rm_field_create(dist, ids, dims[0], dims[1], dims[2], vec(origin), vec(step), C.byref(h) if field else None)
    assert not field or h.value is None, "*field is NULL after a failure"
    return st


def create_blocks(dist=FAKE, ids=FAKE, bl=FAKE, nb=3, dims=(2, 2, 2), origin=(0, 0, 0), step=(0.1, 0.1, 0.1), field=True):
    h = C.c_void_p(SENTINEL)
    st = lib().rm_field_create_blocks(dist, ids, bl, nb, dims[0], dims[1], dims[2], vec(origin), vec(step), None, C.byref(h) if field else None)
    assert not field or h.value is None, "*field is NULL after a failure"
    return st


BAD_STEPS = ((nan, 1, 1), (1, inf, 1), (1, 1, 0.0), (-0.5, 1, 1), (1, -0.0, 1), (1, 1, -inf))
BAD_ORIGINS = ((nan, 0, 0), (0, inf, 0), (0, 0, -inf))
BAD_DIMS = ((0, 2, 2), (2, -1, 2), (4097, 2, 2), (2, 2, 2 ** 31 - 1), (-2 ** 31, 2, 2))
ONE_DIMS = ((1, 2, 2), (2, 1, 2), (2, 2, 1), (1, 1, 1), (4096, 4096, 1))
BAD_BLOCKS = ((0, 2, 2), (2, -1, 2), (2, 2, 0), (513, 1, 1), (1, 513, 1), (1, 1, 2 ** 31 - 1), (-2 ** 31, 2, 2))
BAD_COUNTS = (-1, -2 ** 31, (1 << 22) + 1, 2 ** 31 - 1)


def _lattice_refusals(call, dense):
    """rm_sdf_sample's / rm_sdf_sample_blocks' refusals about the lattice, in their order and with their messages."""
    assert refused(call(origin=None), "null origin or step") and refused(call(step=None), "null origin or step")
    assert refused(call(origin=None, field=False), "null origin or step")  # the lattice comes before the null field
    for o in BAD_ORIGINS:
        assert refused(call(origin=o), "origin must be finite"), o
    for st in BAD_STEPS:
        assert refused(call(step=st), "step must be finite and greater than 0"), st
        assert refused(call(origin=(nan, 0, 0), step=st), "origin"), st
    if dense:
        for d in BAD_DIMS:
            assert refused(call(dims=d), "lattice dimension must be 1 … RM_MAX_LATTICE_DIM"), d
            assert refused(call(dims=d, step=(0, 1, 1)), "step"), d
        assert refused(call(dims=(4096, 4096, 4096)), "more than INT_MAX lattice points")
        for d in ONE_DIMS:
            assert refused(call(dims=d), "at least 2"), d
            assert refused(call(dims=d, field=False), "at least 2"), d
    else:
        for b in BAD_BLOCKS:
            assert refused(call(dims=b), "block dimension"), b
            assert refused(call(dims=b, step=(0, 1, 1)), "step"), b
        for nb in BAD_COUNTS:
            assert refused(call(nb=nb), "numBlocks must be 0 … RM_MAX_BLOCK_LIST"), nb
            assert refused(call(nb=nb, dims=(0, 1, 1)), "block dimension"), nb  # the lattice comes before numBlocks
            assert refused(call(nb=nb, field=False), "numBlocks"), nb           # numBlocks before the null field


def _pointer_refusals(call):
    assert refused(call(field=False), "null field")
    assert refused(call(field=False, dist=None), "null field")  # the null field comes before the arrays
    assert refused(call(dist=None), "null d_dist")
    assert refused(call(dist=None, ids=C.c_void_p(0x1002)), "null d_dist")  # null comes before misaligned
    for k in ("dist", "ids"):
        assert refused(call(**{k: C.c_void_p(0x1002)}), "misaligned"), k
    assert refused(call(dist=HP, ids=None), "d_dist is not device-accessible")
    assert refused(call(dist=HP, ids=C.c_void_p(0x1002)), "misaligned")  # misaligned comes before the device-memory check


def test_create_refusals_in_order():
    _lattice_refusals(create, True)
    _pointer_refusals(create)
    assert refused(create(dims=(2, 2, 2), dist=HP, ids=None), "d_dist is not device-accessible")  # the smallest lattice is valid


def test_create_blocks_refusals_in_order_and_the_empty_list():
    _lattice_refusals(create_blocks, False)
    _pointer_refusals(create_blocks)
    assert refused(create_blocks(bl=None), "null d_blocks with numBlocks above 0")
    assert refused(create_blocks(bl=None, dist=None), "null d_dist")  # d_dist before d_blocks
    assert refused(create_blocks(bl=C.c_void_p(0x1002)), "misaligned")
    assert refused(create_blocks(nb=1 << 22, dims=(512, 512, 512), dist=HP, ids=None), "d_dist is not device-accessible")  # the largest are valid
    assert refused(create_blocks(dist=HP, ids=None, bl=HP), "d_dist is not device-accessible")
    # an empty list needs neither values nor a list: nothing is left to refuse before the HIP calls, which need a device
    assert refused(create_blocks(nb=0, bl=FAKE, dist=HP, ids=None), "d_dist is not device-accessible")  # d_blocks is not looked at


def test_destroy_null_is_a_no_op_and_queries_refuse_a_null_handle():
    assert lib().rm_field_destroy(None) is None
    assert refused(lib().rm_field_sample(None, FAKE, 5, FAKE, None), "null or stale RmField handle")
    assert refused(lib().rm_field_sample(None, FAKE, -1, FAKE, None), "handle")  # the handle comes before the count
    assert refused(lib().rm_field_sample(None, None, 0, None, None), "handle")   # and before the empty call
    assert refused(lib().rm_field_trace(None, FAKE, 5, 0.0, 64, 0, FAKE, None), "null or stale RmField handle")
    assert refused(lib().rm_field_trace(None, FAKE, 5, nan, -1, 7, FAKE, None), "handle")
    assert refused(lib().rm_field_trace(None, None, 0, 0.0, 64, 2, None, None), "handle")
