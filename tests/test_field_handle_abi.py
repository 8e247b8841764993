"""RmField handles without a GPU: the header declares the five entry points and the library exports them under the unchanged ABI
version, the Python layer has its methods, and every refusal of the two creates returns its status before the first HIP call — with
pointers that would fault if read — in the order the header states, leaving *field NULL.  What needs a live handle is in
tests/test_gpu_field_handle.py."""
import ctypes as C
import inspect
import re

import abi_helpers as ah
from abi_helpers import FAKE, HEADER, HP, fake, nan, refused, vec3 as vec
from raymarcher_amd import abi, lib
from raymarcher_amd._lib import SIGNATURES

NAMES = {"rm_field_create": 8, "rm_field_create_blocks": 11, "rm_field_destroy": 1, "rm_field_sample": 5, "rm_field_trace": 8}


def _params(name):
    return ah.params(name, "void" if name == "rm_field_destroy" else "int")


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
    ah.assert_exported(NAMES)
    for name, n in NAMES.items():
        assert name in SIGNATURES and len(SIGNATURES[name][1]) == n == len(_params(name))
        assert SIGNATURES[name][0] is (None if name == "rm_field_destroy" else C.c_int)


def test_abi_version_stays_and_the_header_carries_the_definition():
    ah.assert_abi_version()
    assert re.search(r"#define\s+RM_FIELD_PENUMBRA_K\s+8\.0f", HEADER) and abi.RM_FIELD_PENUMBRA_K == 8.0
    ah.assert_comment_has("RmField RmField;", (
        "counts samples only", "borrows", "consumes d_blocks", "not the kWsBlocks workspace", "rm_set_workspace_limit", "q < res ? q : res",
        "best effort", "another device current", "a ray that never sampled stores 1", "at most mx + my + mz long",
        "equal in every word", "*field = NULL on every failure", "Then a count of 0: RM_OK", "rm_debug_last_path() keeps its value"))


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


def _pointer_refusals(call):
    assert refused(call(field=False), "null field")
    assert refused(call(field=False, dist=None), "null field")  # the null field comes before the arrays
    assert refused(call(dist=None), "null d_dist")
    assert refused(call(dist=None, ids=fake(0x1002)), "null d_dist")  # null comes before misaligned
    for k in ("dist", "ids"):
        assert refused(call(**{k: fake(0x1002)}), "misaligned"), k
    assert refused(call(dist=HP, ids=None), "d_dist is not device-accessible")
    assert refused(call(dist=HP, ids=fake(0x1002)), "misaligned")  # misaligned comes before the device-memory check


def test_create_refusals_in_order():
    ah.lattice_refusals(create, True, still=dict(field=False))  # rm_sdf_sample's, all before the null field
    _pointer_refusals(create)
    assert refused(create(dims=(2, 2, 2), dist=HP, ids=None), "d_dist is not device-accessible")  # the smallest lattice is valid


def test_create_blocks_refusals_in_order_and_the_empty_list():
    ah.lattice_refusals(create_blocks, False, still=dict(field=False))  # rm_sdf_sample_blocks', numBlocks too
    _pointer_refusals(create_blocks)
    assert refused(create_blocks(bl=None), "null d_blocks with numBlocks above 0")
    assert refused(create_blocks(bl=None, dist=None), "null d_dist")  # d_dist before d_blocks
    assert refused(create_blocks(bl=fake(0x1002)), "misaligned")
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
