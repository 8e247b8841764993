"""rm_sdf_sample, rm_sdf_sample_blocks, rm_sdf_trace and rm_sdf_trace_blocks without a GPU: the header declares them and the library
exports them under the unchanged ABI version, the Python layer has its methods, and every refusal returns its status before the
first HIP call — with pointers that would fault if read — in the order the header states."""
import ctypes as C
import inspect
import re

import abi_helpers as ah
from abi_helpers import FAKE, HEADER, HP, fake, inf, nan, refused, vec3 as vec
from raymarcher_amd import abi, lib
from raymarcher_amd._lib import SIGNATURES

NAMES = {"rm_sdf_sample": 11, "rm_sdf_sample_blocks": 13, "rm_sdf_trace": 14, "rm_sdf_trace_blocks": 16}


def test_header_declares_and_library_exports_the_four_symbols():
    dense = ["const float *d_dist", "const int32_t *d_objectId", "int nx", "int ny", "int nz", "const float origin[3]", "const float step[3]"]
    sparse = ["const float *d_dist", "const int32_t *d_objectId", "const int32_t *d_blocks", "int numBlocks", "int mx", "int my", "int mz",
              "const float origin[3]", "const float step[3]"]
    march = ["float iso", "int maxSteps", "unsigned mode", "RmRayHit *d_hits", "void *stream"]
    assert ah.params("rm_sdf_sample") == ["const float *d_points", "int numPoints"] + dense + ["RmFieldSample *d_samples", "void *stream"]
    assert ah.params("rm_sdf_sample_blocks") == ["const float *d_points", "int numPoints"] + sparse + ["RmFieldSample *d_samples", "void *stream"]
    assert ah.params("rm_sdf_trace") == ["const RmRay *d_rays", "int numRays"] + dense + march
    assert ah.params("rm_sdf_trace_blocks") == ["const RmRay *d_rays", "int numRays"] + sparse + march
    ah.assert_exported(NAMES)
    for name, n in NAMES.items():
        assert name in SIGNATURES and SIGNATURES[name][0] is C.c_int and len(SIGNATURES[name][1]) == n == len(ah.params(name))


def test_abi_version_stays_and_the_header_carries_the_definitions():
    ah.assert_abi_version()
    assert C.sizeof(abi.RmFieldSample) == 32 and "} RmFieldSample; /* 32 bytes */" in HEADER
    assert [f[0] for f in abi.RmFieldSample._fields_] == ["gradient", "value", "cell", "objectId"]
    assert abi.RmFieldSample.value.offset == 12 and abi.RmFieldSample.cell.offset == 16 and abi.RmFieldSample.objectId.offset == 28
    assert re.search(r"#define\s+RM_FIELD_OUTSIDE\s+\(-5\)", HEADER) and abi.RM_FIELD_OUTSIDE == -5
    assert re.search(r"#define\s+RM_FIELD_UNLISTED\s+\(-6\)", HEADER) and abi.RM_FIELD_UNLISTED == -6
    assert re.search(r"#define\s+RM_MAX_FIELD_STEPS\s+65536\b", HEADER) and abi.RM_MAX_FIELD_STEPS == 65536
    ah.assert_comment_has("RmFieldSample", (
        "never fused", "a NaN clamps to lo", "lerp(a, b, w) = a + w·(b − a)", "(fx >= 0.5, fy >= 0.5, fz >= 0.5)", "RM_FIELD_UNLISTED",
        "ud all zeros", "Every skip changes an integer block coordinate", "knows nothing about the inside of unlisted blocks",
        "the first listed sample below iso, not t = 0", "before any HIP call", "rm_set_workspace_limit", "rebuilt on every call",
        "rm_debug_last_path() keeps its value"))


def test_python_signatures():
    from raymarcher_amd.render import Renderer
    sig = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert sig(Renderer.sample_lattice) == ["self", "grid", "origin", "step", "points", "ids"]
    assert sig(Renderer.sample_lattice_blocks) == ["self", "grid_blocks", "block_list", "blocks", "origin", "step", "points", "ids"]
    assert sig(Renderer.trace_lattice) == ["self", "grid", "origin", "step", "rays", "iso", "max_steps", "ids", "normals", "out"]
    assert sig(Renderer.trace_lattice_blocks) == ["self", "grid_blocks", "block_list", "blocks", "origin", "step", "rays", "iso", "max_steps",
                                                  "ids", "normals", "out"]
    for f in (Renderer.trace_lattice, Renderer.trace_lattice_blocks):
        p = inspect.signature(f).parameters
        assert (p["iso"].default, p["max_steps"].default, p["ids"].default, p["normals"].default) == (0.001, 256, None, True)
    assert sig(Renderer.scene_field_sparse) == sig(Renderer.scene_mesh_sparse)
    assert inspect.signature(Renderer.scene_field_sparse).parameters["iso"].default == 0.001


def sample(n=5, points=FAKE, dist=FAKE, ids=FAKE, dims=(4, 3, 2), origin=(0, 0, 0), step=(0.1, 0.1, 0.1), out=FAKE):
    return lib().rm_sdf_sample(points, n, dist, ids, dims[0], dims[1], dims[2], vec(origin), vec(step), out, None)


def sample_blocks(n=5, points=FAKE, dist=FAKE, ids=FAKE, bl=FAKE, nb=3, dims=(2, 2, 2), origin=(0, 0, 0), step=(0.1, 0.1, 0.1), out=FAKE):
    return lib().rm_sdf_sample_blocks(points, n, dist, ids, bl, nb, dims[0], dims[1], dims[2], vec(origin), vec(step), out, None)


def trace(n=5, rays=FAKE, dist=FAKE, ids=FAKE, dims=(4, 3, 2), origin=(0, 0, 0), step=(0.1, 0.1, 0.1), iso=0.0, steps=64, mode=0, out=FAKE):
    return lib().rm_sdf_trace(rays, n, dist, ids, dims[0], dims[1], dims[2], vec(origin), vec(step), iso, steps, mode, out, None)


def trace_blocks(n=5, rays=FAKE, dist=FAKE, ids=FAKE, bl=FAKE, nb=3, dims=(2, 2, 2), origin=(0, 0, 0), step=(0.1, 0.1, 0.1), iso=0.0, steps=64,
                 mode=0, out=FAKE):
    return lib().rm_sdf_trace_blocks(rays, n, dist, ids, bl, nb, dims[0], dims[1], dims[2], vec(origin), vec(step), iso, steps, mode, out, None)


def _lattice_refusals(call, dense, first):
    """What all four refuse alike up to the lattice, in order; first: the name of the count's message."""
    for n in (-1, -2 ** 31):
        assert refused(call(n=n), f"negative {first}"), n
        assert refused(call(n=n, origin=None), f"negative {first}"), n  # the count comes first
    ah.lattice_refusals(call, dense, still=dict(n=0))  # a call of nothing is still checked


def _array_refusals(call, inp, out, what):
    """Behind the numeric checks: a count of 0 is RM_OK with nothing read; null, misaligned and host arrays are refused."""
    assert call(n=0) == abi.RM_OK
    assert call(n=0, **{inp: None, out: None}, dist=None, ids=None) == abi.RM_OK
    assert refused(call(**{inp: None}), f"null {what}") and refused(call(**{out: None}), f"null {what}")
    assert refused(call(dist=None), f"null {what}")
    for k in (inp, out):
        assert refused(call(**{k: fake(0x1008)}), "misaligned"), k
    for k in ("dist", "ids"):
        assert refused(call(**{k: fake(0x1002)}), "misaligned"), k
    assert refused(call(**{inp: None, "dist": fake(0x1002)}), f"null {what}")  # null comes before misaligned
    name = {"points": "d_points", "rays": "d_rays"}[inp]
    assert refused(call(**{inp: HP, out: HP}, dist=HP, ids=None), f"{name} is not device-accessible")


def _march_refusals(call, lattice_bad):
    for iso in (nan, inf, -inf):
        assert refused(call(iso=iso), "iso must be finite"), iso
        assert refused(call(iso=iso, **lattice_bad), "dimension"), iso  # the lattice comes before iso
        assert refused(call(iso=iso, steps=-1), "iso"), iso             # iso before maxSteps
    for steps in (-1, 65537, 2 ** 31 - 1, -2 ** 31):
        assert refused(call(steps=steps), "maxSteps must be 0 … RM_MAX_FIELD_STEPS"), steps
        assert refused(call(steps=steps, mode=2), "maxSteps"), steps    # maxSteps before the mode
    for mode in (2, 3, 4, 0x80000000):
        assert refused(call(mode=mode), "mode bits other than RM_TRACE_NO_NORMAL"), mode
        assert refused(call(mode=mode, n=0), "mode bits"), mode         # before the empty call
        assert refused(call(mode=mode, rays=None), "mode bits"), mode   # and before the arrays
    for steps in (0, 65536):
        for mode in (0, 1):
            assert refused(call(steps=steps, mode=mode, out=None), "null d_rays, d_hits or d_dist")


def test_sample_refusals_in_order():
    _lattice_refusals(sample, True, "numPoints")
    _array_refusals(sample, "points", "out", "d_points, d_samples or d_dist")


def test_sample_blocks_refusals_in_order_and_the_empty_list():
    _lattice_refusals(sample_blocks, False, "numPoints")
    _array_refusals(sample_blocks, "points", "out", "d_points, d_samples or d_dist")
    assert refused(sample_blocks(bl=None), "null d_blocks with numBlocks above 0")
    assert refused(sample_blocks(bl=fake(0x1002)), "misaligned")
    assert refused(sample_blocks(nb=1 << 22, dims=(512, 512, 512), out=None), "null d_points")  # the largest lattice and list are valid
    # an empty list is valid and needs neither values nor a list: it gets as far as the device-memory check
    assert refused(sample_blocks(nb=0, bl=None, dist=None, ids=None, points=HP, out=HP), "d_points is not device-accessible")


def test_trace_refusals_in_order():
    _lattice_refusals(trace, True, "numRays")
    _march_refusals(trace, dict(dims=(1, 2, 2)))
    _array_refusals(trace, "rays", "out", "d_rays, d_hits or d_dist")


def test_trace_blocks_refusals_in_order_and_the_empty_list():
    _lattice_refusals(trace_blocks, False, "numRays")
    _march_refusals(trace_blocks, dict(dims=(0, 2, 2)))
    assert refused(trace_blocks(nb=-1, iso=nan), "numBlocks")  # numBlocks before iso
    _array_refusals(trace_blocks, "rays", "out", "d_rays, d_hits or d_dist")
    assert refused(trace_blocks(bl=None), "null d_blocks with numBlocks above 0")
    assert refused(trace_blocks(nb=0, bl=None, dist=None, ids=None, rays=HP, out=HP), "d_rays is not device-accessible")
