"""rm_render_batch without a GPU: the header declares it, the library exports it, and every argument error returns its status
before the first HIP call; Renderer.render_batch checks lengths in Python."""
import ctypes as C
import re

import pytest

import abi_helpers as ah
import helpers as h
import scene_builders as SB
from abi_helpers import FAKE, INT_MAX
from raymarcher_amd import abi, lib
from raymarcher_amd._lib import SIGNATURES


def test_header_declares_and_library_exports_the_batch_entry_point():
    assert ah.params("rm_render_batch")
    assert re.search(r"#define\s+RM_MAX_BATCH_FRAMES\s+1024\b", ah.HEADER_CODE)
    assert abi.RM_MAX_BATCH_FRAMES == 1024
    assert "rm_render_batch" in SIGNATURES
    ah.assert_exported(["rm_render_batch"])


def test_abi_version_is_5():
    ah.assert_abi_version()


def call(cams, globs, num_globals, n, objs, num_objects, lights, num_lights, W=32, H=24, out=None, s=None):
    s = s if s is not None else abi.default_settings()
    return lib().rm_render_batch(cams, globs, num_globals, n, objs, num_objects, lights, num_lights, C.byref(s), None, W, H,
                                 out, None, None)


def test_argument_errors_return_before_any_hip_call():
    L = lib()
    cams, globs, scene = SB.batch(3)
    objs, no, lights, nl = scene[1], scene[2], scene[3], scene[4]
    # numFrames == 0: nothing to write, a null output is fine
    assert call(cams, globs, 1, 0, objs, no, lights, nl, out=None) == abi.RM_OK
    assert call(None, None, 0, 0, objs, no, lights, nl, out=None) == abi.RM_OK
    # negative numFrames
    assert call(cams, globs, 1, -1, objs, no, lights, nl, out=FAKE) == abi.RM_ERR_INVALID_ARGUMENT
    # numGlobals neither 1 nor numFrames
    for ng in (0, 2, 4, -1):
        assert call(cams, globs, ng, 3, objs, no, lights, nl, out=FAKE) == abi.RM_ERR_INVALID_ARGUMENT, ng
    # null arrays
    assert call(None, globs, 1, 3, objs, no, lights, nl, out=FAKE) == abi.RM_ERR_INVALID_ARGUMENT
    assert call(cams, None, 1, 3, objs, no, lights, nl, out=FAKE) == abi.RM_ERR_INVALID_ARGUMENT
    # bad frame size
    for W, H in ((0, 24), (32, 0), (-5, 24), (32, -1)):
        assert call(cams, globs, 3, 3, objs, no, lights, nl, W=W, H=H, out=FAKE) == abi.RM_ERR_INVALID_ARGUMENT, (W, H)
    # over the cap
    assert call(cams, globs, 1, abi.RM_MAX_BATCH_FRAMES + 1, objs, no, lights, nl, out=FAKE) == abi.RM_ERR_CAPACITY
    # the tables are checked as rm_render_res checks them: too many objects, null settings, null output
    many = (abi.RmObject * (abi.RM_MAX_OBJECTS + 1))(*[h.make_object(abi.RM_SPHERE) for _ in range(abi.RM_MAX_OBJECTS + 1)])
    assert call(cams, globs, 3, 3, many, abi.RM_MAX_OBJECTS + 1, lights, nl, out=FAKE) == abi.RM_ERR_CAPACITY
    assert L.rm_render_batch(cams, globs, 3, 3, objs, no, lights, nl, None, None, 32, 24, FAKE, None, None) == abi.RM_ERR_INVALID_ARGUMENT
    assert call(cams, globs, 3, 3, objs, no, lights, nl, out=None) == abi.RM_ERR_INVALID_ARGUMENT
    assert "null output" in L.rm_last_error().decode()


def test_shared_argument_errors_report_in_precedence_order():
    """An input that violates several checks reports the earliest one.  The walk starts from a call that fails every shared check
    and mends them one at a time, in the order the entry point has checked them since it exists (statuses and words written down
    from the library before the multi-frame launchers shared one checking function)."""
    cams, globs, scene = SB.batch(3)
    objs, no, lights, nl = scene[1], scene[2], scene[3], scene[4]
    many = (abi.RmObject * (abi.RM_MAX_OBJECTS + 1))(*[h.make_object(abi.RM_SPHERE) for _ in range(abi.RM_MAX_OBJECTS + 1)])
    start = dict(cams=None, globs=None, ng=2, n=-1, objs=many, no=abi.RM_MAX_OBJECTS + 1, W=0, H=0, out=None)
    ah.walk(lambda a: call(a["cams"], a["globs"], a["ng"], a["n"], a["objs"], a["no"], lights, nl, W=a["W"], H=a["H"], out=a["out"]), start, [
        (dict(), abi.RM_ERR_INVALID_ARGUMENT, "negative numFrames"),
        (dict(n=abi.RM_MAX_BATCH_FRAMES + 1), abi.RM_ERR_CAPACITY, "RM_MAX_BATCH_FRAMES"),
        (dict(n=0), abi.RM_OK, None),  # nothing to write: whatever else is wrong
        (dict(n=3), abi.RM_ERR_INVALID_ARGUMENT, "numGlobals"),
        (dict(ng=3), abi.RM_ERR_INVALID_ARGUMENT, "null cameras or globals"),
        (dict(cams=cams), abi.RM_ERR_INVALID_ARGUMENT, "null cameras or globals"),
        (dict(globs=globs), abi.RM_ERR_INVALID_ARGUMENT, "bad frame size"),
        (dict(W=32), abi.RM_ERR_INVALID_ARGUMENT, "bad frame size"),
        # a batch has no sample frame: sizes that rm_render_supersampled refuses go on to the scene's checks
        (dict(W=INT_MAX // 8 + 1, H=65536 * 8), abi.RM_ERR_CAPACITY, "RM_MAX_OBJECTS"),
        (dict(W=32, H=24), abi.RM_ERR_CAPACITY, "RM_MAX_OBJECTS"),
        (dict(objs=objs, no=no), abi.RM_ERR_INVALID_ARGUMENT, "null output"),
    ])


def test_python_wrapper_checks_lengths():
    from raymarcher_amd.render import Renderer, SceneTables, batch_arrays
    W, H = 32, 24
    scene = h.scene_mandelbulb(W, H)
    cams = [h.make_camera((0, 0, 4.5 + 0.1 * i), (0, 0, -1), (0, 1, 0), 30.0, W, H) for i in range(3)]
    globs = [h.make_globals(itime=i) for i in range(3)]
    c, g = batch_arrays(cams, globs)
    assert len(c) == 3 and len(g) == 3 and g[2].iTime == 2.0
    c, g = batch_arrays(cams, globs[0])
    assert len(g) == 1
    r = Renderer.__new__(Renderer)  # no device is touched before the checks
    t = SceneTables(*scene)
    with pytest.raises(ValueError):
        r.render_batch(t, abi.default_settings(), W, H, cams, globals_=globs[:2])
    with pytest.raises(ValueError):
        r.render_batch(t, abi.default_settings(), W, H, cams, globals_=globs + globs[:1])
    with pytest.raises(ValueError):
        r.render_batch(t, abi.default_settings(), W, H, [(cams[0], None, None)])
    with pytest.raises(ValueError):
        batch_arrays(cams * 400, globs[0])  # 1200 > RM_MAX_BATCH_FRAMES
