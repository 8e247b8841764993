"""rm_render_supersampled without a GPU: the header declares it and carries the definition of a pixel (the order of the reduction),
the library exports it under the unchanged ABI version, every argument error returns its status before the first HIP call, and
Renderer.render_supersampled checks ss and lengths in Python."""
import ctypes as C

import pytest

import abi_helpers as ah
import helpers as h
import scene_builders as SB
from abi_helpers import FAKE, INT_MAX, refused
from raymarcher_amd import abi, lib
from raymarcher_amd._lib import SIGNATURES


def test_header_declares_and_library_exports_the_entry_point():
    params = ah.params("rm_render_supersampled")
    assert len(params) == 16 and params[12] == "int ss" and params[13] == "float *d_rgba"
    assert "rm_render_supersampled" in SIGNATURES
    res, args = SIGNATURES["rm_render_supersampled"]
    batch = SIGNATURES["rm_render_batch"][1]
    assert res is C.c_int and args == batch[:12] + [C.c_int] + batch[12:]  # rm_render_batch's arguments plus ss after H
    ah.assert_exported(["rm_render_supersampled"])


def test_abi_version_stays_5():
    ah.assert_abi_version()


def test_header_comment_carries_the_definition_of_a_pixel():
    ah.assert_comment_has("rm_render_supersampled", (
        "ss·W × ss·H", "x pairs first", "then y pairs", "a(x, y) = S(2x, y) + S(2x + 1, y)", "b(x, y) = a(x, 2y) + a(x, 2y + 1)",
        "ss = 4 applies the level twice", "1.0f / (ss·ss)", "0.25f or 0.0625f", "binary32", "denormals kept",
        "a = S[:, 0::2] + S[:, 1::2]; b = a[0::2] + a[1::2]", "ss == 1 is rm_render_batch",
        "rm_debug_last_path() = 7", "symbol lookup", "before any HIP call"))


def call(cams, globs, num_globals, n, objs, num_objects, lights, num_lights, W=32, H=24, ss=2, out=None, s=None):
    s = s if s is not None else abi.default_settings()
    return lib().rm_render_supersampled(cams, globs, num_globals, n, objs, num_objects, lights, num_lights, C.byref(s), None, W, H, ss,
                                        out, None, None)


def test_argument_errors_return_before_any_hip_call():
    L = lib()
    cams, globs, scene = SB.batch(3)
    objs, no, lights, nl = scene[1], scene[2], scene[3], scene[4]
    # ss outside {1, 2, 4}
    for ss in (0, 3, 8, -2, 5, 16):
        assert refused(call(cams, globs, 3, 3, objs, no, lights, nl, ss=ss, out=FAKE), "ss"), ss
    for ss in (1, 2, 4):
        # numFrames == 0: nothing to write, a null output is fine
        assert call(cams, globs, 1, 0, objs, no, lights, nl, ss=ss, out=None) == abi.RM_OK, ss
        assert call(None, None, 0, 0, objs, no, lights, nl, ss=ss, out=None) == abi.RM_OK, ss
        # negative numFrames
        assert refused(call(cams, globs, 1, -1, objs, no, lights, nl, ss=ss, out=FAKE)), ss
        # numGlobals neither 1 nor numFrames
        for ng in (0, 2, 4, -1):
            assert refused(call(cams, globs, ng, 3, objs, no, lights, nl, ss=ss, out=FAKE)), (ss, ng)
        # null arrays
        assert refused(call(None, globs, 1, 3, objs, no, lights, nl, ss=ss, out=FAKE)), ss
        assert refused(call(cams, None, 1, 3, objs, no, lights, nl, ss=ss, out=FAKE)), ss
        # bad frame size
        for W, H in ((0, 24), (32, 0), (-5, 24), (32, -1)):
            assert refused(call(cams, globs, 3, 3, objs, no, lights, nl, W=W, H=H, ss=ss, out=FAKE)), (ss, W, H)
        # over the cap
        assert refused(call(cams, globs, 1, abi.RM_MAX_BATCH_FRAMES + 1, objs, no, lights, nl, ss=ss, out=FAKE), want=abi.RM_ERR_CAPACITY), ss
        # the tables are checked as rm_render_batch checks them: too many objects, null settings, null output
        many = (abi.RmObject * (abi.RM_MAX_OBJECTS + 1))(*[h.make_object(abi.RM_SPHERE) for _ in range(abi.RM_MAX_OBJECTS + 1)])
        assert refused(call(cams, globs, 3, 3, many, abi.RM_MAX_OBJECTS + 1, lights, nl, ss=ss, out=FAKE), want=abi.RM_ERR_CAPACITY), ss
        assert refused(L.rm_render_supersampled(cams, globs, 3, 3, objs, no, lights, nl, None, None, 32, 24, ss, FAKE, None, None)), ss
        assert refused(call(cams, globs, 3, 3, objs, no, lights, nl, ss=ss, out=None), "null output"), ss


def test_sample_frames_too_large_are_refused_before_any_hip_call():
    cams, globs, scene = SB.batch(1)
    objs, no, lights, nl = scene[1], scene[2], scene[3], scene[4]
    for ss in (2, 4):
        over = INT_MAX // 8 // ss + 1  # ss·over > INT_MAX / 8
        assert refused(call(cams, globs, 1, 1, objs, no, lights, nl, W=over, H=8, ss=ss, out=FAKE)), ss
        assert refused(call(cams, globs, 1, 1, objs, no, lights, nl, W=8, H=over, ss=ss, out=FAKE)), ss
        # within INT_MAX / 8 on each axis, but more 8×8 sample tiles than one launch can index
        assert refused(call(cams, globs, 1, 1, objs, no, lights, nl, W=8, H=65536 * 8 // ss, ss=ss, out=FAKE)), ss
        assert refused(call(cams, globs, 1, 1, objs, no, lights, nl, W=INT_MAX // 8 // ss, H=32768, ss=ss, out=FAKE)), ss


def test_shared_argument_errors_report_in_precedence_order():
    """An input that violates several checks reports the earliest one.  The walk starts from a call that fails every check and
    mends them one at a time, in the order the entry point has checked them since it exists (statuses and words written down from
    the library before the multi-frame launchers shared one checking function)."""
    cams, globs, scene = SB.batch(3)
    objs, no, lights, nl = scene[1], scene[2], scene[3], scene[4]
    many = (abi.RmObject * (abi.RM_MAX_OBJECTS + 1))(*[h.make_object(abi.RM_SPHERE) for _ in range(abi.RM_MAX_OBJECTS + 1)])

    def walked(a):
        return call(a["cams"], a["globs"], a["ng"], a["n"], a["objs"], a["no"], lights, nl, W=a["W"], H=a["H"], ss=a["ss"], out=a["out"])

    for ss in (2, 4):
        start = dict(cams=None, globs=None, ng=2, n=-1, objs=many, no=abi.RM_MAX_OBJECTS + 1, W=0, H=0, ss=3, out=None)
        ah.walk(walked, start, [
            (dict(), abi.RM_ERR_INVALID_ARGUMENT, "ss (samples per pixel"),
            (dict(ss=ss), abi.RM_ERR_INVALID_ARGUMENT, "negative numFrames"),
            (dict(n=abi.RM_MAX_BATCH_FRAMES + 1), abi.RM_ERR_CAPACITY, "RM_MAX_BATCH_FRAMES"),
            (dict(n=0), abi.RM_OK, None),  # nothing to write: whatever else is wrong
            (dict(n=3), abi.RM_ERR_INVALID_ARGUMENT, "numGlobals"),
            (dict(ng=3), abi.RM_ERR_INVALID_ARGUMENT, "null cameras or globals"),
            (dict(cams=cams), abi.RM_ERR_INVALID_ARGUMENT, "null cameras or globals"),
            (dict(globs=globs), abi.RM_ERR_INVALID_ARGUMENT, "bad frame size"),
            (dict(W=INT_MAX // 8 // ss + 1), abi.RM_ERR_INVALID_ARGUMENT, "bad frame size"),  # H = 0 still
            (dict(H=65536 * 8 // ss), abi.RM_ERR_INVALID_ARGUMENT, "INT_MAX / 8"),             # too wide and too many tiles
            (dict(W=8), abi.RM_ERR_INVALID_ARGUMENT, "too many samples"),
            (dict(W=32, H=24), abi.RM_ERR_CAPACITY, "RM_MAX_OBJECTS"),
            (dict(objs=objs, no=no), abi.RM_ERR_INVALID_ARGUMENT, "null output"),
        ])


def test_python_wrapper_checks_ss_and_lengths():
    from raymarcher_amd.render import Renderer, SceneTables
    W, H = 32, 24
    scene = h.scene_mandelbulb(W, H)
    cams = [h.make_camera((0, 0, 4.5 + 0.1 * i), (0, 0, -1), (0, 1, 0), 30.0, W, H) for i in range(3)]
    globs = [h.make_globals(itime=i) for i in range(3)]
    r = Renderer.__new__(Renderer)  # no device is touched before the checks
    t = SceneTables(*scene)
    for ss in (0, 3, 8, -2, 2.5, None):
        with pytest.raises(ValueError):
            r.render_supersampled(t, abi.default_settings(), W, H, cams, ss)
    with pytest.raises(ValueError):
        r.render_supersampled(t, abi.default_settings(), W, H, cams, 2, globals_=globs[:2])
    with pytest.raises(ValueError):
        r.render_sequence(t, abi.default_settings(), W, H, cams, supersample=3)
