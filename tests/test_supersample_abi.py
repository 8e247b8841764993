"""rm_render_supersampled without a GPU: the header declares it and carries the definition of a pixel (the order of the reduction),
the library exports it under the unchanged ABI version, every argument error returns its status before the first HIP call, and
Renderer.render_supersampled checks ss and lengths in Python."""
import ctypes as C
import os
import re

import pytest

import helpers as h
from raymarcher_amd import abi, lib
from raymarcher_amd._lib import LIB_PATH, SIGNATURES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "raymarcher_amd.h")).read()
INT_MAX = 2 ** 31 - 1


def test_header_declares_and_library_exports_the_entry_point():
    body = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    m = re.search(r"\bint\s+rm_render_supersampled\s*\(([^)]*)\)", body)
    assert m, "include/raymarcher_amd.h does not declare rm_render_supersampled"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 16 and params[12] == "int ss" and params[13] == "float *d_rgba"
    assert "rm_render_supersampled" in SIGNATURES
    res, args = SIGNATURES["rm_render_supersampled"]
    batch = SIGNATURES["rm_render_batch"][1]
    assert res is C.c_int and args == batch[:12] + [C.c_int] + batch[12:]  # rm_render_batch's arguments plus ss after H
    lib()
    assert hasattr(C.CDLL(LIB_PATH), "rm_render_supersampled")


def test_abi_version_stays_5():
    assert abi.RM_ABI_VERSION == 5
    assert re.search(r"#define\s+RM_ABI_VERSION\s+5\b", HEADER)
    assert lib().rm_abi_version() == 5


def test_header_comment_carries_the_definition_of_a_pixel():
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int\s+rm_render_supersampled\s*\(", HEADER, flags=re.S)
    assert m, "no comment in front of the declaration"
    text = re.sub(r"\s*\n\s*\*\s?", " ", m.group(1))
    for words in ("ss·W × ss·H", "x pairs first", "then y pairs", "a(x, y) = S(2x, y) + S(2x + 1, y)", "b(x, y) = a(x, 2y) + a(x, 2y + 1)",
                  "ss = 4 applies the level twice", "1.0f / (ss·ss)", "0.25f or 0.0625f", "binary32", "denormals kept",
                  "a = S[:, 0::2] + S[:, 1::2]; b = a[0::2] + a[1::2]", "ss == 1 is rm_render_batch",
                  "rm_debug_last_path() = 7", "symbol lookup", "before any HIP call"):
        assert words in text, f"the comment of rm_render_supersampled lacks: {words}"


def _batch(n, W=32, H=24):
    cams = (abi.RmCamera * max(n, 1))(*[h.make_camera((0, 0, 4.5), (0, 0, -1), (0, 1, 0), 30.0, W, H) for _ in range(max(n, 1))])
    globs = (abi.RmGlobals * max(n, 1))(*[h.make_globals(itime=0.1 * i) for i in range(max(n, 1))])
    scene = h.scene_mandelbulb(W, H)
    return cams, globs, scene


def call(cams, globs, num_globals, n, objs, num_objects, lights, num_lights, W=32, H=24, ss=2, out=None, s=None):
    s = s if s is not None else abi.default_settings()
    return lib().rm_render_supersampled(cams, globs, num_globals, n, objs, num_objects, lights, num_lights, C.byref(s), None, W, H, ss,
                                        out, None, None)


def refused(status, want=None):
    """The status is `want` (RM_ERR_INVALID_ARGUMENT by default) and rm_last_error() says why."""
    want = abi.RM_ERR_INVALID_ARGUMENT if want is None else want
    return status == want and len(lib().rm_last_error().decode()) > 0


def test_argument_errors_return_before_any_hip_call():
    L = lib()
    cams, globs, scene = _batch(3)
    objs, no, lights, nl = scene[1], scene[2], scene[3], scene[4]
    fake = C.c_void_p(0x1000)  # never dereferenced: every call below fails its checks first
    # ss outside {1, 2, 4}
    for ss in (0, 3, 8, -2, 5, 16):
        assert refused(call(cams, globs, 3, 3, objs, no, lights, nl, ss=ss, out=fake)), ss
        assert "ss" in L.rm_last_error().decode()
    for ss in (1, 2, 4):
        # numFrames == 0: nothing to write, a null output is fine
        assert call(cams, globs, 1, 0, objs, no, lights, nl, ss=ss, out=None) == abi.RM_OK, ss
        assert call(None, None, 0, 0, objs, no, lights, nl, ss=ss, out=None) == abi.RM_OK, ss
        # negative numFrames
        assert refused(call(cams, globs, 1, -1, objs, no, lights, nl, ss=ss, out=fake)), ss
        # numGlobals neither 1 nor numFrames
        for ng in (0, 2, 4, -1):
            assert refused(call(cams, globs, ng, 3, objs, no, lights, nl, ss=ss, out=fake)), (ss, ng)
        # null arrays
        assert refused(call(None, globs, 1, 3, objs, no, lights, nl, ss=ss, out=fake)), ss
        assert refused(call(cams, None, 1, 3, objs, no, lights, nl, ss=ss, out=fake)), ss
        # bad frame size
        for W, H in ((0, 24), (32, 0), (-5, 24), (32, -1)):
            assert refused(call(cams, globs, 3, 3, objs, no, lights, nl, W=W, H=H, ss=ss, out=fake)), (ss, W, H)
        # over the cap
        assert refused(call(cams, globs, 1, abi.RM_MAX_BATCH_FRAMES + 1, objs, no, lights, nl, ss=ss, out=fake), abi.RM_ERR_CAPACITY), ss
        # the tables are checked as rm_render_batch checks them: too many objects, null settings, null output
        many = (abi.RmObject * (abi.RM_MAX_OBJECTS + 1))(*[h.make_object(abi.RM_SPHERE) for _ in range(abi.RM_MAX_OBJECTS + 1)])
        assert refused(call(cams, globs, 3, 3, many, abi.RM_MAX_OBJECTS + 1, lights, nl, ss=ss, out=fake), abi.RM_ERR_CAPACITY), ss
        assert refused(L.rm_render_supersampled(cams, globs, 3, 3, objs, no, lights, nl, None, None, 32, 24, ss, fake, None, None)), ss
        assert refused(call(cams, globs, 3, 3, objs, no, lights, nl, ss=ss, out=None)), ss
        assert "null output" in L.rm_last_error().decode()


def test_sample_frames_too_large_are_refused_before_any_hip_call():
    cams, globs, scene = _batch(1)
    objs, no, lights, nl = scene[1], scene[2], scene[3], scene[4]
    fake = C.c_void_p(0x1000)
    for ss in (2, 4):
        over = INT_MAX // 8 // ss + 1  # ss·over > INT_MAX / 8
        assert refused(call(cams, globs, 1, 1, objs, no, lights, nl, W=over, H=8, ss=ss, out=fake)), ss
        assert refused(call(cams, globs, 1, 1, objs, no, lights, nl, W=8, H=over, ss=ss, out=fake)), ss
        # within INT_MAX / 8 on each axis, but more 8×8 sample tiles than one launch can index
        assert refused(call(cams, globs, 1, 1, objs, no, lights, nl, W=8, H=65536 * 8 // ss, ss=ss, out=fake)), ss
        assert refused(call(cams, globs, 1, 1, objs, no, lights, nl, W=INT_MAX // 8 // ss, H=32768, ss=ss, out=fake)), ss


def test_shared_argument_errors_report_in_precedence_order():
    """An input that violates several checks reports the earliest one.  The walk starts from a call that fails every check and
    mends them one at a time, in the order the entry point has checked them since it exists (statuses and words written down from
    the library before the multi-frame launchers shared one checking function)."""
    L = lib()
    cams, globs, scene = _batch(3)
    objs, no, lights, nl = scene[1], scene[2], scene[3], scene[4]
    many = (abi.RmObject * (abi.RM_MAX_OBJECTS + 1))(*[h.make_object(abi.RM_SPHERE) for _ in range(abi.RM_MAX_OBJECTS + 1)])
    for ss in (2, 4):
        a = dict(cams=None, globs=None, ng=2, n=-1, objs=many, no=abi.RM_MAX_OBJECTS + 1, W=0, H=0, ss=3, out=None)
        walk = [
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
        ]
        for step, (mend, status, word) in enumerate(walk):
            a.update(mend)
            got = call(a["cams"], a["globs"], a["ng"], a["n"], a["objs"], a["no"], lights, nl, W=a["W"], H=a["H"], ss=a["ss"], out=a["out"])
            assert got == status, (ss, step, mend, got, L.rm_last_error().decode())
            if word is not None:
                assert word in L.rm_last_error().decode(), (ss, step, mend, L.rm_last_error().decode())


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
