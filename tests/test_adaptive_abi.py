"""rm_render_adaptive without a GPU: the header declares it and carries the definition of a pixel (the contrast test), the library
exports it under the unchanged ABI version, every argument error returns its status before the first HIP call, Renderer.render_adaptive
checks ss, the threshold and lengths in Python, and `adaptive` below — the definition in NumPy, which the GPU tests import — agrees
with the same rule written out per pixel."""
import ctypes as C

import numpy as np
import pytest

import abi_helpers as ah
import helpers as h
import scene_builders as SB
from abi_helpers import FAKE, INT_MAX, refused
from raymarcher_amd import abi, lib
from raymarcher_amd._lib import SIGNATURES


# ---------------------------------------------------------------- the definition in NumPy
def contrast_mask(F, thr):
    """M of the header: (H, W, 4) float32 frame → (H, W) bool.  A pixel is flagged when r, g or b differs from a 4-neighbour inside
    the frame by more than thr — "not (|a − b| <= thr)", so that a NaN difference flags both pixels."""
    F = np.asarray(F)
    assert F.dtype == np.float32 and F.ndim == 3 and F.shape[2] == 4
    thr = np.float32(thr)
    c = F[..., :3]
    with np.errstate(invalid="ignore"):  # inf − inf = NaN is part of the rule
        dx = (~(np.abs(c[:, 1:] - c[:, :-1]) <= thr)).any(-1)
        dy = (~(np.abs(c[1:] - c[:-1]) <= thr)).any(-1)
    m = np.zeros(F.shape[:2], dtype=bool)
    m[:, 1:] |= dx
    m[:, :-1] |= dx
    m[1:] |= dy
    m[:-1] |= dy
    return m


def adaptive(F, Fb, R, Rb, thr):
    """The definition: the 1-sample frame (F, Fb), the supersampled frame (R, Rb), the threshold → (out, bright, mask)."""
    m = contrast_mask(F, thr)
    return np.where(m[..., None], R, F), np.where(m[..., None], Rb, Fb), m


def _per_pixel(F, Fb, R, Rb, thr):
    """The same rule, pixel by pixel, channel by channel, every subtraction one binary32 operation."""
    f = np.float32
    H, W = F.shape[:2]
    out, br, mask = F.copy(), Fb.copy(), np.zeros((H, W), dtype=bool)
    for Y in range(H):
        for X in range(W):
            flagged = False
            for NX, NY in ((X - 1, Y), (X + 1, Y), (X, Y - 1), (X, Y + 1)):
                if NX < 0 or NX >= W or NY < 0 or NY >= H:
                    continue
                for c in range(3):
                    with np.errstate(invalid="ignore"):
                        d = f(abs(f(F[Y, X, c] - F[NY, NX, c])))
                    if not (d <= f(thr)):
                        flagged = True
            mask[Y, X] = flagged
            if flagged:
                out[Y, X] = R[Y, X]
                br[Y, X] = Rb[Y, X]
    return out, br, mask


def test_numpy_definition_equals_the_rule_written_out_per_pixel():
    rng = np.random.default_rng(11)
    f = np.float32
    for (H, W), thr in (((9, 13), 0.1), ((1, 1), 0.0), ((1, 7), 0.25), ((6, 1), 0.05), ((8, 8), 0.0), ((7, 9), np.inf), ((6, 7), -1.0),
                        ((10, 11), 0.125)):
        F = (rng.random((H, W, 4)) * 0.3).astype(f)
        F[..., 3] = rng.random((H, W)).astype(f) * 50  # alpha is not looked at
        if H >= 6 and W >= 6:
            F[2, 3, 0] = np.inf
            F[2, 4, 0] = np.inf          # inf − inf: a NaN difference
            F[4, 1, 1] = -np.inf
            F[5, 5, 2] = np.nan
            F[0, 0, :3] = 0.0
            F[0, 1, :3] = f(1e-45)       # a denormal difference: flagged at threshold 0, not above
            F[1, 0, :3] = 0.0
            F[3, 2, :3] = f(0.5)
            F[3, 3, :3] = f(0.5) + f(thr if np.isfinite(thr) and thr > 0 else 0.25)  # a difference exactly equal to the threshold
            F[4, 3, :3] = F[3, 3, :3]
            F[2, 2, :3] = f(0.5)
            F[2, 3, 1:3] = F[3, 3, 1:3]
        Fb, R, Rb = (rng.standard_normal((H, W, 4)).astype(f) for _ in range(3))
        got = adaptive(F, Fb, R, Rb, thr)
        exp = _per_pixel(F, Fb, R, Rb, thr)
        assert (got[2] == exp[2]).all(), (H, W, thr)
        assert (got[0].view(np.uint32) == exp[0].view(np.uint32)).all() and (got[1].view(np.uint32) == exp[1].view(np.uint32)).all()
        if H * W == 1:
            assert not got[2].any()  # no neighbour: never flagged
        elif thr < 0:
            assert got[2].all()
    # what the planted values must do
    F = np.zeros((2, 3, 4), dtype=f)
    F[0, 1, 0] = f(1e-45)
    assert contrast_mask(F, 0.0).tolist() == [[True, True, True], [False, True, False]]
    assert not contrast_mask(F, 1e-45).any()  # equal to the threshold: not flagged
    F[0, 1, 0] = f(0.25)
    assert not contrast_mask(F, 0.25).any() and contrast_mask(F, np.nextafter(f(0.25), f(0))).sum() == 4
    F[...] = np.inf
    assert contrast_mask(F, np.inf).all()  # inf − inf is NaN: flagged even at +inf
    F[...] = 1.0
    F[..., 3] = np.arange(6, dtype=f).reshape(2, 3)
    assert not contrast_mask(F, 0.0).any()  # alpha differs, r, g, b do not


# ---------------------------------------------------------------- header, library, bindings
PARAMS = ["const RmCamera *cams", "const RmGlobals *globals", "int numGlobals", "int numFrames", "const RmObject *objs", "int numObjects",
          "const RmLight *lights", "int numLights", "const RmSettings *s", "const RmResources *res", "int W", "int H", "int ss",
          "float threshold", "float *d_rgba", "float *d_bright", "uint8_t *d_mask", "uint32_t *d_refined", "void *stream"]


def test_header_declares_and_library_exports_the_entry_point():
    params = ah.params("rm_render_adaptive")
    assert len(params) == 19 and params == PARAMS
    assert "rm_render_adaptive" in SIGNATURES
    res, args = SIGNATURES["rm_render_adaptive"]
    ssig = SIGNATURES["rm_render_supersampled"][1]
    # rm_render_supersampled's arguments plus the threshold after ss and the two outputs after d_bright
    assert res is C.c_int and args == ssig[:13] + [C.c_float] + ssig[13:15] + [C.c_void_p, C.c_void_p] + ssig[15:]
    ah.assert_exported(["rm_render_adaptive"])


def test_abi_version_stays_5():
    ah.assert_abi_version()


def test_header_comment_carries_the_definition_of_a_pixel():
    ah.assert_comment_has("rm_render_adaptive", (
        "4-neighbour", "inside the frame", "not (", "<= threshold", "r, g, b", "rm_render_batch", "rm_render_supersampled",
        "rm_debug_last_path() = 8", "before any HIP call", "symbol lookup", "binary32", "denormals kept", "NaN difference",
        "d_mask", "d_refined", "rm_set_workspace_limit"))


# ---------------------------------------------------------------- argument errors
def call(cams, globs, num_globals, n, objs, num_objects, lights, num_lights, W=32, H=24, ss=2, thr=0.1, out=None, s=None, mask=None,
         refined=None):
    s = s if s is not None else abi.default_settings()
    return lib().rm_render_adaptive(cams, globs, num_globals, n, objs, num_objects, lights, num_lights, C.byref(s), None, W, H, ss, thr,
                                    out, None, mask, refined, None)


def test_argument_errors_return_before_any_hip_call():
    L = lib()
    cams, globs, scene = SB.batch(3)
    objs, no, lights, nl = scene[1], scene[2], scene[3], scene[4]
    # a NaN threshold, with and without the optional outputs
    for ss in (1, 2, 4):
        assert refused(call(cams, globs, 3, 3, objs, no, lights, nl, ss=ss, thr=float("nan"), out=FAKE), "threshold"), ss
        assert refused(call(cams, globs, 3, 3, objs, no, lights, nl, ss=ss, thr=float("nan"), out=FAKE, mask=FAKE, refined=FAKE)), ss
    # ss outside {1, 2, 4}
    for ss in (0, 3, 8, -2, 5, 16):
        assert refused(call(cams, globs, 3, 3, objs, no, lights, nl, ss=ss, out=FAKE), "ss"), ss
    for ss in (1, 2, 4):
        for thr in (0.1, float("inf"), -1.0):
            # numFrames == 0: nothing to write, a null output is fine
            assert call(cams, globs, 1, 0, objs, no, lights, nl, ss=ss, thr=thr, out=None) == abi.RM_OK, ss
            assert call(None, None, 0, 0, objs, no, lights, nl, ss=ss, thr=thr, out=None) == abi.RM_OK, ss
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
        assert refused(L.rm_render_adaptive(cams, globs, 3, 3, objs, no, lights, nl, None, None, 32, 24, ss, 0.1, FAKE, None, None, None,
                                            None)), ss
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
    # more pixels per frame than a 32-bit list entry indexes, whatever ss
    for ss in (1, 2, 4):
        assert refused(call(cams, globs, 1, 1, objs, no, lights, nl, W=65536, H=32768, ss=ss, out=FAKE)), ss


def test_shared_argument_errors_report_in_precedence_order():
    """An input that violates several checks reports the earliest one.  The walk starts from a call that fails every check and
    mends them one at a time, in the order the entry point has checked them since it exists (statuses and words written down from
    the library before the multi-frame launchers shared one checking function).  ss = 1 included: the entry point holds the
    1-sample frame to the sample frame's bounds too."""
    cams, globs, scene = SB.batch(3)
    objs, no, lights, nl = scene[1], scene[2], scene[3], scene[4]
    many = (abi.RmObject * (abi.RM_MAX_OBJECTS + 1))(*[h.make_object(abi.RM_SPHERE) for _ in range(abi.RM_MAX_OBJECTS + 1)])

    def walked(a):
        return call(a["cams"], a["globs"], a["ng"], a["n"], a["objs"], a["no"], lights, nl, W=a["W"], H=a["H"], ss=a["ss"], thr=a["thr"],
                    out=a["out"])

    for ss in (1, 2, 4):
        start = dict(cams=None, globs=None, ng=2, n=-1, objs=many, no=abi.RM_MAX_OBJECTS + 1, W=0, H=0, ss=3, thr=float("nan"), out=None)
        ah.walk(walked, start, [
            (dict(), abi.RM_ERR_INVALID_ARGUMENT, "ss (samples per pixel"),
            (dict(ss=ss), abi.RM_ERR_INVALID_ARGUMENT, "threshold is NaN"),
            (dict(thr=0.1), abi.RM_ERR_INVALID_ARGUMENT, "negative numFrames"),
            (dict(n=abi.RM_MAX_BATCH_FRAMES + 1), abi.RM_ERR_CAPACITY, "RM_MAX_BATCH_FRAMES"),
            (dict(n=0), abi.RM_OK, None),  # nothing to write: whatever else is wrong
            (dict(n=3), abi.RM_ERR_INVALID_ARGUMENT, "numGlobals"),
            (dict(ng=3), abi.RM_ERR_INVALID_ARGUMENT, "null cameras or globals"),
            (dict(cams=cams), abi.RM_ERR_INVALID_ARGUMENT, "null cameras or globals"),
            (dict(globs=globs), abi.RM_ERR_INVALID_ARGUMENT, "bad frame size"),
            (dict(W=INT_MAX // 8 // ss + 1), abi.RM_ERR_INVALID_ARGUMENT, "bad frame size"),  # H = 0 still
            (dict(H=32768), abi.RM_ERR_INVALID_ARGUMENT, "INT_MAX / 8"),                       # too wide, too many tiles and pixels
            (dict(W=INT_MAX // 8 // ss), abi.RM_ERR_INVALID_ARGUMENT, "too many samples"),     # too many tiles and pixels
            (dict(W=65536), abi.RM_ERR_INVALID_ARGUMENT, "list entry"),                        # 2^31 pixels, with a bad table
            (dict(W=32, H=24), abi.RM_ERR_CAPACITY, "RM_MAX_OBJECTS"),
            (dict(objs=objs, no=no), abi.RM_ERR_INVALID_ARGUMENT, "null output"),
        ])


def test_python_wrapper_checks_ss_threshold_and_lengths():
    from raymarcher_amd.render import Renderer, SceneTables
    W, H = 32, 24
    scene = h.scene_mandelbulb(W, H)
    cams = [h.make_camera((0, 0, 4.5 + 0.1 * i), (0, 0, -1), (0, 1, 0), 30.0, W, H) for i in range(3)]
    globs = [h.make_globals(itime=i) for i in range(3)]
    r = Renderer.__new__(Renderer)  # no device is touched before the checks
    t = SceneTables(*scene)
    for ss in (0, 3, 8, -2, 2.5, None):
        with pytest.raises(ValueError):
            r.render_adaptive(t, abi.default_settings(), W, H, cams, ss, 0.1)
    for ss in (1, 2, 4):
        with pytest.raises(ValueError):
            r.render_adaptive(t, abi.default_settings(), W, H, cams, ss, float("nan"))
        with pytest.raises(ValueError):
            r.render_adaptive(t, abi.default_settings(), W, H, cams, ss, np.float32("nan"))
    with pytest.raises(ValueError):
        r.render_adaptive(t, abi.default_settings(), W, H, cams, 2, 0.1, globals_=globs[:2])
    with pytest.raises(ValueError):
        r.render_sequence(t, abi.default_settings(), W, H, cams, supersample=3, adaptive=0.1)
    with pytest.raises(ValueError):
        r.render_sequence(t, abi.default_settings(), W, H, cams, supersample=2, adaptive=float("nan"))
