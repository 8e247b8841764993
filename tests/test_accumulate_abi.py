"""rm_render_accumulated and its lens helpers without a GPU: the header declares them and carries the definition of a pixel (the
order of the sum), the library exports them under the unchanged ABI version, every argument error returns its status before the
first HIP call, the scenefile's lens fields come back from the loader, and the lens cameras focus where they should."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import abi_helpers as ah
import helpers as h
import scene_builders as SB
from abi_helpers import FAKE, HEADER, INT_MAX, refused
from raymarcher_amd import abi, lib
from raymarcher_amd._lib import SIGNATURES


# ---------------------------------------------------------------- the entry point
def test_header_declares_and_library_exports_the_entry_point():
    params = ah.params("rm_render_accumulated")
    assert len(params) == 16 and params[3] == "int numFrames" and params[4] == "int subFrames" and params[13] == "float *d_rgba"
    res, args = SIGNATURES["rm_render_accumulated"]
    batch = SIGNATURES["rm_render_batch"][1]
    assert res is C.c_int and args == batch[:4] + [C.c_int] + batch[4:]  # rm_render_batch's arguments plus subFrames after numFrames
    names = ("rm_render_accumulated", "rm_camera_lens_samples", "rm_scene_camera_lens")
    ah.assert_exported(names)
    for name in names:
        assert name in SIGNATURES and ah.params(name), name


def test_abi_version_and_struct_sizes_stay():
    ah.assert_abi_version()
    assert abi.RM_MAX_SUBFRAMES == 64 and re.search(r"#define\s+RM_MAX_SUBFRAMES\s+64\b", HEADER)
    assert lib().rm_abi_sizeof(7) == C.sizeof(abi.RmCameraData) == 52  # the lens fields did not go into RmCameraData


def test_header_comment_carries_the_definition_of_a_pixel():
    ah.assert_comment_has("rm_render_accumulated", (
        "cams[f·subFrames + j]", "acc = S_0", "acc = acc + S_j", "in that order", "binary32", "denormals kept",
        "1.0f / (float)n", "acc = S[0].copy()", "out = acc * (np.float32(1) / np.float32(n))",
        "subFrames == 1 is rm_render_batch", "no subFrames-sized image exists in device memory", "RM_MAX_SUBFRAMES",
        "rm_debug_last_path() = 9", "symbol lookup", "before any HIP call"))


def call(cams, globs, num_globals, n, sub, objs, num_objects, lights, num_lights, W=32, H=24, out=None, s=None):
    s = s if s is not None else abi.default_settings()
    return lib().rm_render_accumulated(cams, globs, num_globals, n, sub, objs, num_objects, lights, num_lights, C.byref(s), None, W, H,
                                       out, None, None)


def test_argument_errors_return_before_any_hip_call():
    """Null or FAKE device pointers throughout: no call below may reach HIP (this machine has no device to reach)."""
    L = lib()
    cams, globs, scene = SB.batch(12)
    objs, no, lights, nl = scene[1], scene[2], scene[3], scene[4]
    # subFrames outside 1 … RM_MAX_SUBFRAMES
    for sub in (0, -1, -64, abi.RM_MAX_SUBFRAMES + 1, 1000, INT_MAX):
        assert refused(call(cams, globs, 1, 1, sub, objs, no, lights, nl, out=FAKE), "subFrames"), sub
    # numFrames·subFrames over the ring's cap: RM_ERR_CAPACITY, also where neither factor is over it and where the product
    # would not fit an int
    for n, sub in ((abi.RM_MAX_BATCH_FRAMES + 1, 1), (abi.RM_MAX_BATCH_FRAMES // 64 + 1, 64), (513, 2), (INT_MAX, 64)):
        assert refused(call(cams, globs, 1, n, sub, objs, no, lights, nl, out=FAKE), "RM_MAX_BATCH_FRAMES", want=abi.RM_ERR_CAPACITY), (n, sub)
    for sub in (1, 3, 4):
        n = 12 // sub
        # numFrames == 0: nothing to write, a null output is fine
        assert call(cams, globs, 1, 0, sub, objs, no, lights, nl, out=None) == abi.RM_OK, sub
        assert call(None, None, 0, 0, sub, objs, no, lights, nl, out=None) == abi.RM_OK, sub
        # negative numFrames
        assert refused(call(cams, globs, 1, -1, sub, objs, no, lights, nl, out=FAKE)), sub
        # numGlobals neither 1 nor numFrames·subFrames (numFrames alone is not enough)
        for ng in (0, 2, 13, -1) + ((n,) if sub > 1 else ()):
            assert refused(call(cams, globs, ng, n, sub, objs, no, lights, nl, out=FAKE), "numGlobals"), (sub, ng)
        # null arrays
        assert refused(call(None, globs, 1, n, sub, objs, no, lights, nl, out=FAKE)), sub
        assert refused(call(cams, None, 1, n, sub, objs, no, lights, nl, out=FAKE)), sub
        # bad frame size
        for W, H in ((0, 24), (32, 0), (-5, 24), (32, -1), (INT_MAX // 8 + 1, 8), (8, 65536 * 8)):
            assert refused(call(cams, globs, 12, n, sub, objs, no, lights, nl, W=W, H=H, out=FAKE)), (sub, W, H)
        # the tables are checked as rm_render_batch checks them: too many objects, null settings, null output
        many = (abi.RmObject * (abi.RM_MAX_OBJECTS + 1))(*[h.make_object(abi.RM_SPHERE) for _ in range(abi.RM_MAX_OBJECTS + 1)])
        assert refused(call(cams, globs, 12, n, sub, many, abi.RM_MAX_OBJECTS + 1, lights, nl, out=FAKE), want=abi.RM_ERR_CAPACITY), sub
        assert refused(L.rm_render_accumulated(cams, globs, 12, n, sub, objs, no, lights, nl, None, None, 32, 24, FAKE, None, None)), sub
        assert refused(call(cams, globs, 12, n, sub, objs, no, lights, nl, out=None), "null output"), sub


def test_argument_errors_report_in_the_order_of_the_header():
    """An input that violates several checks reports the earliest: subFrames, the cap on numFrames·subFrames, numFrames == 0,
    numGlobals, then rm_render_batch's own."""
    cams, globs, scene = SB.batch(6)
    objs, no, lights, nl = scene[1], scene[2], scene[3], scene[4]
    start = dict(cams=None, globs=None, ng=2, n=abi.RM_MAX_BATCH_FRAMES, sub=0, W=0, H=0, out=None)
    ah.walk(lambda a: call(a["cams"], a["globs"], a["ng"], a["n"], a["sub"], objs, no, lights, nl, W=a["W"], H=a["H"], out=a["out"]), start, [
        (dict(), abi.RM_ERR_INVALID_ARGUMENT, "subFrames"),
        (dict(sub=2), abi.RM_ERR_CAPACITY, "RM_MAX_BATCH_FRAMES"),
        (dict(n=0), abi.RM_OK, None),
        (dict(n=3), abi.RM_ERR_INVALID_ARGUMENT, "numGlobals"),
        (dict(ng=6), abi.RM_ERR_INVALID_ARGUMENT, "null cameras or globals"),
        (dict(cams=cams, globs=globs), abi.RM_ERR_INVALID_ARGUMENT, "bad frame size"),
        (dict(W=32, H=24), abi.RM_ERR_INVALID_ARGUMENT, "null output"),
    ])


# ---------------------------------------------------------------- the scenefile's lens fields
def test_scene_camera_lens_returns_the_fields_of_the_scenefile():
    from raymarcher_amd import Scene
    sc = Scene(path=os.path.join(SB.SCENES, "lighting", "depth_of_field.json"))
    a, f = sc.lens()
    assert np.float32(a) == np.float32(0.008) and np.float32(f) == np.float32(3.0)
    cd = sc.camera_data()  # untouched by the lens fields
    assert (cd.pos[0], cd.pos[1], cd.pos[2]) == (0.0, 0.0, 16.0) and (cd.look[0], cd.look[1], cd.look[2]) == (0.0, 0.0, -1.0)
    assert Scene(path=os.path.join(SB.SCENES, "lighting", "directional_light_2.json")).lens() == (0.0, 0.0)
    one = '{"name": "root", "globalData": {"ambientCoeff": 1, "diffuseCoeff": 1, "specularCoeff": 1}, "cameraData": {"position": ' \
          '[0, 0, 5], "up": [0, 1, 0], "heightAngle": 30, "look": [0, 0, -1], "focalLength": 2.5}, "groups": []}'
    assert Scene(text=one).lens() == (0.0, 2.5)
    L = lib()
    x = C.c_float()
    assert L.rm_scene_camera_lens(None, C.byref(x), C.byref(x)) == abi.RM_ERR_INVALID_ARGUMENT
    assert L.rm_scene_camera_lens(sc._h, None, C.byref(x)) == abi.RM_ERR_INVALID_ARGUMENT


# ---------------------------------------------------------------- the lens cameras
def _camera_data(pos, look, up, angle_deg):
    cd = abi.RmCameraData()
    for i in range(3):
        cd.pos[i], cd.look[i], cd.up[i] = pos[i], look[i], up[i]
    cd.pos[3], cd.look[3], cd.up[3] = 1.0, 0.0, 0.0
    cd.heightAngle = math.radians(angle_deg)
    return cd


def _lens(cd, W, H, radius, focus, n, near=0.1, far=100.0):
    out = (abi.RmCamera * n)()
    st = lib().rm_camera_lens_samples(C.byref(cd), W, H, near, far, radius, focus, n, out)
    assert st == abi.RM_OK, lib().rm_last_error().decode()
    return out


LENSES = [((0.0, 0.0, 16.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 49.5, 0.008, 3.0),      # depth_of_field.json
          ((0.0, 0.0, 4.5), (0.0, 0.0, -4.5), (0.0, 1.0, 0.0), 30.0, 0.12, 3.6),          # unit_mandelbulb.json, look not normalised
          ((2.6, 2.2, 3.0), (-2.6, -2.2, -3.0), (0.1, 1.0, 0.0), 30.0, 0.3, 4.0),         # oblique, up not orthogonal to look
          ((-3.0, 7.0, 1.0), (0.5, -1.0, 0.25), (0.0, 0.0, 1.0), 60.0, 1.5, 9.0)]         # another up axis, a wide lens


@pytest.mark.parametrize("pos,look,up,angle,radius,focus", LENSES)
def test_lens_sample_0_is_the_pinhole_and_radius_0_is_n_pinholes(pos, look, up, angle, radius, focus):
    W, H = 97, 53
    cd = _camera_data(pos, look, up, angle)
    pin = abi.RmCamera()
    assert lib().rm_camera_build(C.byref(cd), W, H, 0.1, 100.0, None, None, C.byref(pin)) == 0
    for n in (1, 2, 5, 16):
        cams = _lens(cd, W, H, radius, focus, n)
        assert bytes(cams[0]) == bytes(pin), n
        assert all(bytes(c) == bytes(pin) for c in _lens(cd, W, H, 0.0, focus, n)), n
        if n > 1:
            assert all(bytes(c) != bytes(pin) for c in list(cams)[1:]), n


@pytest.mark.parametrize("pos,look,up,angle,radius,focus", LENSES)
def test_lens_samples_lie_on_the_disc_and_look_at_the_focus_point(pos, look, up, angle, radius, focus):
    """In float64 from what the kernel reads: the eye of sample k sits on the lens disc where the header puts it, and the ray
    through the centre of its image (clip (0, 0, ∓1, 1) through invProjView: near and far point, as the shader's primary ray)
    passes within 1e-4 world units of pos + focus · normalize(look)."""
    W, H, n = 97, 53, 16
    cd = _camera_data(pos, look, up, angle)
    p, l, upv = (np.array(v, dtype=np.float32).astype(np.float64) for v in (pos, look, up))
    l = l / np.linalg.norm(l)
    w = -l
    v = upv - np.dot(upv, w) * w
    v = v / np.linalg.norm(v)
    u = np.cross(v, w)
    F = p + float(np.float32(focus)) * l
    R = float(np.float32(radius))
    for k, cam in enumerate(_lens(cd, W, H, radius, focus, n)):
        eye = np.array(cam.eyePosition[:3], dtype=np.float64)
        r, th = R * math.sqrt(k / (n - 1)), k * math.pi * (3.0 - math.sqrt(5.0))
        want = p + r * (math.cos(th) * u + math.sin(th) * v)
        assert np.abs(eye - want).max() <= 1e-6 * max(1.0, np.abs(want).max()), (k, eye, want)  # rounded once to float
        M = np.array(cam.invProjView[:], dtype=np.float64).reshape(4, 4).T  # column-major storage
        near, far = M @ np.array([0.0, 0.0, -1.0, 1.0]), M @ np.array([0.0, 0.0, 1.0, 1.0])
        a, b = near[:3] / near[3], far[:3] / far[3]
        d = (b - a) / np.linalg.norm(b - a)
        miss = np.linalg.norm(np.cross(F - a, d))
        assert miss < 1e-4, (k, miss)
        assert np.dot(F - a, d) > 0.0  # in front of the camera
    assert abs(np.linalg.norm(np.array(_lens(cd, W, H, radius, focus, n)[n - 1].eyePosition[:3], dtype=np.float64) - p) - R) < 1e-5  # the last sample: the rim


def test_lens_argument_errors():
    L = lib()
    cd = _camera_data(*LENSES[0][:4])
    out = (abi.RmCamera * 4)()

    def st(radius=0.1, focus=3.0, n=4, cdp=C.byref(cd), outp=out, W=32, H=24):
        return L.rm_camera_lens_samples(cdp, W, H, 0.1, 100.0, radius, focus, n, outp)

    assert st() == abi.RM_OK
    for n in (0, -1, -100):
        assert refused(st(n=n)), n
    for radius in (-0.1, -1e-30, float("inf"), float("-inf"), float("nan")):
        assert refused(st(radius=radius)), radius
    for focus in (0.0, -0.0, -3.0, float("inf"), float("-inf"), float("nan")):
        assert refused(st(focus=focus)), focus
    assert refused(st(cdp=None)) and refused(st(outp=None))
    assert refused(st(W=0)) and refused(st(H=-1))  # what rm_camera_build refuses
    flat = _camera_data((0, 0, 5), (0, 1, 0), (0, 1, 0), 30.0)  # up parallel to look
    assert refused(st(cdp=C.byref(flat)))


# ---------------------------------------------------------------- the Python layer
def test_python_wrappers_check_before_any_device_is_touched():
    from raymarcher_amd.render import Renderer, SceneTables, lens_cameras, shutter_globals
    W, H = 32, 24
    scene = h.scene_mandelbulb(W, H)
    cams = [h.make_camera((0, 0, 4.5 + 0.1 * i), (0, 0, -1), (0, 1, 0), 30.0, W, H) for i in range(6)]
    r = Renderer.__new__(Renderer)  # no device is touched before the checks
    t = SceneTables(*scene)
    s = abi.default_settings()
    for sub in (0, -1, 65, 2.0, None, True):
        with pytest.raises(ValueError):
            r.render_accumulated(t, s, W, H, cams, sub)
    with pytest.raises(ValueError):
        r.render_accumulated(t, s, W, H, cams, 4)  # 6 cameras are not frames of 4
    with pytest.raises(ValueError):
        r.render_accumulated(t, s, W, H, cams, 3, globals_=[scene[5]] * 2)  # neither one nor one per camera
    for kw in (dict(supersample=2), dict(adaptive=0.1), dict(supersample=4, adaptive=0.1)):
        with pytest.raises(ValueError):
            r.render_sequence(t, s, W, H, cams, accumulate=3, **kw)
    with pytest.raises(ValueError):
        r.render_sequence(t, s, W, H, cams, accumulate=4)
    with pytest.raises(ValueError):
        lens_cameras(_camera_data(*LENSES[0][:4]), W, H, 0.1, 3.0, 0)
    with pytest.raises(ValueError):
        shutter_globals(scene[5], 0.0, 1.0, 0)
    # lens_cameras is the C helper
    cd = _camera_data(*LENSES[2][:4])
    assert [bytes(c) for c in lens_cameras(cd, W, H, 0.3, 4.0, 5)] == [bytes(c) for c in _lens(cd, W, H, 0.3, 4.0, 5)]


def test_shutter_globals_are_the_interval_midpoints():
    from raymarcher_amd.render import shutter_globals
    g = h.make_globals(power=7.5, julia=(0.25, -0.5), itime=99.0)
    for t0, t1, n in ((0.0, 1.0, 1), (0.0, 1.0, 4), (3.7, 3.7 + 1 / 24, 5), (10.0, 9.0, 3), (0.1, 0.7, 16)):
        gs = shutter_globals(g, t0, t1, n)
        assert len(gs) == n
        for j, gj in enumerate(gs):
            want = np.float32(np.float64(t0) + (j + 0.5) * (np.float64(t1) - np.float64(t0)) / n)
            assert np.float32(gj.iTime).view(np.uint32) == want.view(np.uint32), (t0, t1, n, j)
            assert (gj.power, gj.juliaSeed[0], gj.juliaSeed[1], gj.ka) == (g.power, g.juliaSeed[0], g.juliaSeed[1], g.ka)
    assert g.iTime == 99.0  # the caller's struct is not changed
