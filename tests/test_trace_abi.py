"""rm_trace_rays and rm_camera_rays without a GPU: the header declares them and the library exports them under the unchanged ABI
version, the two structs are 32 bytes, every argument error returns its status before the first HIP call — with pointers that would
fault if read — and rm_camera_rays, a host function, equals the specification's primary rays in every bit
(tests/trace_spec/rm_trace_spec.c: the oracle's own rayPlanes, interpolateVarying and normalize3)."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

import abi_helpers as ah
import helpers as h
import scene_builders as SB
import trace_helpers as T
from abi_helpers import FAKE, HEADER, HP, INT_MAX, fake, refused
from raymarcher_amd import abi, camera_rays, lib
from raymarcher_amd._lib import SIGNATURES
from scene_builders import three_primitives as _scene


# ---------------------------------------------------------------- symbols, structs, the written definition
def test_header_declares_and_library_exports_both_symbols():
    assert ah.params("rm_trace_rays") == [
        "const RmRay *d_rays", "int numRays", "const RmObject *objs", "int numObjects",
        "const RmGlobals *g", "const RmSettings *s", "unsigned mode", "RmRayHit *d_hits", "void *stream"]
    assert ah.params("rm_camera_rays") == ["const RmCamera *cam", "int W", "int H", "const int32_t *xy", "int n", "RmRay *out"]
    P = C.POINTER
    assert SIGNATURES["rm_trace_rays"] == (C.c_int, [C.c_void_p, C.c_int, P(abi.RmObject), C.c_int, P(abi.RmGlobals), P(abi.RmSettings),
                                                     C.c_uint, C.c_void_p, C.c_void_p])
    assert SIGNATURES["rm_camera_rays"] == (C.c_int, [P(abi.RmCamera), C.c_int, C.c_int, P(C.c_int32), C.c_int, C.c_void_p])
    ah.assert_exported(["rm_trace_rays", "rm_camera_rays"])


def test_abi_version_stays_and_the_structs_are_32_bytes():
    ah.assert_abi_version()
    assert lib().rm_abi_sizeof(11) == C.sizeof(abi.RmRay) == 32
    assert lib().rm_abi_sizeof(12) == C.sizeof(abi.RmRayHit) == 32
    assert lib().rm_abi_sizeof(99) == -1 and lib().rm_abi_sizeof(13) == -1
    assert [f[0] for f in abi.RmRay._fields_] == ["origin", "tMax", "dir", "reserved"]
    assert [f[0] for f in abi.RmRayHit._fields_] == ["normal", "t", "position", "objectId"]
    assert abi.RmRay.tMax.offset == 12 and abi.RmRay.dir.offset == 16 and abi.RmRayHit.t.offset == 12 and abi.RmRayHit.objectId.offset == 28
    for name, val in (("RM_TRACE_CLOSEST", "0u"), ("RM_TRACE_NO_NORMAL", "1u"), ("RM_TRACE_OCCLUSION", "2u"), ("RM_RAY_INVALID", r"\(-2\)")):
        assert re.search(rf"#define\s+{name}\s+{val}", HEADER), name
    assert (abi.RM_TRACE_CLOSEST, abi.RM_TRACE_NO_NORMAL, abi.RM_TRACE_OCCLUSION, abi.RM_RAY_INVALID) == (0, 1, 2, -2)


def test_header_comment_carries_the_definition():
    ah.assert_comment_has("RmRay", (
        "NOT normalised", "units of |dir|", "raymarch(origin, dir, tMax, OUTSIDE)", "frag:1453-1484", "frag:2318-2337",
        "frag:1436-1444", "frag:1679-1691", "frag:1703-1725", "softshadow(origin, dir, 0, tMax, 8)",
        "t = tMax as given", "not the march's ray depth", "penumbra factor", "objectId == −1 ? t : 0", "RM_RAY_INVALID, t = 0",
        "evaluates nothing", "cannot refuse them", "does not depend on which other rays", "before any HIP call",
        "rm_debug_last_path() = 12", "symbol lookup"))
    assert re.search(r"12 = a launch of rm_trace_rays", HEADER), "rm_debug_last_path's comment does not document 12"
    assert re.search(r"11 RmRay, 12 RmRayHit", HEADER), "rm_abi_sizeof's comment does not list the two structs"


def test_python_signatures():
    from raymarcher_amd.render import Renderer
    sig = inspect.signature(Renderer.trace_rays)
    assert list(sig.parameters) == ["self", "tables", "settings", "rays", "mode", "normals", "out"]
    assert sig.parameters["mode"].default == "closest" and sig.parameters["normals"].default is True
    assert list(inspect.signature(Renderer.pick).parameters) == ["self", "tables", "settings", "W", "H", "x", "y", "camera"]
    assert list(inspect.signature(camera_rays).parameters) == ["camera", "W", "H", "pixels"]


# ---------------------------------------------------------------- refusals, all without a device


def call(objs, no, g, s="default", n=100, mode=0, rays=FAKE, hits=FAKE):
    s = abi.default_settings() if s == "default" else s
    return lib().rm_trace_rays(rays, n, objs, no, C.byref(g) if g is not None else None, C.byref(s) if s is not None else None, mode,
                               hits, None)


def test_counts_and_scene_pointers():
    objs, no, g = _scene()
    assert refused(call(objs, no, g, n=-1), text="numRays")
    assert refused(call(objs, no, g, n=-INT_MAX), text="numRays")
    # numRays == 0: RM_OK with null everything, nothing is read
    assert call(objs, no, g, n=0, rays=None, hits=None) == abi.RM_OK
    assert call(None, 0, None, s=None, n=0, rays=None, hits=None) == abi.RM_OK
    assert call(None, 5, None, s=None, n=0, mode=77, rays=None, hits=None) == abi.RM_OK
    # every positive int fits one grid: INT_MAX rays get as far as the scene pointers
    assert refused(call(objs, no, None, n=INT_MAX), text="null scene pointer")
    assert refused(call(objs, no, g, s=None), text="null scene pointer")
    assert refused(call(None, no, g), text="null scene pointer")
    assert refused(call(objs, -1, g), text="null scene pointer")


def test_mode_bits():
    objs, no, g = _scene()
    for mode in (4, 8, 0x80000000, 0xFFFFFFFF, 5, 6):
        assert refused(call(objs, no, g, mode=mode), text="unknown mode bits"), mode
    assert refused(call(objs, no, g, mode=abi.RM_TRACE_NO_NORMAL | abi.RM_TRACE_OCCLUSION), text="RM_TRACE_NO_NORMAL")
    # the three modes that exist get as far as the arrays
    for mode in (abi.RM_TRACE_CLOSEST, abi.RM_TRACE_NO_NORMAL, abi.RM_TRACE_OCCLUSION):
        assert refused(call(objs, no, g, mode=mode, rays=None), text="null d_rays or d_hits"), mode
    # the mode is checked after the scene pointers and before the scene's content
    assert refused(call(objs, no, None, mode=4), text="null scene pointer")
    assert refused(call(objs, no, g, s=abi.default_settings(features=abi.RM_FEAT_SEA), mode=4), text="unknown mode bits")


def test_capacity_unsupported_and_loop_bounds():
    objs, no, g = _scene()
    many = (abi.RmObject * (abi.RM_MAX_OBJECTS + 1))(*[h.make_object(abi.RM_SPHERE) for _ in range(abi.RM_MAX_OBJECTS + 1)])
    assert refused(call(many, abi.RM_MAX_OBJECTS + 1, g), "RM_MAX_OBJECTS", want=abi.RM_ERR_CAPACITY)
    assert refused(call(many, abi.RM_MAX_OBJECTS, g, rays=None), text="null d_rays or d_hits")
    for feat in (abi.RM_FEAT_TERRAIN, abi.RM_FEAT_CLOUD, abi.RM_FEAT_SEA, abi.RM_FEAT_TERRAIN | abi.RM_FEAT_PERLIN_BUMP):
        assert refused(call(objs, no, g, s=abi.default_settings(features=feat)), "TERRAIN / CLOUD / SEA", want=abi.RM_ERR_UNSUPPORTED), feat
    for feat in (0, abi.RM_FEAT_SKY_BACKGROUND, abi.RM_FEAT_NIGHTSKY_BACKGROUND, abi.RM_FEAT_REFERENCE_DEFAULT):
        assert refused(call(objs, no, g, s=abi.default_settings(features=feat), hits=None), text="null d_rays or d_hits"), feat
    assert refused(call(objs, no, h.make_globals(two_d=1)), "isTwoD", want=abi.RM_ERR_UNSUPPORTED)
    for field in ("maxSteps", "fractalIters", "mengerLevels"):
        assert refused(call(objs, no, g, s=abi.default_settings(**{field: -1})), text="loop bound"), field
    assert refused(call(objs, no, g, s=abi.default_settings(maxSteps=0), rays=None), text="null d_rays or d_hits")
    objs[1].type = abi.RM_CUSTOM
    assert refused(call(objs, no, g), "object 1", want=abi.RM_ERR_UNSUPPORTED)
    assert "CUSTOM" in lib().rm_last_error().decode()
    for ty in (99, -1):
        objs[1].type = abi.RM_CUBE
        objs[2].type = ty
        assert refused(call(objs, no, g), "object 2", want=abi.RM_ERR_UNSUPPORTED), ty


def test_the_two_arrays():
    objs, no, g = _scene()
    assert refused(call(objs, no, g, rays=None), text="null d_rays or d_hits")
    assert refused(call(objs, no, g, hits=None), text="null d_rays or d_hits")
    assert refused(call(None, 0, g, hits=None), text="null d_rays or d_hits")  # an empty table needs no pointer
    for off in (4, 8, 12, 1):
        assert refused(call(objs, no, g, rays=fake(0x1000 + off)), text="16-byte aligned"), off
        assert refused(call(objs, no, g, hits=fake(0x1000 + off)), text="16-byte aligned"), off
    # host memory is not device memory: each array is checked (the only check that asks the HIP runtime)
    assert refused(call(objs, no, g, rays=HP, hits=HP), text="d_rays")


# ---------------------------------------------------------------- rm_camera_rays against the specification
def _cameras(W, H):
    return {"directional_light_2": SB.directional_light_2(W, H)[0], "mandelbulb": h.scene_mandelbulb(W, H)[0]}


@pytest.mark.parametrize("W,H", [(64, 36), (37, 23)])
@pytest.mark.parametrize("name", ["directional_light_2", "mandelbulb"])
def test_camera_rays_equal_the_specs_primary_rays_in_every_bit(name, W, H):
    cam = _cameras(W, H)[name]
    rays = camera_rays(cam, W, H)
    assert rays.shape == (W * H, 8) and rays.dtype == np.float32
    T.assert_bits(rays, T.spec_primary_rays(cam, W, H), f"{name} {W}x{H} whole frame")
    assert (rays[:, 3] == np.float32(cam.initialFar)).all() and (T.bits(rays[:, 7]) == 0).all()
    assert np.abs(np.linalg.norm(rays[:, 4:7].astype(np.float64), axis=1) - 1.0).max() <= 1e-6
    # an explicit list, in an order of its own, with repeats and the four corners
    rng = np.random.default_rng(W * 1000 + H)
    px = np.stack([rng.integers(0, W, 300), rng.integers(0, H, 300)], axis=1)
    px = np.concatenate([px, [[0, 0], [W - 1, 0], [0, H - 1], [W - 1, H - 1], [0, 0]]]).astype(np.int32)
    listed = camera_rays(cam, W, H, px)
    T.assert_bits(listed, T.spec_primary_rays(cam, W, H, px), f"{name} {W}x{H} pixel list")
    T.assert_bits(listed, rays[px[:, 1] * W + px[:, 0]], f"{name} {W}x{H} list against the whole frame")


def test_camera_rays_refusals():
    W, H = 37, 23
    cam = _cameras(W, H)["mandelbulb"]
    out = (abi.RmRay * (W * H))()
    L = lib()

    def xy(*pairs):
        a = np.array(pairs, dtype=np.int32).reshape(-1)
        return a.ctypes.data_as(C.POINTER(C.c_int32)), a

    for x, y in ((-1, 0), (0, -1), (W, 0), (0, H), (W - 1, H), (INT_MAX, 0), (-INT_MAX - 1, 3)):
        p, keep = xy((3, 4), (x, y))
        out[0].tMax = -7.0
        assert refused(L.rm_camera_rays(C.byref(cam), W, H, p, 2, out), text="outside the frame"), (x, y)
        assert out[0].tMax == -7.0, "a refused call wrote a ray"
    p, keep = xy((3, 4))
    assert refused(L.rm_camera_rays(None, W, H, p, 1, out))
    assert refused(L.rm_camera_rays(C.byref(cam), W, H, p, 1, None))
    assert refused(L.rm_camera_rays(C.byref(cam), 0, H, p, 1, out))
    assert refused(L.rm_camera_rays(C.byref(cam), W, -1, p, 1, out))
    assert refused(L.rm_camera_rays(C.byref(cam), W, H, p, -1, out))
    assert refused(L.rm_camera_rays(C.byref(cam), W, H, None, W * H - 1, out), text="W·H")
    assert L.rm_camera_rays(C.byref(cam), W, H, p, 0, out) == abi.RM_OK
    assert L.rm_camera_rays(C.byref(cam), W, H, None, W * H, out) == abi.RM_OK
    with pytest.raises(Exception):
        camera_rays(cam, W, H, [(W, 0)])
