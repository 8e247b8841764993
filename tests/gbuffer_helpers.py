"""The specification of rm_render_gbuffer for the tests: tests/gbuffer_spec/rm_gbuffer_spec.c, which includes the oracle's source and
restates the head of its render() with the oracle's own static functions, built on demand and loaded with ctypes by
helpers.load_spec.  Nothing under oracle/ is touched.  Also the float64 primary rays of the analytic checks."""
import ctypes as C

import numpy as np

import helpers as h
from raymarcher_amd import abi

P = C.POINTER
SIGNATURES = {"rmo_spec_gbuffer": (C.c_int, [P(abi.RmCamera), P(abi.RmObject), C.c_int, P(abi.RmGlobals), P(abi.RmSettings), C.c_int,
                                             C.c_int, P(C.c_float), P(C.c_int32), P(C.c_float)])}


def spec():
    """ctypes handle of the spec library (helpers.load_spec: rebuilt when a source it is made of is newer)."""
    return h.load_spec("gbuffer", SIGNATURES)


def spec_gbuffer(cam, objs, num_objects, g, s, W, H, position=True):
    """The G-buffer of one frame by the specification → (normal_depth (H, W, 4) float32, object_id (H, W) int32, position (H, W, 4)
    float32 or None), row 0 at the bottom."""
    nd = np.empty((H, W, 4), dtype=np.float32)
    ids = np.empty((H, W), dtype=np.int32)
    pos = np.empty((H, W, 4), dtype=np.float32) if position else None
    st = spec().rmo_spec_gbuffer(C.byref(cam), objs, num_objects, C.byref(g), C.byref(s), W, H, h.fptr(nd),
                                 ids.ctypes.data_as(C.POINTER(C.c_int32)), h.fptr(pos) if position else None)
    assert st == 0, f"spec status {st}"
    return nd, ids, pos


def primary_rays(cam, W, H):
    """(ro, rd) of every pixel centre in float64 from the camera's inverse projection-view matrix, (H, W, 3) each, row 0 at the
    bottom — an independent statement of frag:2388-2392 for the analytic checks (evaluated per pixel, not from the corners)."""
    M = np.array(cam.invProjView[:], dtype=np.float64).reshape(4, 4).T  # column-major storage
    x = (np.arange(W) + 0.5) / W * 2.0 - 1.0
    y = (np.arange(H) + 0.5) / H * 2.0 - 1.0
    X, Y = np.meshgrid(x, y)

    def unproject(z):
        p = np.stack([X, Y, np.full_like(X, z), np.ones_like(X)], axis=-1) @ M.T
        return p[..., :3] / p[..., 3:4]
    ro, far = unproject(-1.0), unproject(1.0)
    rd = far - ro
    return ro, rd / np.linalg.norm(rd, axis=-1, keepdims=True)
