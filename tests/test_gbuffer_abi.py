"""rm_render_gbuffer without a GPU: the header declares it and the library exports it under the unchanged ABI version, every
argument error returns its status before the first HIP call, and the specification the GPU tests compare against
(tests/gbuffer_spec/rm_gbuffer_spec.c, the oracle's own functions) is sane: it hits exactly the pixels the oracle's render hits,
its misses and normals are what the definition says, and on a sphere it agrees with the analytic intersection."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

import abi_helpers as ah
import gbuffer_helpers as G
import helpers as h
import scene_builders as SB
from abi_helpers import FAKE, HEADER, HP, INT_MAX, refused
from raymarcher_amd import abi, lib
from raymarcher_amd._lib import SIGNATURES

SURFACE_DIST = 1e-3  # frag:32


# ---------------------------------------------------------------- symbol and signature
def test_header_declares_and_library_exports_the_symbol():
    assert ah.params("rm_render_gbuffer") == [
        "const RmCamera *cams", "const RmGlobals *globals", "int numGlobals", "int numFrames", "const RmObject *objs",
        "int numObjects", "const RmSettings *s", "int W", "int H", "float *d_normalDepth", "int32_t *d_objectId", "float *d_position",
        "void *stream"]
    res, args = SIGNATURES["rm_render_gbuffer"]
    P = C.POINTER
    assert res is C.c_int and args == [P(abi.RmCamera), P(abi.RmGlobals), C.c_int, C.c_int, P(abi.RmObject), C.c_int, P(abi.RmSettings),
                                       C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    ah.assert_exported(["rm_render_gbuffer"])


def test_abi_version_stays():
    ah.assert_abi_version()


def test_header_comment_carries_the_definition():
    ah.assert_comment_has("rm_render_gbuffer", (
        "frag:2388-2392", "2443", "2318-2337", "1453-1484", "1436-1444", "1679-1691", "raymarch(ro, rd, far, OUTSIDE)",
        "reports its own index", "not a view-space z", "bumpNormal(n, p, 10, 2)", "depth = far", "frag:2328",
        "(n.x, n.y, n.z, depth)", "hit ? 1 : 0", "names the frame", "before any HIP call", "rm_debug_last_path() = 11",
        "symbol lookup"))
    assert re.search(r"11 = a launch\s+\*?\s*of rm_render_gbuffer", HEADER), "rm_debug_last_path's comment does not document 11"


def test_python_signature():
    from raymarcher_amd.render import Renderer
    sig = inspect.signature(Renderer.render_gbuffer)
    assert list(sig.parameters) == ["self", "tables", "settings", "W", "H", "cameras", "globals_", "position", "out_normal_depth",
                                    "out_object_id", "out_position"]
    assert sig.parameters["cameras"].default is None and sig.parameters["position"].default is False


# ---------------------------------------------------------------- refusals, all without a device
def _scene(n, W=32, H=24):
    objs, no, _ = SB.three_primitives()
    cams = (abi.RmCamera * n)(*[h.make_camera((0, 0, 5), (0, 0, -1), (0, 1, 0), 40.0, W, H) for _ in range(n)])
    globs = (abi.RmGlobals * n)(*[h.make_globals(itime=0.1 * i) for i in range(n)])
    return cams, globs, objs, no


def call(cams, globs, ng, n, objs, no, s="default", W=32, H=24, nd=FAKE, ids=FAKE, pos=None):
    s = abi.default_settings() if s == "default" else s
    return lib().rm_render_gbuffer(cams, globs, ng, n, objs, no, C.byref(s) if s is not None else None, W, H, nd, ids, pos, None)


def test_frame_counts_globals_and_sizes():
    cams, globs, objs, no = _scene(3)
    assert refused(call(cams, globs, 1, -1, objs, no), text="numFrames")
    for n in (abi.RM_MAX_BATCH_FRAMES + 1, INT_MAX):
        assert refused(call(cams, globs, 1, n, objs, no), "RM_MAX_BATCH_FRAMES", want=abi.RM_ERR_CAPACITY)
    # numFrames == 0: RM_OK with null outputs, nothing is read
    assert call(cams, globs, 1, 0, objs, no, nd=None, ids=None) == abi.RM_OK
    assert call(None, None, 0, 0, None, 0, s=None, nd=None, ids=None) == abi.RM_OK
    for ng in (0, 2, 4, -1):
        assert refused(call(cams, globs, ng, 3, objs, no), text="numGlobals"), ng
    assert refused(call(None, globs, 1, 3, objs, no), text="null cameras or globals")
    assert refused(call(cams, None, 1, 3, objs, no), text="null cameras or globals")
    for W, H in ((0, 24), (32, 0), (-5, 24), (32, -1), (INT_MAX // 8 + 1, 8), (8, 65536 * 8)):
        assert refused(call(cams, globs, 3, 3, objs, no, W=W, H=H)), (W, H)


def test_the_three_unsupported_cases():
    L = lib()
    cams, globs, objs, no = _scene(3)
    for feat in (abi.RM_FEAT_TERRAIN, abi.RM_FEAT_CLOUD, abi.RM_FEAT_SEA, abi.RM_FEAT_TERRAIN | abi.RM_FEAT_PERLIN_BUMP):
        assert refused(call(cams, globs, 3, 3, objs, no, s=abi.default_settings(features=feat)), want=abi.RM_ERR_UNSUPPORTED), feat
    # the other feature bits are fine: they get as far as the output pointers
    for feat in (0, abi.RM_FEAT_SKY_BACKGROUND, abi.RM_FEAT_NIGHTSKY_BACKGROUND, abi.RM_FEAT_REFERENCE_DEFAULT):
        assert refused(call(cams, globs, 3, 3, objs, no, s=abi.default_settings(features=feat), nd=None), text="null output"), feat
    # isTwoD in frame 2 of 3: the error names the frame
    globs[2].isTwoD = 1
    assert refused(call(cams, globs, 3, 3, objs, no), "frame 2", want=abi.RM_ERR_UNSUPPORTED)
    assert refused(call(cams, globs, 1, 3, objs, no, nd=None), text="null output")  # with one shared globals frame 2's is never read
    globs[2].isTwoD = 0
    globs[0].isTwoD = 1
    assert refused(call(cams, globs, 1, 3, objs, no), "frame 0", want=abi.RM_ERR_UNSUPPORTED)
    globs[0].isTwoD = 0
    objs[1].type = abi.RM_CUSTOM
    assert refused(call(cams, globs, 3, 3, objs, no), "object 1", want=abi.RM_ERR_UNSUPPORTED)
    assert "CUSTOM" in L.rm_last_error().decode()


def test_object_validation_and_outputs():
    cams, globs, objs, no = _scene(3)
    assert refused(call(cams, globs, 3, 3, None, no))
    assert refused(call(cams, globs, 3, 3, objs, -1))
    assert refused(call(cams, globs, 3, 3, objs, no, s=None))
    many = (abi.RmObject * (abi.RM_MAX_OBJECTS + 1))(*[h.make_object(abi.RM_SPHERE) for _ in range(abi.RM_MAX_OBJECTS + 1)])
    assert refused(call(cams, globs, 3, 3, many, abi.RM_MAX_OBJECTS + 1), want=abi.RM_ERR_CAPACITY)
    assert refused(call(cams, globs, 3, 3, objs, no, s=abi.default_settings(maxSteps=-1)), text="loop bound")
    objs[2].type = 99
    assert refused(call(cams, globs, 3, 3, objs, no), "object 2", want=abi.RM_ERR_UNSUPPORTED)
    objs[2].type = abi.RM_TORUS
    # a texLoc, a sky box or an emissive rectangle without its sampler is not an error here: the call gets to its outputs
    objs[0].texLoc = 3
    objs[1].isEmissive = 1
    s = abi.default_settings(enableSkyBox=1, features=abi.RM_FEAT_NIGHTSKY_BACKGROUND)
    assert refused(call(cams, globs, 3, 3, objs, no, s=s, nd=None), text="null output")
    assert refused(call(cams, globs, 3, 3, objs, no, s=s, ids=None), text="null output")
    assert refused(call(cams, globs, 3, 3, None, 0, nd=None), text="null output")  # an empty table needs no pointer
    # host memory is not device memory: each output is checked, the optional one too
    assert refused(call(cams, globs, 3, 3, objs, no, nd=HP, ids=HP), text="d_normalDepth")


# ---------------------------------------------------------------- the specification, on the CPU
@pytest.mark.parametrize("name", ["directional_light_2", "mandelbulb"])
def test_spec_hits_what_the_oracle_hits(name):
    W, H = 64, 36
    scene = SB.directional_light_2(W, H) if name == "directional_light_2" else h.scene_mandelbulb(W, H)
    s = abi.default_settings()
    _, cnt = h.oracle_render(scene, s, W, H, counters=True)
    nd, ids, pos = G.spec_gbuffer(scene[0], scene[1], scene[2], scene[5], s, W, H)
    hit = ids >= 0
    assert int(hit.sum()) == int(cnt.hitPixels) and 0 < hit.sum() < W * H
    assert np.isfinite(nd).all() and np.isfinite(pos).all()
    assert (ids[~hit] == -1).all() and (ids < scene[2]).all()
    # every miss: depth initialFar, a zero normal, a zero position
    far = np.float32(scene[0].initialFar)
    assert (nd[~hit][:, 3].view(np.uint32) == far.view(np.uint32)).all()
    assert (nd[~hit][:, :3] == 0).all() and (pos[~hit] == 0).all()
    # every hit: a unit normal, position flag 1, depth in front of far
    assert np.abs(np.linalg.norm(nd[hit][:, :3].astype(np.float64), axis=-1) - 1.0).max() <= 1e-5
    assert (pos[hit][:, 3] == 1).all() and (nd[hit][:, 3] < far).all() and (nd[hit][:, 3] > 0).all()
    # without position the two required outputs are the same bits
    nd2, ids2, none = G.spec_gbuffer(scene[0], scene[1], scene[2], scene[5], s, W, H, position=False)
    assert none is None and (nd2.view(np.uint32) == nd.view(np.uint32)).all() and (ids2 == ids).all()


def test_spec_on_a_lone_unit_sphere_against_the_analytic_intersection():
    """Radius 1 at the origin, no bump.  Where the analytic n·(−rd) >= 0.5: the march stops within SURFACE_DIST of the surface, which
    is at most 2·SURFACE_DIST along such a ray, plus the subtracted minD (< SURFACE_DIST) → depth within 3·SURFACE_DIST; the normal
    within 1e-2 of p/|p| — a gate against a swapped tap or sign, which errs by O(1), not an accuracy claim."""
    W, H = 64, 36
    cam = h.make_camera((0.3, 0.4, 4.0), (-0.3, -0.4, -4.0), (0, 1, 0), 35.0, W, H)
    objs = (abi.RmObject * 1)(h.make_object(abi.RM_SPHERE, model=h.scale(2, 2, 2), scale_factor=2.0))
    g = h.make_globals()
    s = abi.default_settings(features=abi.RM_FEAT_WHITE_BACKGROUND)
    nd, ids, pos = G.spec_gbuffer(cam, objs, 1, g, s, W, H)
    ro, rd = G.primary_rays(cam, W, H)
    b = (ro * rd).sum(-1)
    disc = b * b - ((ro * ro).sum(-1) - 1.0)
    t = -b - np.sqrt(np.maximum(disc, 0.0))
    p = ro + rd * t[..., None]
    facing = (disc > 0) & (-(p * rd).sum(-1) >= 0.5)  # |p| = 1: the analytic normal is p
    assert facing.sum() > 50
    assert (ids[facing] == 0).all()
    assert np.abs(nd[facing][:, 3].astype(np.float64) - t[facing]).max() <= 3 * SURFACE_DIST
    assert np.abs(nd[facing][:, :3].astype(np.float64) - p[facing]).max() <= 1e-2
    assert np.abs(pos[facing][:, :3].astype(np.float64) - p[facing]).max() <= 3 * SURFACE_DIST
    assert (ids[disc < -1e-3] == -1).all()
