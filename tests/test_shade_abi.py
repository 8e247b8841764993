"""rm_shade_rays without a GPU: the header declares it and the library exports it under the unchanged ABI version, the comment
carries the definition, and every argument error returns its status, in the documented order, before the first HIP call — with
pointers that would fault if read."""
import ctypes as C
import inspect
import re

import abi_helpers as ah
import helpers as h
import scene_builders as SB
from abi_helpers import CAPACITY, FAKE, HEADER, HP, INT_MAX, fake, refused
from raymarcher_amd import abi, lib
from raymarcher_amd._lib import SIGNATURES
from scene_builders import three_primitives_lit as _scene

UNSUPPORTED = abi.RM_ERR_UNSUPPORTED


# ---------------------------------------------------------------- the symbol and the written definition
def test_header_declares_and_library_exports_the_symbol():
    assert ah.params("rm_shade_rays") == [
        "const RmRay *d_rays", "int numRays", "float far", "const RmObject *objs", "int numObjects", "const RmLight *lights",
        "int numLights", "const RmGlobals *g", "const RmSettings *s", "const RmResources *res", "float *d_rgba", "float *d_bright",
        "void *stream"]
    Ptr = C.POINTER
    assert SIGNATURES["rm_shade_rays"] == (C.c_int, [C.c_void_p, C.c_int, C.c_float, Ptr(abi.RmObject), C.c_int, Ptr(abi.RmLight), C.c_int,
                                                     Ptr(abi.RmGlobals), Ptr(abi.RmSettings), Ptr(abi.RmResources), C.c_void_p,
                                                     C.c_void_p, C.c_void_p])
    ah.assert_exported(["rm_shade_rays"])
    assert abi.RM_PATH_SHADE_RAYS == 13 and abi.RM_PATH_TRACE_RAYS == 12
    ah.assert_abi_version()


def test_header_comment_carries_the_definition():
    ah.assert_comment_has("rm_shade_rays", (
        "NOT normalised", "assumes a unit rd", "frag:2405-2419", "frag:2443", "frag:2491-2524", "frag:2526-2570", "frag:2572",
        "frag:1938-1946", "render(ro, rd, OUTSIDE, far, bg)", "ONE value per call", "RmRay.tMax is NOT read",
        "(0, 0, 0, 0) in both outputs", "alpha 0 marks it", "evaluates nothing", "cannot refuse them",
        "does not depend on which other rays", "before any HIP call", "rm_debug_last_path() = 13", "symbol lookup"))
    assert re.search(r"13 = a launch of rm_shade_rays", HEADER), "rm_debug_last_path's comment does not document 13"


def test_python_signatures():
    from raymarcher_amd import panorama_rays, tile_order
    from raymarcher_amd.render import Renderer
    sig = inspect.signature(Renderer.shade_rays)
    assert list(sig.parameters) == ["self", "tables", "settings", "rays", "far", "bright", "out", "out_bright"]
    assert sig.parameters["far"].default is None and sig.parameters["bright"].default is False
    assert list(inspect.signature(Renderer.render_panorama).parameters) == ["self", "tables", "settings", "W", "H", "position", "forward",
                                                                            "up", "far"]
    sig = inspect.signature(panorama_rays)
    assert list(sig.parameters) == ["position", "W", "H", "forward", "up"]
    assert tuple(sig.parameters["forward"].default) == (0, 0, -1) and tuple(sig.parameters["up"].default) == (0, 1, 0)
    assert list(inspect.signature(tile_order).parameters) == ["W", "H", "tile"] and inspect.signature(tile_order).parameters["tile"].default == 8


# ---------------------------------------------------------------- refusals, all without a device
DEFAULT = object()


def call(objs, no, lights, nl, g, s=DEFAULT, n=100, far=100.0, res=None, rays=FAKE, rgba=FAKE, bright=None):
    s = abi.default_settings() if s is DEFAULT else s
    return lib().rm_shade_rays(rays, n, far, objs, no, lights, nl, C.byref(g) if g is not None else None,
                               C.byref(s) if s is not None else None, C.byref(res) if res is not None else None, rgba, bright, None)


ARRAYS = "null d_rays or d_rgba"  # the first check behind the scene's: a call that gets this far passed everything before it


def test_counts_and_scene_pointers():
    objs, no, lights, nl, g = _scene()
    assert refused(call(objs, no, lights, nl, g, n=-1), text="numRays")
    assert refused(call(objs, no, lights, nl, g, n=-INT_MAX), text="numRays")
    # numRays == 0: RM_OK with null everything, nothing is read
    assert call(objs, no, lights, nl, g, n=0, rays=None, rgba=None) == abi.RM_OK
    assert call(None, 5, None, -3, None, s=None, n=0, far=float("nan"), rays=None, rgba=None) == abi.RM_OK
    # every positive int fits one grid: INT_MAX rays get as far as the scene pointers
    assert refused(call(objs, no, lights, nl, None, n=INT_MAX), text="null scene pointer")
    assert refused(call(objs, no, lights, nl, g, s=None), text="null scene pointer")
    assert refused(call(None, no, lights, nl, g), text="null scene pointer")
    assert refused(call(objs, no, None, nl, g), text="null scene pointer")
    assert refused(call(objs, -1, lights, nl, g), text="null scene pointer")
    assert refused(call(objs, no, lights, -1, g), text="null scene pointer")
    # empty tables need no pointers
    assert refused(call(None, 0, None, 0, g, rays=None), text=ARRAYS)


def test_far():
    objs, no, lights, nl, g = _scene()
    for far in (float("nan"), -1.0, -1e-30, float("inf"), float("-inf")):
        assert refused(call(objs, no, lights, nl, g, far=far), text="far"), far
    for far in (0.0, -0.0, 1e-30, 3.0e38):
        assert refused(call(objs, no, lights, nl, g, far=far, rays=None), text=ARRAYS), far
    # far is checked behind the scene pointers and ahead of the scene's content
    assert refused(call(objs, no, lights, nl, None, far=-1.0), text="null scene pointer")
    assert refused(call(objs, no, lights, nl, g, s=abi.default_settings(features=abi.RM_FEAT_SEA), far=-1.0), text="far")


def test_layers_capacity_loop_bounds_and_types_in_order():
    objs, no, lights, nl, g = _scene()
    for feat in (abi.RM_FEAT_TERRAIN, abi.RM_FEAT_CLOUD, abi.RM_FEAT_SEA, abi.RM_FEAT_TERRAIN | abi.RM_FEAT_PERLIN_BUMP):
        assert refused(call(objs, no, lights, nl, g, s=abi.default_settings(features=feat)), "TERRAIN / CLOUD / SEA", want=UNSUPPORTED), feat
    for feat in (0, abi.RM_FEAT_SKY_BACKGROUND, abi.RM_FEAT_DARK_BACKGROUND, abi.RM_FEAT_REFERENCE_DEFAULT):
        assert refused(call(objs, no, lights, nl, g, s=abi.default_settings(features=feat), rgba=None), text=ARRAYS), feat
    assert refused(call(objs, no, lights, nl, h.make_globals(two_d=1)), "isTwoD", want=UNSUPPORTED)
    many = (abi.RmObject * (abi.RM_MAX_OBJECTS + 1))(*[h.make_object(abi.RM_SPHERE) for _ in range(abi.RM_MAX_OBJECTS + 1)])
    assert refused(call(many, abi.RM_MAX_OBJECTS + 1, lights, nl, g), "RM_MAX_OBJECTS", want=CAPACITY)
    assert refused(call(many, abi.RM_MAX_OBJECTS, lights, nl, g, rays=None), text=ARRAYS)
    lots = (abi.RmLight * (abi.RM_MAX_LIGHTS + 1))(*[h.make_light(abi.RM_LIGHT_POINT) for _ in range(abi.RM_MAX_LIGHTS + 1)])
    assert refused(call(objs, no, lots, abi.RM_MAX_LIGHTS + 1, g), "RM_MAX_LIGHTS", want=CAPACITY)
    assert refused(call(objs, no, lots, abi.RM_MAX_LIGHTS, g, rays=None), text=ARRAYS)
    for field in ("maxSteps", "fractalIters", "mengerLevels", "numReflection"):
        assert refused(call(objs, no, lights, nl, g, s=abi.default_settings(**{field: -1})), text="loop bound"), field
    assert refused(call(objs, no, lights, nl, g, s=abi.default_settings(maxSteps=0, numReflection=0), rays=None), text=ARRAYS)
    # the layers come before the capacity, the capacity before the loop bounds, the loop bounds before the types
    assert refused(call(many, abi.RM_MAX_OBJECTS + 1, lights, nl, g, s=abi.default_settings(features=abi.RM_FEAT_CLOUD)), "TERRAIN", want=UNSUPPORTED)
    assert refused(call(many, abi.RM_MAX_OBJECTS + 1, lights, nl, g, s=abi.default_settings(maxSteps=-1)), want=CAPACITY)
    objs[1].type = abi.RM_CUSTOM
    assert refused(call(objs, no, lights, nl, g, s=abi.default_settings(maxSteps=-1)), text="loop bound")
    assert refused(call(objs, no, lights, nl, g), "object 1", want=UNSUPPORTED)
    assert "CUSTOM" in lib().rm_last_error().decode()
    for ty in (99, -1):
        objs[1].type = abi.RM_CUBE
        objs[2].type = ty
        assert refused(call(objs, no, lights, nl, g), "object 2", want=UNSUPPORTED), ty
    objs[2].type = abi.RM_TORUS
    lights[1].type = 7
    assert refused(call(objs, no, lights, nl, g), "light 1", want=UNSUPPORTED)


def test_samplers_are_asked_for_as_by_rm_render_res():
    """Every sampler a feature, an object or a light reads must be supplied: rm_render_res's statuses and texts.  The pixel pointers
    of the resources that ARE supplied here are fake and never read: the calls stop at the arrays."""
    objs, no, lights, nl, g = _scene()
    tex = abi.RmTexture(0x2000, 4, 4)
    night = abi.default_settings(features=abi.RM_FEAT_NIGHTSKY_BACKGROUND)
    assert refused(call(objs, no, lights, nl, g, s=night), "noise", want=UNSUPPORTED)
    assert refused(call(objs, no, lights, nl, g, s=night, res=abi.RmResources()), "noise", want=UNSUPPORTED)
    res = abi.RmResources()
    res.noise = tex
    assert refused(call(objs, no, lights, nl, g, s=night, res=res, rays=None), text=ARRAYS)
    box = abi.default_settings(enableSkyBox=1)
    assert refused(call(objs, no, lights, nl, g, s=box), "enableSkyBox", want=UNSUPPORTED)
    res = abi.RmResources()
    for f in range(5):
        res.skybox[f] = tex
    assert refused(call(objs, no, lights, nl, g, s=box, res=res), "enableSkyBox", want=UNSUPPORTED)
    res.skybox[5] = tex
    assert refused(call(objs, no, lights, nl, g, s=box, res=res, rays=None), text=ARRAYS)
    objs[0].texLoc = 0
    assert refused(call(objs, no, lights, nl, g), "texLoc", want=UNSUPPORTED)
    res = abi.RmResources()
    arr = (abi.RmTexture * 1)(tex)
    res.textures, res.numTextures = arr, 1
    assert refused(call(objs, no, lights, nl, g, res=res, rays=None), text=ARRAYS)
    objs[0].texLoc = 1
    assert refused(call(objs, no, lights, nl, g, res=res), "texLoc", want=UNSUPPORTED)
    objs[0].texLoc = -1
    objs[2].texLoc = 0  # a torus takes no texture
    assert refused(call(objs, no, lights, nl, g, res=res), "textures are only defined", want=UNSUPPORTED)
    objs[2].texLoc = -1
    res.numTextures = abi.RM_MAX_TEXTURES + 1
    assert refused(call(objs, no, lights, nl, g, res=res), "RM_MAX_TEXTURES", want=CAPACITY)
    scene = SB.area_light_scene(8, 8)
    assert refused(call(*scene[1:6]), "LTC", want=UNSUPPORTED)
    res = abi.RmResources()
    res.ltc1 = 0x3000
    assert refused(call(*scene[1:6], res=res), "LTC", want=UNSUPPORTED)
    res.ltc2 = 0x4000
    assert refused(call(*scene[1:6], res=res, rgba=None), text=ARRAYS)


def test_the_three_arrays():
    objs, no, lights, nl, g = _scene()
    assert refused(call(objs, no, lights, nl, g, rays=None), text=ARRAYS)
    assert refused(call(objs, no, lights, nl, g, rgba=None), text=ARRAYS)
    for off in (4, 8, 12, 1):
        bad = fake(0x1000 + off)
        assert refused(call(objs, no, lights, nl, g, rays=bad), text="16-byte aligned"), off
        assert refused(call(objs, no, lights, nl, g, rgba=bad), text="16-byte aligned"), off
        assert refused(call(objs, no, lights, nl, g, bright=bad), text="16-byte aligned"), off
    # the arrays come behind everything about the scene
    objs[0].type = abi.RM_CUSTOM
    assert refused(call(objs, no, lights, nl, g, rays=None), "object 0", want=UNSUPPORTED)
    objs[0].type = abi.RM_SPHERE
    # host memory is not device memory: the only check that asks the HIP runtime, and the last
    assert refused(call(objs, no, lights, nl, g, rays=HP, rgba=HP), text="d_rays")
