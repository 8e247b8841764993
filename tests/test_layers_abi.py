"""rm_shade_rays_layers and rm_trace_rays_layers without a GPU: the header declares them and the library exports them under the
unchanged ABI version, the comments carry the definitions, the Python methods have the documented signatures, and every argument
error returns its status, in the documented order, before the first HIP call — with pointers that would fault if read."""
import ctypes as C
import inspect
import re

import abi_helpers as ah
import helpers as h
from abi_helpers import CAPACITY, FAKE, HEADER, HP, INT_MAX, fake, refused
from raymarcher_amd import abi, lib
from raymarcher_amd._lib import SIGNATURES
from scene_builders import three_primitives_lit as _scene

UNSUPPORTED = abi.RM_ERR_UNSUPPORTED
TERRAIN, CLOUD, SEA = abi.RM_FEAT_TERRAIN, abi.RM_FEAT_CLOUD, abi.RM_FEAT_SEA
LAYER_MASKS = (TERRAIN, CLOUD, SEA, TERRAIN | abi.RM_FEAT_PERLIN_BUMP, TERRAIN | CLOUD | SEA | abi.RM_FEAT_SKY_BACKGROUND)


# ---------------------------------------------------------------- the symbols and the written definitions
def test_header_declares_and_library_exports_both_symbols():
    assert ah.params("rm_shade_rays_layers") == [
        "const RmRay *d_rays", "int numRays", "float far", "int imageWidth", "const RmObject *objs", "int numObjects",
        "const RmLight *lights", "int numLights", "const RmGlobals *g", "const RmSettings *s", "const RmResources *res", "float *d_rgba",
        "float *d_bright", "void *stream"]
    assert ah.params("rm_trace_rays_layers") == [
        "const RmRay *d_rays", "int numRays", "int imageWidth", "const RmObject *objs", "int numObjects", "const RmGlobals *g",
        "const RmSettings *s", "unsigned mode", "RmRayHit *d_hits", "void *stream"]
    # the old symbols' arguments with imageWidth put in: nothing else moved
    old = ah.params("rm_shade_rays")
    assert ah.params("rm_shade_rays_layers") == old[:3] + ["int imageWidth"] + old[3:]
    old = ah.params("rm_trace_rays")
    assert ah.params("rm_trace_rays_layers") == old[:2] + ["int imageWidth"] + old[2:]
    s, t = SIGNATURES["rm_shade_rays"], SIGNATURES["rm_trace_rays"]
    assert SIGNATURES["rm_shade_rays_layers"] == (C.c_int, s[1][:3] + [C.c_int] + s[1][3:])
    assert SIGNATURES["rm_trace_rays_layers"] == (C.c_int, t[1][:2] + [C.c_int] + t[1][2:])
    ah.assert_exported(["rm_shade_rays_layers", "rm_trace_rays_layers"])  # bindings detect the symbols by lookup
    ah.assert_abi_version()
    for name, val in (("RM_HIT_SEA", r"\(-3\)"), ("RM_HIT_TERRAIN", r"\(-4\)")):
        assert re.search(rf"#define\s+{name}\s+{val}", HEADER), name
    assert (abi.RM_HIT_SEA, abi.RM_HIT_TERRAIN, abi.RM_PATH_SHADE_RAYS_LAYERS, abi.RM_PATH_TRACE_RAYS_LAYERS) == (-3, -4, 14, 15)


def test_header_comments_carry_the_definitions():
    ah.assert_comment_has("rm_shade_rays_layers", (
        "imageWidth", "iResolution.x", "frag:2284-2310", "frag:2444-2456", "frag:2459-2475", "frag:2506-2518", "frag:2555-2567",
        "frag:2422-2426", "validated but NOT read", "cloud over terrain over sea over the object hit", "fires no secondary rays",
        "in every bit", "before any HIP call", "rm_debug_last_path() = 14", "symbol lookup", "RM_ERR_INVALID_ARGUMENT",
        "isTwoD"))
    ah.assert_comment_has("rm_trace_rays_layers", (
        "raymarch(origin, dir, tMax, OUTSIDE)", "frag:2284-2291, 2252-2282", "frag:2128-2135, 2060-2090; tmin = 15",
        "frag:2106-2111", "frag:2243-2250", "RM_HIT_TERRAIN (−4)", "RM_HIT_SEA (−3)", "a collision response needs the surface",
        "not the fbm-perturbed", "(dot(d, d)·0.1) / imageWidth", "a volume has no closest hit", "RM_TRACE_NO_NORMAL",
        "does not see the layers", "does not touch the noise texture", "does not depend on which other rays",
        "before any HIP call", "rm_debug_last_path() = 15", "symbol lookup"))
    assert re.search(r"14 = a launch of rm_shade_rays_layers, 15 = a\s+\*?\s*launch of rm_trace_rays_layers", HEADER), \
        "rm_debug_last_path's comment does not document 14 and 15"
    timing = ah.comment_before("rm_get_stage_timing")
    assert "rm_shade_rays_layers" in timing and "rm_trace_rays_layers" in timing


def test_python_signatures():
    from raymarcher_amd.render import Renderer
    sig = inspect.signature(Renderer.shade_rays_layers)
    assert list(sig.parameters) == ["self", "tables", "settings", "rays", "image_width", "far", "bright", "out", "out_bright"]
    assert sig.parameters["image_width"].default is inspect.Parameter.empty
    assert sig.parameters["far"].default is None and sig.parameters["bright"].default is False
    assert sig.parameters["out"].default is None and sig.parameters["out_bright"].default is None
    sig = inspect.signature(Renderer.trace_rays_layers)
    assert list(sig.parameters) == ["self", "tables", "settings", "rays", "image_width", "normals", "out"]
    assert sig.parameters["normals"].default is True and sig.parameters["out"].default is None
    sig = inspect.signature(Renderer.render_panorama_layers)
    assert list(sig.parameters) == ["self", "tables", "settings", "W", "H", "position", "forward", "up", "far"]
    old = inspect.signature(Renderer.render_panorama)
    assert [p.default for p in sig.parameters.values()] == [p.default for p in old.parameters.values()]


# ---------------------------------------------------------------- refusals, all without a device
DEFAULT = object()
SHADE_ARRAYS = "null d_rays or d_rgba"  # the first check behind the scene's: a call that gets this far passed everything before it
TRACE_ARRAYS = "null d_rays or d_hits"


def _noise():
    res = abi.RmResources()
    res.noise = abi.RmTexture(0x2000, 4, 4)  # a fake pointer, never read
    return res


def shade(objs, no, lights, nl, g, s=DEFAULT, n=100, far=100.0, width=64, res=None, rays=FAKE, rgba=FAKE, bright=None):
    s = abi.default_settings() if s is DEFAULT else s
    return lib().rm_shade_rays_layers(rays, n, far, width, objs, no, lights, nl, C.byref(g) if g is not None else None,
                                      C.byref(s) if s is not None else None, C.byref(res) if res is not None else None, rgba, bright, None)


def trace(objs, no, g, s=DEFAULT, n=100, width=64, mode=0, rays=FAKE, hits=FAKE):
    s = abi.default_settings() if s is DEFAULT else s
    return lib().rm_trace_rays_layers(rays, n, width, objs, no, C.byref(g) if g is not None else None,
                                      C.byref(s) if s is not None else None, mode, hits, None)


def feat(bits, **over):
    return abi.default_settings(features=bits, **over)


def test_counts_and_scene_pointers():
    objs, no, lights, nl, g = _scene()
    for n in (-1, -INT_MAX):
        assert refused(shade(objs, no, lights, nl, g, n=n), text="numRays")
        assert refused(trace(objs, no, g, n=n), text="numRays")
    # numRays == 0: RM_OK with null everything and any imageWidth, nothing is read
    assert shade(objs, no, lights, nl, g, n=0, rays=None, rgba=None) == abi.RM_OK
    assert shade(None, 5, None, -3, None, s=None, n=0, far=float("nan"), width=-7, rays=None, rgba=None) == abi.RM_OK
    assert trace(None, 5, None, s=None, n=0, width=0, mode=77, rays=None, hits=None) == abi.RM_OK
    # every positive int fits one grid: INT_MAX rays get as far as the scene pointers
    assert refused(shade(objs, no, lights, nl, None, n=INT_MAX), text="null scene pointer")
    assert refused(trace(objs, no, None, n=INT_MAX), text="null scene pointer")
    assert refused(shade(objs, no, lights, nl, g, s=None), text="null scene pointer")
    assert refused(shade(None, no, lights, nl, g), text="null scene pointer")
    assert refused(shade(objs, no, None, nl, g), text="null scene pointer")
    assert refused(shade(objs, -1, lights, nl, g), text="null scene pointer")
    assert refused(shade(objs, no, lights, -1, g), text="null scene pointer")
    assert refused(trace(objs, no, g, s=None), text="null scene pointer")
    assert refused(trace(None, no, g), text="null scene pointer")
    assert refused(trace(objs, -1, g), text="null scene pointer")
    # the scene pointers come before far, the mode bits and imageWidth
    assert refused(shade(objs, no, lights, nl, None, far=-1.0, width=0), text="null scene pointer")
    assert refused(trace(objs, no, None, mode=4, width=0), text="null scene pointer")


def test_image_width():
    """imageWidth >= 1 in every call, whatever the feature mask: right behind far (shade) and the mode bits (trace)."""
    objs, no, lights, nl, g = _scene()
    for bits in (0, abi.RM_FEAT_REFERENCE_DEFAULT) + LAYER_MASKS:
        for width in (0, -1, -INT_MAX):
            assert refused(shade(objs, no, lights, nl, g, s=feat(bits), width=width, res=_noise()), text="imageWidth"), (bits, width)
            assert refused(trace(objs, no, g, s=feat(bits), width=width), text="imageWidth"), (bits, width)
            assert refused(trace(objs, no, g, s=feat(bits), width=width, mode=abi.RM_TRACE_OCCLUSION), text="imageWidth"), (bits, width)
        for width in (1, 64, INT_MAX):
            assert refused(shade(objs, no, lights, nl, g, s=feat(bits), width=width, res=_noise(), rays=None), text=SHADE_ARRAYS), (bits, width)
            assert refused(trace(objs, no, g, s=feat(bits), width=width, hits=None), text=TRACE_ARRAYS), (bits, width)
    # far and the mode bits come first, everything about the scene's content after
    for far in (float("nan"), -1.0, float("inf")):
        assert refused(shade(objs, no, lights, nl, g, far=far, width=0), text="far"), far
    for mode in (4, 0x80000000):
        assert refused(trace(objs, no, g, mode=mode, width=0), text="unknown mode bits"), mode
    assert refused(trace(objs, no, g, mode=abi.RM_TRACE_NO_NORMAL | abi.RM_TRACE_OCCLUSION, width=0), text="RM_TRACE_NO_NORMAL")
    two_d = h.make_globals(two_d=1)
    assert refused(shade(objs, no, lights, nl, two_d, width=0), text="imageWidth")
    assert refused(trace(objs, no, two_d, width=0), text="imageWidth")
    assert refused(trace(objs, no, two_d, s=feat(SEA), width=0, mode=abi.RM_TRACE_OCCLUSION), text="imageWidth")
    many = (abi.RmObject * (abi.RM_MAX_OBJECTS + 1))(*[h.make_object(abi.RM_SPHERE) for _ in range(abi.RM_MAX_OBJECTS + 1)])
    assert refused(shade(many, abi.RM_MAX_OBJECTS + 1, lights, nl, g, width=0), text="imageWidth")
    assert refused(trace(many, abi.RM_MAX_OBJECTS + 1, g, width=0), text="imageWidth")
    assert refused(shade(objs, no, lights, nl, g, s=feat(SEA), width=0), text="imageWidth")  # ahead of the missing noise sampler


def test_the_layers_are_accepted_and_occlusion_with_one_is_refused():
    objs, no, lights, nl, g = _scene()
    for bits in LAYER_MASKS:
        assert refused(shade(objs, no, lights, nl, g, s=feat(bits), res=_noise(), rays=None), text=SHADE_ARRAYS), bits
        for mode in (abi.RM_TRACE_CLOSEST, abi.RM_TRACE_NO_NORMAL):
            assert refused(trace(objs, no, g, s=feat(bits), mode=mode, rays=None), text=TRACE_ARRAYS), (bits, mode)
        assert refused(trace(objs, no, g, s=feat(bits), mode=abi.RM_TRACE_OCCLUSION), "RM_TRACE_OCCLUSION", want=UNSUPPORTED), bits
        assert "TERRAIN / CLOUD / SEA" in lib().rm_last_error().decode()
    for bits in (0, abi.RM_FEAT_SKY_BACKGROUND, abi.RM_FEAT_REFERENCE_DEFAULT):  # without a layer bit occlusion is rm_trace_rays'
        assert refused(trace(objs, no, g, s=feat(bits), mode=abi.RM_TRACE_OCCLUSION, rays=None), text=TRACE_ARRAYS), bits
    # occlusion with a layer comes before the 2-D mode and the table's content
    assert refused(trace(objs, no, h.make_globals(two_d=1), s=feat(CLOUD), mode=abi.RM_TRACE_OCCLUSION), "RM_TRACE_OCCLUSION", want=UNSUPPORTED)
    objs[1].type = abi.RM_CUSTOM
    assert refused(trace(objs, no, g, s=feat(TERRAIN), mode=abi.RM_TRACE_OCCLUSION), "RM_TRACE_OCCLUSION", want=UNSUPPORTED)
    assert refused(trace(objs, no, g, s=feat(TERRAIN)), "object 1", want=UNSUPPORTED)


def test_the_sea_needs_the_noise_sampler_to_shade_and_not_to_trace():
    objs, no, lights, nl, g = _scene()
    for bits in (SEA, SEA | TERRAIN | CLOUD, SEA | abi.RM_FEAT_SKY_BACKGROUND):
        assert refused(shade(objs, no, lights, nl, g, s=feat(bits)), "noise", want=UNSUPPORTED), bits
        assert refused(shade(objs, no, lights, nl, g, s=feat(bits), res=abi.RmResources()), "noise", want=UNSUPPORTED), bits
        assert "supply RmResources.noise" in lib().rm_last_error().decode()  # rm_render_res's text
        assert refused(shade(objs, no, lights, nl, g, s=feat(bits), res=_noise(), rays=None), text=SHADE_ARRAYS), bits
        assert refused(trace(objs, no, g, s=feat(bits), rays=None), text=TRACE_ARRAYS), bits  # the sea's geometry reads no sampler
    for bits in (TERRAIN, CLOUD, TERRAIN | CLOUD):
        assert refused(shade(objs, no, lights, nl, g, s=feat(bits), rays=None), text=SHADE_ARRAYS), bits


def test_two_d_capacity_loop_bounds_and_types_in_order():
    objs, no, lights, nl, g = _scene()
    two_d = h.make_globals(two_d=1)
    many = (abi.RmObject * (abi.RM_MAX_OBJECTS + 1))(*[h.make_object(abi.RM_SPHERE) for _ in range(abi.RM_MAX_OBJECTS + 1)])
    lots = (abi.RmLight * (abi.RM_MAX_LIGHTS + 1))(*[h.make_light(abi.RM_LIGHT_POINT) for _ in range(abi.RM_MAX_LIGHTS + 1)])
    for bits in (abi.RM_FEAT_REFERENCE_DEFAULT, TERRAIN | CLOUD):
        assert refused(shade(objs, no, lights, nl, two_d, s=feat(bits)), "isTwoD", want=UNSUPPORTED), bits
        assert refused(trace(objs, no, two_d, s=feat(bits)), "isTwoD", want=UNSUPPORTED), bits
        assert refused(shade(many, abi.RM_MAX_OBJECTS + 1, lights, nl, g, s=feat(bits)), "RM_MAX_OBJECTS", want=CAPACITY), bits
        assert refused(trace(many, abi.RM_MAX_OBJECTS + 1, g, s=feat(bits)), "RM_MAX_OBJECTS", want=CAPACITY), bits
        assert refused(shade(many, abi.RM_MAX_OBJECTS, lights, nl, g, s=feat(bits), rays=None), text=SHADE_ARRAYS), bits
        assert refused(trace(many, abi.RM_MAX_OBJECTS, g, s=feat(bits), rays=None), text=TRACE_ARRAYS), bits
        assert refused(shade(objs, no, lots, abi.RM_MAX_LIGHTS + 1, g, s=feat(bits)), "RM_MAX_LIGHTS", want=CAPACITY), bits
        assert refused(shade(objs, no, lots, abi.RM_MAX_LIGHTS, g, s=feat(bits), rays=None), text=SHADE_ARRAYS), bits
        for field in ("maxSteps", "fractalIters", "mengerLevels", "numReflection"):
            assert refused(shade(objs, no, lights, nl, g, s=feat(bits, **{field: -1})), text="loop bound"), (bits, field)
        for field in ("maxSteps", "fractalIters", "mengerLevels"):
            assert refused(trace(objs, no, g, s=feat(bits, **{field: -1})), text="loop bound"), (bits, field)
        # the 2-D mode comes before the capacity, the capacity before the loop bounds
        assert refused(shade(many, abi.RM_MAX_OBJECTS + 1, lights, nl, two_d, s=feat(bits)), "isTwoD", want=UNSUPPORTED), bits
        assert refused(trace(many, abi.RM_MAX_OBJECTS + 1, two_d, s=feat(bits)), "isTwoD", want=UNSUPPORTED), bits
        assert refused(shade(many, abi.RM_MAX_OBJECTS + 1, lights, nl, g, s=feat(bits, maxSteps=-1)), want=CAPACITY), bits
        assert refused(trace(many, abi.RM_MAX_OBJECTS + 1, g, s=feat(bits, maxSteps=-1)), want=CAPACITY), bits
    # the loop bounds come before the types
    layers = feat(TERRAIN | CLOUD)
    objs[1].type = abi.RM_CUSTOM
    assert refused(shade(objs, no, lights, nl, g, s=feat(TERRAIN | CLOUD, maxSteps=-1)), text="loop bound")
    assert refused(trace(objs, no, g, s=feat(TERRAIN | CLOUD, maxSteps=-1)), text="loop bound")
    assert refused(shade(objs, no, lights, nl, g, s=layers), "object 1", want=UNSUPPORTED) and "CUSTOM" in lib().rm_last_error().decode()
    assert refused(trace(objs, no, g, s=layers), "object 1", want=UNSUPPORTED) and "CUSTOM" in lib().rm_last_error().decode()
    for ty in (99, -1):
        objs[1].type = abi.RM_CUBE
        objs[2].type = ty
        assert refused(shade(objs, no, lights, nl, g, s=layers), "object 2", want=UNSUPPORTED), ty
        assert refused(trace(objs, no, g, s=layers), "object 2", want=UNSUPPORTED), ty
    objs[2].type = abi.RM_TORUS
    lights[1].type = 7
    assert refused(shade(objs, no, lights, nl, g, s=layers), "light 1", want=UNSUPPORTED)
    assert refused(trace(objs, no, g, s=layers, rays=None), text=TRACE_ARRAYS)  # a trace reads no light


def test_the_arrays():
    objs, no, lights, nl, g = _scene()
    layers = feat(TERRAIN | CLOUD | abi.RM_FEAT_SKY_BACKGROUND)
    for s in (DEFAULT, layers):
        assert refused(shade(objs, no, lights, nl, g, s=s, rays=None), text=SHADE_ARRAYS)
        assert refused(shade(objs, no, lights, nl, g, s=s, rgba=None), text=SHADE_ARRAYS)
        assert refused(trace(objs, no, g, s=s, rays=None), text=TRACE_ARRAYS)
        assert refused(trace(objs, no, g, s=s, hits=None), text=TRACE_ARRAYS)
        assert refused(trace(None, 0, g, s=s, hits=None), text=TRACE_ARRAYS)  # an empty table needs no pointer
        assert refused(shade(None, 0, None, 0, g, s=s, rays=None), text=SHADE_ARRAYS)
        for off in (4, 8, 12, 1):
            bad = fake(0x1000 + off)
            assert refused(shade(objs, no, lights, nl, g, s=s, rays=bad), text="16-byte aligned"), off
            assert refused(shade(objs, no, lights, nl, g, s=s, rgba=bad), text="16-byte aligned"), off
            assert refused(shade(objs, no, lights, nl, g, s=s, bright=bad), text="16-byte aligned"), off
            assert refused(trace(objs, no, g, s=s, rays=bad), text="16-byte aligned"), off
            assert refused(trace(objs, no, g, s=s, hits=bad), text="16-byte aligned"), off
    # the arrays come behind everything about the scene
    objs[0].type = abi.RM_CUSTOM
    assert refused(shade(objs, no, lights, nl, g, s=layers, rays=None), "object 0", want=UNSUPPORTED)
    assert refused(trace(objs, no, g, s=layers, rays=None), "object 0", want=UNSUPPORTED)
    objs[0].type = abi.RM_SPHERE
    # host memory is not device memory: the only check that asks the HIP runtime, and the last
    assert refused(shade(objs, no, lights, nl, g, s=layers, rays=HP, rgba=HP), text="d_rays")
    assert refused(trace(objs, no, g, s=layers, rays=HP, hits=HP), text="d_rays")
