"""The specification of rm_shade_rays for the tests: tests/shade_spec/rm_shade_spec.c, which includes the oracle's source and restates
its shadePixel from the background colour on for a given (ro, rd, far), built on demand and loaded with ctypes by
helpers.load_spec.  Nothing under oracle/ is touched.  Also the scenes, one or more per kernel class, that more than one shade test
module uses."""
import ctypes as C
import functools

import numpy as np

import helpers as h
import scene_builders as SB
from raymarcher_amd import abi

P = C.POINTER
SIGNATURES = {"rmo_spec_shade": (C.c_int, [P(abi.RmObject), C.c_int, P(abi.RmLight), C.c_int, P(abi.RmGlobals), P(abi.RmSettings),
                                           P(abi.RmResources), P(C.c_float), C.c_int, C.c_float, P(C.c_float), P(C.c_float)])}
PATH_SHADE = 13  # rm_debug_last_path() of a launch of rm_shade_rays
tables_of, assert_bits = h.tables_of, h.assert_bit_equal


def spec():
    """ctypes handle of the spec library (helpers.load_spec: rebuilt when a source it is made of is newer)."""
    return h.load_spec("shade", SIGNATURES)


def spec_shade(scene, s, rays, far, res=None, expect=0):
    """(colour, bright), float32 (n, 4) each, of `rays` (float32 (n, 8)) by the specification.  scene: the tests' tuple (camera,
    objects, count, lights, count, globals) — the camera is not read; res: the resources dict of scene_builders.resource_case."""
    rays = np.ascontiguousarray(rays, dtype=np.float32)
    col = np.full((len(rays), 4), np.nan, dtype=np.float32)
    br = np.full((len(rays), 4), np.nan, dtype=np.float32)
    r, _keep = h.host_resources(**(res or {}))
    _, objs, no, lights, nl, g = scene[:6]
    st = spec().rmo_spec_shade(objs, no, lights, nl, C.byref(g), C.byref(s), C.byref(r), h.fptr(rays), len(rays), far, h.fptr(col),
                               h.fptr(br))
    assert st == expect, f"spec status {st}"
    return col, br


def _with_materials(scene, reflective):
    """A copy of the scene whose objects all have cReflective = reflective."""
    cam, objs, no, lights, nl, g = scene
    o = (abi.RmObject * max(no, 1))(*[abi.RmObject.from_buffer_copy(bytes(objs[i])) for i in range(no)])
    for i in range(no):
        for k in range(3):
            o[i].cReflective[k] = reflective
    return cam, o, no, lights, nl, g


# name → ((BULB, ENV, TEX, SEC) of the kernel class the launcher must pick, builder(W, H) → (scene, settings, resources)).  BULB: 0 the
# table walk, 1 the general bulb, 2 the plain bulb.  One scene or more per class of dispatch_class, from scene_builders;
# every bulb case has hard shadows from directional lights only, the shadow pool's case.
def _cases():
    SKY, WB = abi.RM_FEAT_SKY_BACKGROUND, abi.RM_FEAT_WHITE_BACKGROUND
    ds = abi.default_settings

    def menger(W, H, refl):
        sc = SB.menger_scene(W, H)
        return (sc[:5] + (h.make_globals(itime=7.5),)), ds(mengerLevels=3, enableReflection=refl), {}

    def bulb(builder, refl):
        def make(W, H):
            sc = builder(W, H)
            return (_with_materials(sc, 0.5) if refl else sc), ds(fractalIters=8, enableReflection=refl), {}
        return make

    def resource(name, **over):
        def make(W, H):
            scene, s, res = SB.resource_case(name, W, H)
            for k, v in over.items():
                setattr(s, k, v)
            return scene, s, res
        return make

    def textured(feat):
        return lambda W, H: (SB.textured_scene(W, H), ds(features=feat), {"textures": SB.synthetic_textures()})

    def empty(W, H):
        cam = h.make_camera((0, 0, 4.5), (0, 0, -4.5), (0, 1, 0), 30.0, W, H)
        objs, _ = h.table([])
        return (cam, objs, 0, None, 0, h.make_globals()), ds(), {}

    return {
        "generic_nosec": ((0, 0, 0, 0), lambda W, H: (SB.directional_light_2(W, H), ds(enableSoftShadow=1, enableAmbientOcclusion=1), {})),
        "generic_sec": ((0, 0, 0, 1), lambda W, H: (SB.reflect_refract_scene(W, H),
                                                    ds(enableReflection=1, enableRefraction=1, numReflection=2), {})),
        "menger_sec": ((0, 0, 0, 1), lambda W, H: menger(W, H, 1)),
        "menger_nosec": ((0, 0, 0, 0), lambda W, H: menger(W, H, 0)),
        "plain_bulb_nosec": ((2, 0, 0, 0), bulb(h.scene_mandelbulb, 0)),
        "plain_bulb_sec": ((2, 0, 0, 1), bulb(h.scene_mandelbulb, 1)),
        "moved_bulb_nosec": ((1, 0, 0, 0), bulb(SB.moved_bulb_scene, 0)),
        "moved_bulb_sec": ((1, 0, 0, 1), bulb(SB.moved_bulb_scene, 1)),
        "tex_nosec": ((0, 0, 1, 0), textured(WB)),
        "tex_sec": ((0, 0, 1, 1), resource("skybox_reflect")),
        "area_light": ((0, 0, 1, 1), resource("area_light")),
        "env_sec": ((0, 1, 0, 1), resource("night_sky")),
        "env_nosec": ((0, 1, 0, 0), resource("night_sky", enableReflection=0)),
        "envtex_nosec": ((0, 1, 1, 0), textured(SKY | abi.RM_FEAT_PERLIN_BUMP)),
        "envtex_sec": ((0, 1, 1, 1), resource("skybox_reflect", features=SKY)),
        "empty": ((0, 0, 0, 0), empty),
    }


CASES = _cases()
CLASSES = sorted({c for c, _ in CASES.values()})
assert len(CLASSES) == 12, "the cases must cover the twelve kernel classes"


@functools.lru_cache(maxsize=None)
def case(name, W=8, H=8):
    """(scene, settings, resources) of a case; W, H only shape the camera, which rm_shade_rays does not read."""
    return CASES[name][1](W, H)


def class_of(scene, s):
    """The (BULB, ENV, TEX, SEC) that rm_frame.cpp's classify_frame and bulb_class give a call without layers, restated from their
    comments: what the launcher must pick for the case, checked against the case's own label."""
    from raymarcher_amd import lib
    _, objs, no, lights, nl, g = scene[:6]
    env = int(bool(s.features & (abi.RM_FEAT_SKY_BACKGROUND | abi.RM_FEAT_NIGHTSKY_BACKGROUND)))
    tex = int(bool(s.enableSkyBox) or any(objs[i].texLoc != -1 or objs[i].isEmissive for i in range(no)) or
              any(lights[i].type == abi.RM_LIGHT_AREA for i in range(nl)))
    refl = any(any(objs[i].cReflective[k] != 0.0 for k in range(3)) for i in range(no))
    tran = any(any(objs[i].cTransparent[k] != 0.0 for k in range(3)) for i in range(no))
    sec = int(bool((s.enableReflection and refl and s.numReflection > 0) or (s.enableRefraction and tran)))
    bulb = 0
    if no == 1 and objs[0].type == abi.RM_MANDELBULB and not env and not tex:
        bulb = 2 if lib().rm_debug_bulb_plain(objs, 1, C.byref(g)) == 1 else 1
    return bulb, env, tex, sec


def normalised(rays):
    """The rays with their directions normalised in float32 (v · (1 / |v|)); invalid rays stay as they are."""
    out = np.array(rays, dtype=np.float32)
    d = out[:, 4:7]
    with np.errstate(all="ignore"):
        n = np.sqrt((d * d).sum(axis=1, dtype=np.float32), dtype=np.float32)
        ok = np.isfinite(n) & (n > 0)
        d[ok] = d[ok] * (np.float32(1.0) / n[ok])[:, None]
    return out


