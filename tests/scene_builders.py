"""The scenes and resources that more than one test module, script or tool builds: the tests' scene tuple is (camera, objects,
count, lights, count, globals).  Helpers and builders used by more than one module live here or in helpers.py, never in a test_*
module.  Every builder returns fresh objects on every call.  Needs neither torch nor the HIP library at import time."""
import math
import os

import numpy as np

import helpers as h
from raymarcher_amd import abi

SCENES = os.path.join(os.path.dirname(__file__), "golden", "scenes")


def scene_tuple(t):
    return t.camera, t.objects, t.num_objects, t.lights, t.num_lights, t.globals_


def ieq(a, b):
    import torch
    return bool((a.view(dtype=torch.int32) == b.view(dtype=torch.int32)).all())


def rot_x(a):
    M = np.eye(4)
    M[1, 1], M[1, 2], M[2, 1], M[2, 2] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a)
    return M


def rot_y(v, deg):
    a = math.radians(deg)
    return (v[0] * math.cos(a) + v[2] * math.sin(a), v[1], -v[0] * math.sin(a) + v[2] * math.cos(a))


def orbit(pos, look, fov, W, H, n, deg=4.0, far=100.0):
    """n cameras turned about the y axis by deg degrees per frame (position and view direction)."""
    return [h.make_camera(rot_y(pos, deg * i), rot_y(look, deg * i), (0, 1, 0), fov, W, H, far=far) for i in range(n)]


def batch(n, W=32, H=24):
    """max(n, 1) equal cameras on helpers.scene_mandelbulb, one RmGlobals per camera 0.1 apart in iTime → (cameras, globals, scene)."""
    cams = (abi.RmCamera * max(n, 1))(*[h.make_camera((0, 0, 4.5), (0, 0, -1), (0, 1, 0), 30.0, W, H) for _ in range(max(n, 1))])
    globs = (abi.RmGlobals * max(n, 1))(*[h.make_globals(itime=0.1 * i) for i in range(max(n, 1))])
    return cams, globs, h.scene_mandelbulb(W, H)


def three_primitives():
    """A sphere, a cube and a torus, each moved one unit its own way → (objects, 3, globals)."""
    objs = (abi.RmObject * 3)(h.make_object(abi.RM_SPHERE, model=h.translate(-1, 0, 0)), h.make_object(abi.RM_CUBE, model=h.translate(1, 0, 0)),
                              h.make_object(abi.RM_TORUS, model=h.translate(0, 1, 0)))
    return objs, 3, h.make_globals()


def three_primitives_lit():
    """three_primitives under a directional and a point light → (objects, 3, lights, 2, globals)."""
    objs, no, g = three_primitives()
    lights = (abi.RmLight * 2)(h.make_light(abi.RM_LIGHT_DIRECTIONAL, (1, 1, 1), (0, -1, 0)), h.make_light(abi.RM_LIGHT_POINT, pos=(1, 2, 3)))
    return objs, no, lights, 2, g


def three_primitives_table():
    """helpers.table of a sphere and a cube one unit left and right and a torus at the origin → (objects, 3, globals)."""
    objs, no = h.table([h.make_object(abi.RM_SPHERE, model=h.translate(-1, 0, 0)), h.make_object(abi.RM_CUBE, model=h.translate(1, 0, 0)),
                        h.make_object(abi.RM_TORUS)])
    return objs, no, h.make_globals()


def all_primitives_scene(W=64, H=64):
    cam = h.make_camera((0, 0, 6), (0, 0, -1), (0, 1, 0), 45.0, W, H)
    types = [abi.RM_CUBE, abi.RM_CONE, abi.RM_CYLINDER, abi.RM_SPHERE, abi.RM_OCTAHEDRON, abi.RM_TORUS, abi.RM_CAPSULE,
             abi.RM_DEATHSTAR, abi.RM_RECTANGLE, abi.RM_SIERPINSKI, abi.RM_MENGERSPONGE, abi.RM_MANDELBULB]
    objs = (abi.RmObject * len(types))()
    for i, t in enumerate(types):
        gx, gy = (i % 4) - 1.5, (i // 4) - 1.0
        M = h.translate(1.6 * gx, 1.6 * gy, 0.0) @ h.scale(0.9, 0.8 + 0.05 * i, 0.9)
        objs[i] = h.make_object(t, model=M, scale_factor=min(0.9, 0.8 + 0.05 * i), ambient=(.2, .2, .2),
                                diffuse=(0.3 + 0.05 * i, 0.8, 1.0 - 0.05 * i), specular=(1, 1, 1), shininess=15.0 + i)
    lights = (abi.RmLight * 3)(
        h.make_light(abi.RM_LIGHT_DIRECTIONAL, (1, 1, 1), (-0.3, -1, -0.6)),
        h.make_light(abi.RM_LIGHT_POINT, (1, 0.8, 0.6), pos=(3, 3, 4), func=(0.5, 0.1, 0.01)),
        h.make_light(abi.RM_LIGHT_SPOT, (0.7, 0.8, 1), direction=(0, -1, -1), pos=(0, 5, 5), func=(0.8, 0.02, 0.0),
                     angle=np.deg2rad(35.0), penumbra=np.deg2rad(12.0)))
    return cam, objs, len(types), lights, 3, h.make_globals()


def env_scene(W, H, pos=(0, 500, 5), look=(0.3, 0.12, -1)):
    """Terrain + volumetric cloud + sky (the shader's TERRAIN / CLOUD / SKY_BACKGROUND defines), with a reflective
    torus floating in front of the camera so secondary rays also see the layers (frag:2506-2518)."""
    cam = h.make_camera(pos, look, (0, 1, 0), 70.0, W, H, far=2000.0)
    objs = (abi.RmObject * 1)(h.make_object(abi.RM_TORUS, model=h.translate(8, pos[1] + 3, -30) @ h.scale(12, 12, 12),
                                            scale_factor=12, ambient=(.3, .3, .3), specular=(1, 1, 1), shininess=50,
                                            reflective=(.6, .6, .6), transparent=(.5, .5, .5), ior=1.3))
    lights = (abi.RmLight * 1)(h.make_light(abi.RM_LIGHT_DIRECTIONAL, (3, 2.6, 2.0), (-0.577, -0.577, 0.577)))
    return cam, objs, 1, lights, 1, h.make_globals()


ENV_ALL = abi.RM_FEAT_SKY_BACKGROUND | abi.RM_FEAT_TERRAIN | abi.RM_FEAT_CLOUD | abi.RM_FEAT_PERLIN_BUMP


def reflect_refract_scene(W, H):
    cam = h.make_camera((0, 1.2, 5), (0, -0.2, -1), (0, 1, 0), 40.0, W, H)
    objs = (abi.RmObject * 4)(
        h.make_object(abi.RM_SPHERE, model=h.translate(-1.1, 0, 0) @ h.scale(1.6, 1.6, 1.6), scale_factor=1.6,
                      ambient=(.1, .1, .1), diffuse=(.8, .2, .2), specular=(1, 1, 1), shininess=30, reflective=(.8, .8, .8)),
        h.make_object(abi.RM_SPHERE, model=h.translate(1.1, 0, 0.3) @ h.scale(1.5, 1.5, 1.5), scale_factor=1.5,
                      ambient=(.1, .1, .1), diffuse=(.2, .3, .8), specular=(1, 1, 1), shininess=50,
                      transparent=(.9, .9, .9), ior=1.4),
        h.make_object(abi.RM_CUBE, model=h.translate(0, -1.3, 0) @ h.scale(8, 1, 8), scale_factor=1.0,
                      ambient=(.2, .2, .2), diffuse=(.6, .6, .5), specular=(.3, .3, .3), shininess=5, reflective=(.3, .3, .3)),
        h.make_object(abi.RM_TORUS, model=h.translate(0.2, 0.4, -2.0) @ h.scale(2, 2, 2), scale_factor=2.0,
                      ambient=(.1, .2, .1), diffuse=(.3, .9, .3), specular=(1, 1, 1), shininess=10))
    lights = (abi.RmLight * 2)(
        h.make_light(abi.RM_LIGHT_DIRECTIONAL, (1, 1, 1), (-0.5, -1, -0.4)),
        h.make_light(abi.RM_LIGHT_POINT, (.8, .8, 1), pos=(-3, 4, 3), func=(0.6, 0.05, 0.0)))
    return cam, objs, 4, lights, 2, h.make_globals(kt=0.8)


def menger_scene(W, H):
    cam = h.make_camera((2.6, 2.2, 3.0), (-2.6, -2.2, -3.0), (0, 1, 0), 30.0, W, H)
    objs = (abi.RmObject * 1)(h.make_object(abi.RM_MENGERSPONGE, ambient=(.3, .3, .3), diffuse=(1, 1, 1),
                                            specular=(1, 1, 1), shininess=25.0, reflective=(.4, .4, .4)))
    lights = (abi.RmLight * 2)(h.make_light(abi.RM_LIGHT_DIRECTIONAL, (1, 1, 1), (-1, -1.5, -0.7)),
                               h.make_light(abi.RM_LIGHT_DIRECTIONAL, (.5, .5, .6), (1, -0.5, 0.3)))
    return cam, objs, 1, lights, 2, h.make_globals()


def directional_light_2(W, H):
    """lighting/directional_light_2.json through the library's loader, as the scene tuple the tests pass around."""
    from raymarcher_amd import Scene
    t = Scene(path=os.path.join(SCENES, "lighting", "directional_light_2.json")).tables(W, H)
    return t.camera, t.objects, t.num_objects, t.lights, t.num_lights, t.globals_


def moved_bulb_scene(W, H):
    """helpers.scene_mandelbulb with the bulb translated and rotated: the general Mandelbulb class."""
    scene = h.scene_mandelbulb(W, H)
    model = h.translate(0.15, -0.1, 0.2) @ h.rotation((0.3, 1.0, -0.2), 0.7)
    objs = (abi.RmObject * 1)(h.make_object(abi.RM_MANDELBULB, model=model))
    return (scene[0], objs, 1) + tuple(scene[3:])


# directional light directions: the c3 frame's three, then ones that light the bulb from the sides and from behind the camera
BULB_LIGHT_DIRS = [(0, 0, 1), (0, -1, 0), (0, 0, -1), (1, -0.3, -0.2), (-0.7, 0.2, -0.6), (0.2, 0.9, -0.1), (-0.3, -0.4, 0.8),
                   (0.6, 0.5, 0.6), (-1, -1, -1), (0.1, -0.2, -1)]
BULB_LIGHT_COLORS = [(1, 1, 1), (1.5, 1.1, 0.7), (1, 1, 1), (0.4, 0.6, 0.9), (0.9, 0.3, 0.3)]


def bulb_scene(W, H, nl=3, model=None, sf=1.0, julia=(0, 0), pos=(0, 0, 4.5), look=(0, 0, -1), up=(0, 1, 0), near=0.1, far=100.0,
               lights=None, refl=(0, 0, 0)):
    """helpers.scene_mandelbulb's bulb and material under any model, camera and Julia seed, lit by the first nl directional lights
    of BULB_LIGHT_DIRS (nl = 3: scene_mandelbulb's own three) or by `lights`, a list of RmLight."""
    cam = h.make_camera(pos, look, up, 30.0, W, H, near=near, far=far)
    objs = (abi.RmObject * 1)(h.make_object(abi.RM_MANDELBULB, model=model, scale_factor=sf, ambient=(.3, .3, .3),
                                            diffuse=(1, 1, 1), specular=(1, 1, 1), shininess=100.0, ior=1.5, reflective=refl))
    if lights is None:
        lights = [h.make_light(abi.RM_LIGHT_DIRECTIONAL, BULB_LIGHT_COLORS[i % 5], BULB_LIGHT_DIRS[i]) for i in range(nl)]
    arr = (abi.RmLight * len(lights))(*lights)
    return cam, objs, 1, arr, len(lights), h.make_globals(julia=julia)


def synthetic_textures():
    """Two procedural RGBA8 textures (rows bottom-up): a 37×23 colour gradient with a grid and a 64×64 checker."""
    rng = np.random.default_rng(11)
    yy, xx = np.mgrid[0:23, 0:37]
    a = np.stack([xx * 255 // 36, yy * 255 // 22, (xx * 7 + yy * 13) % 256, np.full_like(xx, 255)], -1).astype(np.uint8)
    a[::4, :, :3] //= 2
    yy, xx = np.mgrid[0:64, 0:64]
    b = np.where(((xx // 8 + yy // 8) % 2)[..., None] == 0, np.array([230, 40, 40, 255]), np.array([30, 60, 220, 255])).astype(np.uint8)
    b[..., :3] = np.clip(b[..., :3].astype(int) + rng.integers(-20, 20, (64, 64, 3)), 0, 255).astype(np.uint8)
    return [np.ascontiguousarray(a), np.ascontiguousarray(b)]


def textured_scene(W, H):
    """scenefiles/textures_tests in one frame: textured cube (floor), sphere, cone and cylinder + an untextured torus."""
    cam = h.make_camera((0.4, 2.2, 5.5), (-0.05, -0.35, -1), (0, 1, 0), 42.0, W, H)
    def tex(o, loc, ru, rv, blend):
        o.texLoc, o.repeatU, o.repeatV, o.blend = loc, ru, rv, blend
        return o
    objs = (abi.RmObject * 5)(
        tex(h.make_object(abi.RM_CUBE, model=h.translate(0, -0.8, 0) @ h.scale(7, 0.5, 7), scale_factor=0.5, ambient=(.2, .2, .2),
                          diffuse=(.9, .9, .9), specular=(.4, .4, .4), shininess=8), 1, 6.0, 6.0, 0.8),
        tex(h.make_object(abi.RM_SPHERE, model=h.translate(-1.5, 0.3, 0) @ h.scale(1.6, 1.6, 1.6), scale_factor=1.6,
                          ambient=(.1, .1, .1), diffuse=(1, 1, 1), specular=(1, 1, 1), shininess=30), 0, 2.0, 1.0, 1.0),
        tex(h.make_object(abi.RM_CONE, model=h.translate(0.3, 0.2, 0.8) @ h.scale(1.2, 1.5, 1.2), scale_factor=1.2,
                          ambient=(.1, .1, .1), diffuse=(.7, .9, .7), specular=(.5, .5, .5), shininess=12), 0, 3.0, 2.0, 0.5),
        tex(h.make_object(abi.RM_CYLINDER, model=h.translate(1.9, 0.2, -0.4) @ h.scale(1.1, 1.5, 1.1), scale_factor=1.1,
                          ambient=(.1, .1, .1), diffuse=(.9, .8, .6), specular=(.5, .5, .5), shininess=12), 1, 2.0, 1.0, 0.9),
        h.make_object(abi.RM_TORUS, model=h.translate(0, 1.6, -1.5) @ h.scale(2, 2, 2), scale_factor=2.0, ambient=(.1, .1, .2),
                      diffuse=(.3, .4, .9), specular=(1, 1, 1), shininess=20))
    lights = (abi.RmLight * 2)(h.make_light(abi.RM_LIGHT_DIRECTIONAL, (1, 1, 1), (-0.4, -1, -0.5)),
                               h.make_light(abi.RM_LIGHT_POINT, (.9, .8, .7), pos=(3, 4, 4), func=(0.7, 0.04, 0.0)))
    return cam, objs, 5, lights, 2, h.make_globals()


POST_CASES = {
    "gamma": dict(enableGammaCorrection=1),
    "hdr": dict(enableHDR=1, exposure=1.7),
    "bloom": dict(enableBloom=1, exposure=1.0),
    "bloom_hdr_fxaa": dict(enableBloom=1, enableHDR=1, enableFXAA=1, exposure=0.8),
    "fxaa_only": dict(enableFXAA=1),
    "gamma_fxaa": dict(enableGammaCorrection=1, enableFXAA=1),
    "none": dict(),
}


def synthetic_noise():
    """256×256 RGBA8 with DIFFERENT channels (the reference's noise_texture_1.png is grey; distinct channels also
    exercise noiseV's .yx swizzle).  A few texels are pushed to 255 so that stars (noise > 0.99) exist."""
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, (256, 256, 4), dtype=np.uint8)
    a[rng.integers(0, 256, 900), rng.integers(0, 256, 900), :2] = 255
    a[..., 3] = 255
    return np.ascontiguousarray(a)


def synthetic_skybox(n=24):
    """Six n×n RGBA8 faces, each a different two-colour gradient with a bright spot (bloom source)."""
    yy, xx = np.mgrid[0:n, 0:n]
    faces = []
    for f in range(6):
        c0 = np.array([(f * 40) % 256, (255 - f * 30) % 256, (f * 90 + 30) % 256])
        c1 = np.array([(200 + f * 10) % 256, (f * 50) % 256, (120 + f * 20) % 256])
        t = ((xx + (f + 1) * yy) / ((f + 2) * (n - 1.0)))[..., None]
        img = c0 * (1 - t) + c1 * t
        img[(xx - n // 3) ** 2 + (yy - n // 2) ** 2 < 6] = 255
        faces.append(np.ascontiguousarray(np.concatenate([img, np.full((n, n, 1), 255)], -1).astype(np.uint8)))
    return faces


def synthetic_ltc():
    """Smooth stand-ins for the LTC tables (float, 64×64×4; u = column): t1 ≈ the inverse-matrix parameters,
    t2 = (fresnel scale, fresnel bias, unused, horizon-clipping form factor)."""
    v, u = np.mgrid[0:64, 0:64] / 63.0
    t1 = np.stack([0.55 + 0.45 * v, 0.25 * u * v, 0.15 * (1 - v), 0.5 + 0.5 * np.sqrt(v)], -1)
    t2 = np.stack([0.9 - 0.5 * v, 0.1 + 0.3 * u, 0 * u, np.clip(0.35 + 0.65 * u + 0.1 * v, 0, 1.2)], -1)
    return t1.astype(np.float32), t2.astype(np.float32)


def night_scene(W, H):
    cam = h.make_camera((1.6, 0.4, -5), (-0.42, 0.36, 1), (0, 1, 0), 60.0, W, H)  # looks toward MOON (frag:107)
    objs = (abi.RmObject * 2)(
        h.make_object(abi.RM_SPHERE, model=h.translate(-0.9, 0, 0) @ h.scale(1.5, 1.5, 1.5), scale_factor=1.5, ambient=(.1, .1, .15),
                      diffuse=(.5, .5, .7), specular=(1, 1, 1), shininess=25, reflective=(.9, .9, .9)),
        h.make_object(abi.RM_CUBE, model=h.translate(1.3, -0.2, 0.4) @ h.scale(1.1, 1.1, 1.1), scale_factor=1.1, ambient=(.1, .1, .1),
                      diffuse=(.7, .4, .3), specular=(.5, .5, .5), shininess=10))
    lights = (abi.RmLight * 1)(h.make_light(abi.RM_LIGHT_DIRECTIONAL, (.9, .9, 1), (0.4, -0.4, -0.3)))
    return cam, objs, 2, lights, 1, h.make_globals(itime=1.3)


def sea_scene(W, H):
    cam = h.make_camera((0, 3.5, 6), (0, -0.35, -1), (0, 1, 0), 50.0, W, H, far=100.0)
    objs = (abi.RmObject * 1)(
        h.make_object(abi.RM_SPHERE, model=h.translate(0, 1.8, -1.5) @ h.scale(2, 2, 2), scale_factor=2.0, ambient=(.2, .2, .2),
                      diffuse=(.8, .3, .2), specular=(1, 1, 1), shininess=20, reflective=(.6, .6, .6)))
    lights = (abi.RmLight * 1)(h.make_light(abi.RM_LIGHT_DIRECTIONAL, (1, 1, 1), (-0.4, -1, -0.3)))
    return cam, objs, 1, lights, 1, h.make_globals(itime=0.7)


def area_light_scene(W, H):
    """A floor, a sphere and a torus under one rectangular area light with its emissive rectangle
    (RayMarchScene::initScene appends one per area light, raymarchscene.cpp:121-133) plus a point light."""
    cam = h.make_camera((0, 1.6, 5.5), (0, -0.2, -1), (0, 1, 0), 45.0, W, H)
    ctm = h.translate(0.3, 2.2, -1.0) @ rot_x(np.deg2rad(65.0)) @ h.scale(2.4, 1.4, 1.0)
    rect = h.make_object(abi.RM_RECTANGLE, model=ctm, scale_factor=1.0)
    rect.isEmissive, rect.lightIdx = 1, 0
    rect.color[0], rect.color[1], rect.color[2] = 1.0, 0.9, 0.6
    objs = (abi.RmObject * 4)(
        h.make_object(abi.RM_CUBE, model=h.translate(0, -1.0, 0) @ h.scale(9, 0.4, 9), scale_factor=0.4, ambient=(.1, .1, .1),
                      diffuse=(.7, .7, .7), specular=(.6, .6, .6), shininess=12, reflective=(.25, .25, .25)),
        h.make_object(abi.RM_SPHERE, model=h.translate(-1.2, 0, 0.2) @ h.scale(1.5, 1.5, 1.5), scale_factor=1.5, ambient=(.1, .1, .1),
                      diffuse=(.3, .5, .9), specular=(1, 1, 1), shininess=40),
        h.make_object(abi.RM_TORUS, model=h.translate(1.4, -0.2, 0) @ h.scale(1.8, 1.8, 1.8), scale_factor=1.8, ambient=(.1, .1, .1),
                      diffuse=(.9, .5, .2), specular=(.8, .8, .8), shininess=20),
        rect)
    area = h.make_light(abi.RM_LIGHT_AREA, (1.0, 0.9, 0.6), func=(1, 0, 0))
    area.intensity, area.twoSided = 0.0, 1  # sceneparser.cpp:18-30 drops the parsed intensity; twoSided is always set
    corners = [(-0.5, 0.5, 0), (0.5, 0.5, 0), (0.5, -0.5, 0), (-0.5, -0.5, 0)]  # realtime.h:136-141
    for k, c in enumerate(corners):
        w = ctm @ np.array([*c, 1.0])
        for j in range(3):
            area.points[k][j] = float(np.float32(w[j]))
    lights = (abi.RmLight * 2)(area, h.make_light(abi.RM_LIGHT_POINT, (.5, .5, .6), pos=(-3, 3, 3), func=(0.8, 0.05, 0)))
    return cam, objs, 4, lights, 2, h.make_globals()


def resource_case(name, W, H):
    """name → (scene, settings, resources dict) of the sampler-driven cases."""
    WB = abi.RM_FEAT_WHITE_BACKGROUND
    if name == "night_sky":
        return night_scene(W, H), abi.default_settings(features=abi.RM_FEAT_NIGHTSKY_BACKGROUND, enableReflection=1), {"noise": synthetic_noise()}
    if name == "sea_sky":
        return sea_scene(W, H), abi.default_settings(features=abi.RM_FEAT_SEA | abi.RM_FEAT_SKY_BACKGROUND, enableReflection=1), \
            {"noise": synthetic_noise()}
    if name == "sea_terrain_cloud":
        sc = sea_scene(W, H)
        sc = (h.make_camera((0, 700, 6), (0, -0.2, -1), (0, 1, 0), 50.0, W, H),) + sc[1:]
        return sc, abi.default_settings(features=ENV_ALL | abi.RM_FEAT_SEA), {"noise": synthetic_noise()}
    if name == "sea_terrain":
        sc = sea_scene(W, H)
        sc = (h.make_camera((0, 700, 6), (0, -0.2, -1), (0, 1, 0), 50.0, W, H, far=2000.0),) + sc[1:]
        return sc, abi.default_settings(features=abi.RM_FEAT_SKY_BACKGROUND | abi.RM_FEAT_TERRAIN | abi.RM_FEAT_SEA), {"noise": synthetic_noise()}
    if name == "skybox_reflect":
        return reflect_refract_scene(W, H), abi.default_settings(features=WB, enableSkyBox=1, enableReflection=1, enableRefraction=1), \
            {"skybox": synthetic_skybox()}
    if name == "area_light":
        t1, t2 = synthetic_ltc()
        return area_light_scene(W, H), abi.default_settings(features=WB, enableReflection=1), \
            {"ltc1": h.oracle_ltc_quantise(t1), "ltc2": h.oracle_ltc_quantise(t2)}
    if name == "area_light_soft_bump":
        t1, t2 = synthetic_ltc()
        return area_light_scene(W, H), abi.default_settings(enableSoftShadow=1, enableAmbientOcclusion=1), \
            {"ltc1": h.oracle_ltc_quantise(t1), "ltc2": h.oracle_ltc_quantise(t2)}
    if name == "area_light_bump_ao":
        t1, t2 = synthetic_ltc()
        return area_light_scene(W, H), abi.default_settings(enableAmbientOcclusion=1), \
            {"ltc1": h.oracle_ltc_quantise(t1), "ltc2": h.oracle_ltc_quantise(t2)}
    raise KeyError(name)


RESOURCE_CASES = ["night_sky", "sea_sky", "sea_terrain", "sea_terrain_cloud", "skybox_reflect", "area_light", "area_light_soft_bump",
                  "area_light_bump_ao"]


def random_primitive_case(rng, W, H):
    """A random all-primitive table (the class of the table walk's pass-over test AND of the march loops' single-object fast
    path), one to eight objects, sometimes over a floor slab, two to ten lights of the three plain kinds, every shading option."""
    f = rng.uniform
    types = [abi.RM_CUBE, abi.RM_CONE, abi.RM_CYLINDER, abi.RM_SPHERE, abi.RM_OCTAHEDRON, abi.RM_TORUS, abi.RM_CAPSULE,
             abi.RM_DEATHSTAR, abi.RM_RECTANGLE]
    objs = []
    for _ in range(int(rng.integers(1, 9))):
        ty = int(rng.choice(types))
        sc = float(f(0.6, 1.8))
        sx, sy, sz = (sc * float(f(0.8, 1.25)) for _ in range(3))
        M = h.translate(f(-2.2, 2.2), f(-1.0, 1.2), f(-2.5, 1.0)) @ rot_x(f(-0.6, 0.6)) @ h.scale(sx, sy, sz)
        objs.append(h.make_object(ty, model=M, scale_factor=min(sx, sy, sz), ambient=tuple(f(0, .3, 3)), diffuse=tuple(f(.2, 1, 3)),
                                  specular=tuple(f(0, 1, 3)), shininess=float(rng.choice([0, 1, 7.5, 25, 100])),
                                  reflective=tuple(f(0, .8, 3)) if f() < 0.4 else (0, 0, 0),
                                  transparent=tuple(f(0, .8, 3)) if f() < 0.3 else (0, 0, 0), ior=float(f(1.05, 1.6))))
    if f() < 0.5:  # a floor: long grazing shadow rays
        objs.append(h.make_object(abi.RM_CUBE, model=h.translate(0, -1.6, -1) @ h.scale(9, 0.2, 9), scale_factor=0.2,
                                  diffuse=(.7, .7, .7), ambient=(.1, .1, .1)))
    lights = []
    for _ in range(int(rng.choice([2, 2, 3, 3, 3, 4, 5, 6, 7, 10]))):
        kind = int(rng.integers(0, 3))
        col = tuple(f(.2, 1.2, 3))
        if kind == abi.RM_LIGHT_DIRECTIONAL:
            lights.append(h.make_light(kind, col, direction=(f(-1, 1), f(-1, 0.6), f(-1, 1))))
        elif kind == abi.RM_LIGHT_POINT:
            lights.append(h.make_light(kind, col, pos=(f(-4, 4), f(-1, 5), f(-3, 5)), func=(f(.5, 1), f(0, .1), f(0, .02))))
        else:
            lights.append(h.make_light(kind, col, direction=(f(-.3, .3), -1, f(-.6, 0)), pos=(f(-2, 2), f(3, 5), f(0, 3)),
                                       func=(f(.5, 1), f(0, .1), 0), angle=float(f(.4, .9)), penumbra=float(f(.05, .3))))
    feats = int(rng.choice([abi.RM_FEAT_WHITE_BACKGROUND, abi.RM_FEAT_DARK_BACKGROUND, 0]))
    if f() < 0.5:
        feats |= abi.RM_FEAT_PERLIN_BUMP
    s = abi.default_settings(features=feats, enableSoftShadow=int(f() < 0.5), enableAmbientOcclusion=int(f() < 0.4),
                             enableReflection=int(f() < 0.4), enableRefraction=int(f() < 0.3),
                             maxSteps=int(rng.choice([16, 64, 256])), numReflection=int(rng.choice([1, 2, 3])))
    g = h.make_globals(ka=f(.2, .8), kd=f(.3, 1), ks=f(.2, 1), kt=f(.2, 1))
    cam = h.make_camera((f(-1, 1), f(0.5, 2.5), f(4.5, 6.5)), (f(-.15, .15), f(-.45, -.05), -1), (0, 1, 0), float(f(35, 60)), W, H)
    return (cam, (abi.RmObject * len(objs))(*objs), len(objs), (abi.RmLight * len(lights))(*lights), len(lights), g), s


def random_tablewalk_case(rng, W, H):
    """A WIDE random all-primitive scene (helpers.random_tablewalk_objects: arbitrary-axis rotations, shear, anisotropy 0.2–5,
    scaleFactors that are not the smallest scale, nested and coincident objects, tables of up to 30), sometimes over a floor slab
    or inside an enclosing box, one to ten lights of the three plain kinds, every shading option, cameras outside, inside an
    object, or on an object's surface."""
    f = rng.uniform
    objs = h.random_tablewalk_objects(rng, max_objects=28)
    if f() < 0.4:  # a floor: long grazing shadow rays
        objs.append(h.make_object(abi.RM_CUBE, model=h.translate(0, -1.8, -1) @ h.scale(11, 0.2, 11), scale_factor=0.2,
                                  diffuse=(.7, .7, .7), ambient=(.1, .1, .1), reflective=(.3, .3, .3) if f() < 0.3 else (0, 0, 0)))
    if f() < 0.15:  # everything (camera too) inside one big cube: every ray hits, negative distances never occur but no ray leaves
        objs.append(h.make_object(abi.RM_CUBE, model=h.scale(24, 24, 24), scale_factor=24, diffuse=(.4, .5, .4), ambient=(.1, .1, .1)))
    lights = []
    for _ in range(int(rng.choice([1, 2, 2, 3, 3, 3, 4, 5, 7, 10]))):
        kind = int(rng.integers(0, 3))
        col = tuple(f(.2, 1.2, 3))
        if kind == abi.RM_LIGHT_DIRECTIONAL:
            lights.append(h.make_light(kind, col, direction=(f(-1, 1), f(-1, 0.6), f(-1, 1))))
        elif kind == abi.RM_LIGHT_POINT:
            lights.append(h.make_light(kind, col, pos=(f(-4, 4), f(-1, 5), f(-3, 5)), func=(f(.5, 1), f(0, .1), f(0, .02))))
        else:
            lights.append(h.make_light(kind, col, direction=(f(-.3, .3), -1, f(-.6, 0)), pos=(f(-2, 2), f(3, 5), f(0, 3)),
                                       func=(f(.5, 1), f(0, .1), 0), angle=float(f(.4, .9)), penumbra=float(f(.05, .3))))
    feats = int(rng.choice([abi.RM_FEAT_WHITE_BACKGROUND, abi.RM_FEAT_DARK_BACKGROUND, 0]))
    if f() < 0.5:
        feats |= abi.RM_FEAT_PERLIN_BUMP
    s = abi.default_settings(features=feats, enableSoftShadow=int(f() < 0.5), enableAmbientOcclusion=int(f() < 0.4),
                             enableReflection=int(f() < 0.4), enableRefraction=int(f() < 0.3),
                             maxSteps=int(rng.choice([16, 64, 256, 256])), numReflection=int(rng.choice([1, 2, 3])))
    g = h.make_globals(ka=f(.2, .8), kd=f(.3, 1), ks=f(.2, 1), kt=f(.2, 1))
    where = f()
    if where < 0.2:  # the camera inside an object (its near plane, where rays start, may still be outside a small one)
        o = objs[int(rng.integers(0, len(objs)))]
        M = np.linalg.inv(np.array(list(o.invModel), dtype=np.float64).reshape(4, 4).T)
        pos = tuple((M @ np.array([*f(-0.15, 0.15, 3), 1.0]))[:3])
        look = tuple(f(-1, 1, 3) + np.array([0, 0, -0.3]))
    elif where < 0.3:  # on (about) the bounding ball of an object, looking along it
        o = objs[int(rng.integers(0, len(objs)))]
        M = np.linalg.inv(np.array(list(o.invModel), dtype=np.float64).reshape(4, 4).T)
        d = rng.normal(size=3)
        pos = tuple((M @ np.array([*(d / np.linalg.norm(d) * 0.6), 1.0]))[:3])
        look = tuple(np.cross(d, rng.normal(size=3)))
    else:
        pos, look = (f(-1, 1), f(0.5, 2.5), f(4.5, 6.5)), (f(-.15, .15), f(-.45, -.05), -1)
    if np.linalg.norm(look) < 1e-3 or abs(np.dot(look, (0, 1, 0))) > 0.98 * np.linalg.norm(look):
        look = (0.1, -0.2, -1)
    cam = h.make_camera(pos, look, (0, 1, 0), float(f(35, 70)), W, H)
    return (cam, (abi.RmObject * len(objs))(*objs), len(objs), (abi.RmLight * len(lights))(*lights), len(lights), g), s


def random_bulb_case(rng, W, H):
    """A random scene of the single-Mandelbulb class (its own kernel instantiation: bounding-ball culls of two radii,
    v_min orbit trap, per-lane shadow-ray queue): model transform incl. anisotropic scales and tiny objects, Julia seeds
    inside and outside the tight ball's bound, powers, 1–5 lights of any kind (all-directional sets take the queue), every
    option, camera anywhere around — also inside the ball."""
    f = rng.uniform
    sc = float(rng.choice([1.0, 1.0, 1.7, 0.4, 0.04, 0.008]))
    an = (1.0, 1.0, 1.0) if f() < 0.7 else tuple(f(0.6, 2.5, 3))
    M = h.translate(*(f(-0.4, 0.4, 3) * sc)) @ rot_x(f(-1.0, 1.0)) @ h.scale(sc * an[0], sc * an[1], sc * an[2])
    o = h.make_object(abi.RM_MANDELBULB, model=M, scale_factor=sc * min(an), ambient=tuple(f(0, .4, 3)), diffuse=tuple(f(.2, 1, 3)),
                      specular=tuple(f(0, 1, 3)), shininess=float(rng.choice([0, 7.5, 25, 100])),
                      reflective=tuple(f(0, .8, 3)) if f() < 0.3 else (0, 0, 0),
                      transparent=tuple(f(0, .8, 3)) if f() < 0.2 else (0, 0, 0), ior=float(f(1.05, 1.6)))
    lights = []
    all_dir = f() < 0.6
    for _ in range(int(rng.integers(1, 6))):
        kind = abi.RM_LIGHT_DIRECTIONAL if all_dir else int(rng.integers(0, 3))
        col = tuple(f(.3, 1.6, 3))
        if kind == abi.RM_LIGHT_DIRECTIONAL:
            d = f(-1, 1, 3)
            lights.append(h.make_light(kind, col, direction=tuple(d if np.abs(d).max() > 0.1 else (0, -1, 0))))
        elif kind == abi.RM_LIGHT_POINT:
            lights.append(h.make_light(kind, col, pos=tuple(f(-4, 4, 3) * max(sc, 0.2)), func=(f(.5, 1), f(0, .1), f(0, .02))))
        else:
            lights.append(h.make_light(kind, col, direction=(f(-.3, .3), -1, f(-.6, 0)), pos=(f(-2, 2) * sc, f(3, 5) * sc, f(0, 3) * sc),
                                       func=(f(.5, 1), f(0, .1), 0), angle=float(f(.4, .9)), penumbra=float(f(.05, .3))))
    feats = int(rng.choice([abi.RM_FEAT_WHITE_BACKGROUND, abi.RM_FEAT_DARK_BACKGROUND, 0])) | (abi.RM_FEAT_PERLIN_BUMP if f() < 0.6 else 0)
    if f() < 0.2:
        feats |= abi.RM_FEAT_BULB_POWER8_ALGEBRAIC
    s = abi.default_settings(features=feats, enableSoftShadow=int(f() < 0.25), enableAmbientOcclusion=int(f() < 0.3),
                             enableReflection=int(f() < 0.4), enableRefraction=int(f() < 0.3),
                             maxSteps=int(rng.choice([1, 17, 64, 256])), fractalIters=int(rng.choice([1, 4, 12, 20])),
                             numReflection=int(rng.choice([1, 2])))
    julia = (0, 0) if f() < 0.6 else (tuple(f(-.6, .6, 2)) if f() < 0.6 else tuple(f(-1.6, 1.6, 2)))
    g = h.make_globals(ka=f(.2, .8), kd=f(.3, 1), ks=f(.2, 1), kt=f(.2, 1), power=float(rng.choice([8.0, 8.0, 8.0, 6.0, 3.5])), julia=julia)
    dist = float(rng.choice([4.5, 3.0, 1.6, 0.8])) * sc * max(an)
    dirv = f(-1, 1, 3)
    dirv = dirv / (np.linalg.norm(dirv) + 1e-9)
    pos = tuple(dirv * dist)
    look = tuple(-dirv + f(-0.15, 0.15, 3))
    cam = h.make_camera(pos, look, (0.1, 1, 0.05), float(f(25, 70)), W, H, near=0.02 * dist, far=float(rng.choice([100.0, 100.0, 6.0 * dist])))
    return (cam, (abi.RmObject * 1)(o), 1, (abi.RmLight * len(lights))(*lights), len(lights), g), s
