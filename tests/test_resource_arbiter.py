"""The paths that read RmResources — object textures through the uv maps and getDiffuse's blend, the sky box, LTC area lights, the
emissive rectangles and BrightColor — against the independent NumPy float64 arbiter (tests/arbiter_numpy.py, written from the shader
text and the GL 3.3 specification).

Every case checks two things:
  (a) the NumPy arbiter and the C arbiter (oracle/rm_oracle_f64.c) agree within 1e-6 on every pixel, except where a pixel lies at
      a jump (a uv seam, cap or face edge within TEX_A texels; a march within GEOM of its hit test; an N·L or LTC `behind` test
      within COS) or took the sphere's pole rule, which the C arbiter's binary64 `v == 1` never takes;
  (b) the binary32 oracle — the contract the HIP kernels reproduce bit for bit — is within the north star's 1e-3 of the NumPy
      arbiter on colour AND bright on every pixel, except pixels that lie at a jump (TEX_B texels, GEOM, COS, or |luminance − 1| <
      LUM for the bright attachment) or that are ill-conditioned: turning the primary ray by 1e-6 rad and the shading normals by
      2e-4 rad (getNormal's binary32 noise) moves the arbiter's own value by at least a tenth of the discrepancy (grazing hits,
      shadow rays that skim an edge, mirrors, minified photographs).
      Every exception must be explained; their count is bounded per case by what was measured (stated at each case).

The synthetic textures are random bytes: one texel read wrongly is an error of order 0.1, not the 1e-3 of a smooth photograph.
|uv|·size stays ≤ 512 texels: beyond that binary32 itself loses about 1e-4 of a texel weight (ulp(512) = 6e-5)."""
import os

import numpy as np
import pytest

import arbiter_numpy as an
import helpers as h
from raymarcher_amd import abi
from raymarcher_amd.render import Scene

GOLD = os.path.join(os.path.dirname(__file__), "golden")
TEX_A, TEX_B = 0.05, 0.01   # texels
GEOM = 1e-6                 # world units
COS = 1e-4
LUM = 1e-3
JITTER = (1e-6, 2e-4)   # radians: primary rays, shading normals (see arbiter_numpy.render_frame_table)


def explain(case, f64, info, sens, o32, b32, c64, max_exceptions, ratio=0.1):
    """Assertions (a) and (b) above; returns the number of explained exceptions of (b)."""
    tex, geom, cos, pole = info["tex"], info["geom"], info["cos"], info["pole"]
    assert np.isfinite(f64).all() and np.isfinite(o32).all() and np.isfinite(b32).all()
    dd = np.abs(c64 - f64).max(-1)
    jump_a = (tex < TEX_A) | (geom < GEOM) | (cos < COS) | (pole == 0)
    bad = (dd > 1e-6) & ~jump_a
    assert not bad.any(), (f"{case}: the C and NumPy arbiters differ by up to {dd[bad].max():.2e} on {bad.sum()} pixels no margin "
                           f"explains, the first at {tuple(np.argwhere(bad)[0])}")
    d = np.abs(o32 - f64).max(-1)
    db = np.abs(b32 - info["bright"]).max(-1)
    jump_b = (tex < TEX_B) | (geom < GEOM) | (cos < COS)
    exc = (d > 1e-3) | (db > 1e-3)
    ok = jump_b | (sens >= ratio * np.maximum(d, db)) | ((d <= 1e-3) & (info["lum"] < LUM))
    bad = exc & ~ok
    assert not bad.any(), (f"{case}: {bad.sum()} pixels beyond 1e-3 of the arbiter that no margin explains: "
                           + "; ".join(f"{tuple(p)} colour {d[tuple(p)]:.2e} bright {db[tuple(p)]:.2e} tex {tex[tuple(p)]:.2e}"
                                       for p in np.argwhere(bad)[:5]))
    assert exc.sum() <= max_exceptions, f"{case}: {exc.sum()} explained exceptions, more than the {max_exceptions} measured"
    return int(exc.sum())


def run(case, tables, settings, W, H, res, max_exceptions, ratio=0.1):
    f64, hit, info = an.render_frame_table(tables, settings, W, H, resources=res, diag=True)
    fj = an.render_frame_table(tables, settings, W, H, resources=res, jitter=JITTER)[0]
    sens = np.abs(fj - f64).max(-1)
    scene = (tables.camera, tables.objects, tables.num_objects, tables.lights, tables.num_lights, tables.globals_)
    kw = {k: v for k, v in res.items() if k != "textures"}
    o32, b32 = h.oracle_render(scene, settings, W, H, bright=True, textures=res.get("textures"), **kw)
    c64 = h.arbiter_render(scene, settings, W, H, textures=res.get("textures"), **kw)
    explain(case, f64, info, sens, o32, b32, c64, max_exceptions, ratio)
    return f64, hit, info


def resources_of(t):
    r = {}
    if t.textures:
        r["textures"] = t.textures
    if t.ltc1 is not None:
        r["ltc1"], r["ltc2"] = t.ltc1, t.ltc2
    if t.skybox:
        r["skybox"] = t.skybox
    return r


# ---------------------------------------------------------------------------------------------- scenefiles with their textures on
W, H = 96, 54
TEXTURED = [("textures_tests/" + n, 0) for n in ("directional_light_textured", "texture_cone", "texture_cone2", "texture_cube",
                                                    "texture_cube2", "texture_cyl", "texture_cyl2", "texture_cyl3", "texture_sphere",
                                                    "texture_sphere2")]
TEXTURED[0] = (TEXTURED[0][0], 2)
TEXTURED += [("textures_tests/texture_cube_sample", 6), ("simple/unit_sphere", 0), ("simple/recursive_sphere_2", 1),
             ("lighting/depth_of_field", 1), ("lighting/shadow_test", 2)]


@pytest.mark.parametrize("name,max_exc", TEXTURED, ids=[n for n, _ in TEXTURED])
def test_textured_scenefiles(name, max_exc):
    """Every textures_tests/*.json and the textured objects of unit_sphere (C1, 64 steps), recursive_sphere_2, depth_of_field and
    shadow_test, through the product's loader and image readers, soft shadows + AO on (C1: its BASELINE settings).  Measured: 0
    explained exceptions per frame but 1, 4, 1 in directional_light_textured, texture_cube_sample, shadow_test (silhouettes,
    shadow edges, minified photographs)."""
    t = Scene(path=os.path.join(GOLD, "scenes", name + ".json")).tables(W, H)
    assert any(t.objects[i].texLoc >= 0 for i in range(t.num_objects))
    s = abi.default_settings(maxSteps=64) if name == "simple/unit_sphere" else abi.default_settings(enableSoftShadow=1, enableAmbientOcclusion=1)
    run(name, t, s, W, H, resources_of(t), max_exc)


# ---------------------------------------------------------------------------------------------- adversarial synthetic textures
def random_image(rows, cols, seed):
    return np.ascontiguousarray(np.random.default_rng(seed).integers(0, 256, (rows, cols, 4), dtype=np.uint8))


def rot_y(a):
    M = np.eye(4)
    M[0, 0], M[0, 2], M[2, 0], M[2, 2] = np.cos(a), np.sin(a), -np.sin(a), np.cos(a)
    return M


def rot_x(a):
    M = np.eye(4)
    M[1, 1], M[1, 2], M[2, 1], M[2, 2] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a)
    return M


def textured_scene(W, H, rep, blend, cam_pos=(0.4, 1.9, 5.0), look_y=-0.35):
    """A cube, a cone, a cylinder and a sphere, each textured (slot = its index), each turned so that its object-space +x — the
    seam θ = 0 of the side maps, the cube's ±x/±z edges — faces the camera, which looks down on the caps' rims and the sphere's
    north pole.  A directional and a point light; a tilted second sphere shows its south pole too."""
    cam = h.make_camera(cam_pos, (0, look_y, -1), (0, 1, 0), 50.0, W, H)
    types = [abi.RM_CUBE, abi.RM_CONE, abi.RM_CYLINDER, abi.RM_SPHERE, abi.RM_SPHERE]
    places = [(-2.1, 0, -0.5), (-0.7, 0, 0), (0.7, 0, 0), (2.1, 0, -0.5), (0.0, 1.2, -1.6)]
    objs = (abi.RmObject * len(types))()
    for i, (ty, pl) in enumerate(zip(types, places)):
        M = h.translate(*pl) @ rot_y(np.deg2rad(-80.0 + 25 * i)) @ (rot_x(np.deg2rad(150.0)) if i == 4 else np.eye(4)) @ h.scale(1.2, 1.2, 1.2)
        o = h.make_object(ty, model=M, scale_factor=1.2, ambient=(.1, .1, .1), diffuse=(.6, .5, .4), specular=(.3, .3, .3), shininess=20)
        o.texLoc, o.repeatU, o.repeatV, o.blend = i, rep[0], rep[1], blend
        objs[i] = o
    lights = (abi.RmLight * 2)(h.make_light(abi.RM_LIGHT_DIRECTIONAL, (.9, .9, .9), (-0.3, -1.0, -0.6)),
                               h.make_light(abi.RM_LIGHT_POINT, (.6, .6, .7), pos=(1.5, 3, 4), func=(1, 0.05, 0)))
    from raymarcher_amd.render import SceneTables
    return SceneTables(cam, objs, len(types), lights, 2, h.make_globals())


SIZES = [(1, 1), (1, 5), (5, 1), (3, 7), (17, 9), (64, 64)]
SYNTH = [(sz, rep, blend) for sz, rep, blend in [
    ((1, 1), (1.0, 1.0), 1.0), ((1, 5), (2.5, 7.0), 0.5), ((5, 1), (7.0, -3.0), 1.0), ((3, 7), (-3.0, 2.5), 1.0),
    ((17, 9), (2.5, -3.0), 1.0), ((64, 64), (7.0, 7.0), 1.0), ((64, 64), (-3.0, 1.0), 0.5), ((17, 9), (1.0, 2.5), 0.0)]]
SW, SH = 80, 48


def synthetic_textured(sz, rep, blend, W=SW, H=SH):
    t = textured_scene(W, H, rep, blend)
    t.textures = [random_image(sz[0], sz[1], seed=17 * i + sz[0] * 131 + sz[1]) for i in range(5)]
    return t


@pytest.mark.parametrize("sz,rep,blend", SYNTH, ids=[f"{a}x{b}_rep{r[0]:g},{r[1]:g}_blend{bl:g}" for (a, b), r, bl in SYNTH])
def test_random_byte_textures(sz, rep, blend):
    """Random-byte RGBA textures of 1×1 … 64×64 on a cube, a cone, a cylinder and two spheres: repeatU/V in {1, 2.5, 7, −3} (−3
    maps uv to negative texel indices: the REPEAT wrap of i < 0), blend 0, 0.5 and 1, every seam, cap rim and pole in view.  Every
    pixel is within 1e-3 but those at a uv jump (measured: 0 per frame, 3 with 64×64 at repeat 7)."""
    assert max(abs(rep[0]) * sz[1], abs(rep[1]) * sz[0]) <= 512
    t = synthetic_textured(sz, rep, blend)
    s = abi.default_settings(enableSoftShadow=1)
    f64, hit, info = run(f"random {sz} {rep} {blend}", t, s, SW, SH, {"textures": t.textures}, 5)
    assert hit.mean() > 0.12 and np.isfinite(info["tex"]).sum() > 0.1 * SW * SH  # textured surfaces fill the frame
    if sz == (64, 64) and rep[0] == 7.0:
        assert (info["tex"] < 1.0).sum() >= 5   # the cameras do see seams / caps / edges
        assert (info["pole"] == 0).sum() >= 1   # and a pole


# ---------------------------------------------------------------------------------------------- the sky box
def random_faces(n, seed):
    return [random_image(n, n, seed * 10 + f) for f in range(6)]


def skybox_scene(W, H, cam_pos, look, fov):
    """Two mirrors (a sphere and a cube, reflective 0.8) in front of a camera whose wide view crosses the cube map's face edges and
    corners (|x| = |y| = |z|)."""
    cam = h.make_camera(cam_pos, look, (0, 1, 0), fov, W, H)
    objs = (abi.RmObject * 2)(
        h.make_object(abi.RM_SPHERE, model=h.translate(1.2, 0.9, 1.6) @ h.scale(1.0, 1.0, 1.0), scale_factor=1.0, ambient=(.05, .05, .05),
                      diffuse=(.2, .2, .2), specular=(.5, .5, .5), shininess=30, reflective=(.8, .8, .8)),
        h.make_object(abi.RM_CUBE, model=h.translate(2.2, 2.4, 1.2) @ rot_y(0.5) @ h.scale(0.8, 0.8, 0.8), scale_factor=0.8,
                      ambient=(.05, .05, .05), diffuse=(.2, .2, .2), reflective=(.8, .8, .8)))
    lights = (abi.RmLight * 1)(h.make_light(abi.RM_LIGHT_DIRECTIONAL, (1, 1, 1), (-0.2, -1.0, -0.4)))
    from raymarcher_amd.render import SceneTables
    return SceneTables(cam, objs, 2, lights, 1, h.make_globals())


SKY = [(1, (0, 0, 0), (1, 1, 1), 100.0), (5, (0, 0, 0), (1, 1, 1), 100.0), (24, (0, 0, 0), (1, 1, 1), 100.0),
       (24, (0, 0, 0), (-1, -0.2, -1), 110.0), (5, (0, 0, 0), (0.1, -1, 0.05), 120.0)]


@pytest.mark.parametrize("n,pos,look,fov", SKY, ids=[f"{n}px_look{look}" for n, _p, look, _f in SKY])
def test_sky_box(n, pos, look, fov):
    """Random-byte square faces of 1, 5 and 24 texels, wide cameras whose rays cross face edges and the corners |x| = |y| = |z|
    (seen directly and in the mirrors, one bounce; Perlin bump off, so that mirrors do not scatter the rays): face selection with the x-before-y-before-z tie rule, the (s, t) of table 3.19
    and CLAMP_TO_EDGE inside a face.  Measured: 0 exceptions but 5 on the 24-texel faces seen in the mirrors (ill-conditioned)."""
    W, H = 72, 54
    t = skybox_scene(W, H, pos, look, fov)
    t.skybox = random_faces(n, n)
    s = abi.default_settings(enableSkyBox=1, enableReflection=1, features=abi.RM_FEAT_WHITE_BACKGROUND)
    f64, hit, info = run(f"sky {n}", t, s, W, H, {"skybox": t.skybox}, 6)
    assert (~hit).mean() > 0.5 and (info["tex"] < 1.0).sum() >= 3  # mostly sky, and its face edges are in view


def test_beach_sky_box():
    """cubemap/beach.json with its own six faces, decoded by the product's JPEG reader as initCubeMap loads them: the sky box on
    the miss path.  (Its mirror spheres reflect a 1024-texel photograph through binary32 four-tap normals — ill-conditioned on
    ≈1 % of the pixels — so the bounces through the box are held by test_sky_box's random faces instead.)"""
    from raymarcher_amd import lib
    from raymarcher_amd.render import load_image
    z = np.load(os.path.join(GOLD, "glsl", "scenefile_sweep_beach.npz"))
    t = Scene(path=os.path.join(GOLD, "scenes", "cubemap", "beach.json")).tables(W, H)
    t.skybox = [load_image(os.path.join(GOLD, "scenes", lib().rm_skybox_face_path(int(z["cubemap"]), f).decode()), flip_vertical=True)
                for f in range(6)]
    s = abi.default_settings(enableSkyBox=1)
    run("beach", t, s, W, H, resources_of(t), 2)


# ---------------------------------------------------------------------------------------------- area lights
def fixture_ltc(name="frame_res_area_light.npz"):
    z = np.load(os.path.join(GOLD, "glsl", name))
    k1, k2 = ("res_ltc1", "res_ltc2") if "res_ltc1" in z.files else ("ltc1", "ltc2")
    return np.ascontiguousarray(z[k1]), np.ascontiguousarray(z[k2])


@pytest.mark.parametrize("name,max_exc", [("lighting/bloom", 0), ("lighting/arealight", 3), ("simple/unit_plane", 0)])
def test_area_light_scenefiles(name, max_exc):
    """bloom.json, arealight.json and unit_plane.json with the 8-bit LTC tables the reference uploads (fixtures).  Measured: bloom
    and unit_plane every pixel within 1e-3 (colour and bright); arealight 3 pixels on the rim of a mirror sphere, ill-conditioned."""
    t = Scene(path=os.path.join(GOLD, "scenes", name + ".json")).tables(W, H)
    t.ltc1, t.ltc2 = fixture_ltc(f"scenefile_sweep_{name.split('/')[1]}.npz")
    run(name, t, abi.default_settings(), W, H, resources_of(t), max_exc)


def area_scene(W, H, two_sided, cam_pos=(0, 1.6, 5.5), look=(0, -0.2, -1), tilt=65.0, point=True):
    """A floor, a sphere and a torus under a rectangular area light (its emissive rectangle is object 3, lightIdx 0) and, with
    point=True, a point light.  Parts of the floor and the torus lie behind the light's plane."""
    cam = h.make_camera(cam_pos, look, (0, 1, 0), 45.0, W, H)
    ctm = h.translate(0.3, 1.2, -1.0) @ rot_x(np.deg2rad(tilt)) @ h.scale(2.4, 1.4, 1.0)
    rect = h.make_object(abi.RM_RECTANGLE, model=ctm, scale_factor=1.0)
    rect.isEmissive, rect.lightIdx = 1, 0
    rect.color[0], rect.color[1], rect.color[2] = 1.0, 0.9, 0.6
    objs = (abi.RmObject * 4)(
        h.make_object(abi.RM_CUBE, model=h.translate(0, -1.0, 0) @ h.scale(9, 0.4, 9), scale_factor=0.4, ambient=(.1, .1, .1),
                      diffuse=(.7, .7, .7), specular=(.6, .6, .6), shininess=12, reflective=(.25, .25, .25)),
        h.make_object(abi.RM_SPHERE, model=h.translate(-1.2, 0, 0.2) @ h.scale(1.5, 1.5, 1.5), scale_factor=1.5, ambient=(.1, .1, .1),
                      diffuse=(.3, .5, .9), specular=(1, 1, 1), shininess=40),
        h.make_object(abi.RM_TORUS, model=h.translate(1.4, -0.2, -2.0) @ h.scale(1.8, 1.8, 1.8), scale_factor=1.8, ambient=(.1, .1, .1),
                      diffuse=(.9, .5, .2), specular=(.8, .8, .8), shininess=20),
        rect)
    area = h.make_light(abi.RM_LIGHT_AREA, (1.0, 0.9, 0.6), func=(1, 0, 0))
    area.intensity, area.twoSided = 0.7, int(two_sided)
    for k, c in enumerate([(-0.5, 0.5, 0), (0.5, 0.5, 0), (0.5, -0.5, 0), (-0.5, -0.5, 0)]):
        w = ctm @ np.array([*c, 1.0])
        for j in range(3):
            area.points[k][j] = float(np.float32(w[j]))
    lights = (abi.RmLight * 2)(area, h.make_light(abi.RM_LIGHT_POINT, (.5, .5, .6), pos=(-3, 3, 3), func=(0.8, 0.05, 0)))
    from raymarcher_amd.render import SceneTables
    return SceneTables(cam, objs, 4, lights, 2 if point else 1, h.make_globals())


AREA = [("two_sided", 1, {}, {}), ("one_sided", 0, {}, {}),
        ("one_sided_soft_ao", 0, {"enableSoftShadow": 1, "enableAmbientOcclusion": 1}, {}),
        ("two_sided_reflection", 1, {"enableReflection": 1}, {}),
        ("grazing", 1, {}, {"cam_pos": (0, -0.45, 6.0), "look": (0, -0.02, -1), "tilt": 90.0, "point": False}),
        ("grazing_one_sided", 0, {"enableAmbientOcclusion": 1}, {"cam_pos": (4.0, -0.5, 3.0), "look": (-1, 0.0, -0.8), "tilt": 88.0})]


@pytest.mark.parametrize("case,two_sided,over,geo", AREA, ids=[a[0] for a in AREA])
def test_synthetic_area_lights(case, two_sided, over, geo):
    """A rectangle light, one- and two-sided, shading points in front of and behind its plane, with a point light beside it, soft
    shadows and AO on and off, one reflection bounce (which sees the emissive rectangle: UB5), and grazing views where the specular
    transform degenerates (UB11).  The LTC tables are the reference's 8-bit texels (fixture).  Colour and bright.  Measured: 0
    exceptions per frame, 1 with the reflection bounce."""
    W, H = 80, 48
    t = area_scene(W, H, two_sided, **geo)
    t.ltc1, t.ltc2 = fixture_ltc()
    f64, hit, info = run(case, t, abi.default_settings(**over), W, H, resources_of(t), 3)
    assert np.isfinite(info["cos"]).sum() > 0.2 * W * H
