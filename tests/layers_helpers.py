"""The specification of rm_shade_rays_layers and rm_trace_rays_layers for the tests: tests/layers_spec/rm_layers_spec.c, which
includes the oracle's source and calls its own render, envLayers, seaRender, terrainRender, seaMapHeight, getSeaNormal and
terrainNormal, built on demand and loaded with ctypes by helpers.load_spec.  Nothing under oracle/ is touched.  Also the layer cases
(scene_builders' env_scene and sea_scene) and feature masks that more than one layers test module uses."""
import ctypes as C
import functools

import numpy as np

import helpers as h
import scene_builders as SB
import trace_helpers as T
from raymarcher_amd import abi

PATH_SHADE_LAYERS, PATH_TRACE_LAYERS = 14, 15  # rm_debug_last_path() of a launch of rm_shade_rays_layers / rm_trace_rays_layers
HIT_SEA, HIT_TERRAIN = -3, -4
SIZES_WH = ((64, 36), (37, 23))
N = 4099
COUNTS = (1, 63, 64, 65, 257, N)

SKY, DARK = abi.RM_FEAT_SKY_BACKGROUND, abi.RM_FEAT_DARK_BACKGROUND
TERRAIN, CLOUD, SEA, BUMP = abi.RM_FEAT_TERRAIN, abi.RM_FEAT_CLOUD, abi.RM_FEAT_SEA, abi.RM_FEAT_PERLIN_BUMP
LAYER_BITS = TERRAIN | CLOUD | SEA


P = C.POINTER
SIGNATURES = {
    "rmo_spec_shade_layers": (C.c_int, [P(abi.RmObject), C.c_int, P(abi.RmLight), C.c_int, P(abi.RmGlobals), P(abi.RmSettings),
                                        P(abi.RmResources), P(C.c_float), C.c_int, C.c_float, C.c_int, P(C.c_float), P(C.c_float)]),
    "rmo_spec_trace_layers": (C.c_int, [P(abi.RmObject), C.c_int, P(abi.RmGlobals), P(abi.RmSettings), P(C.c_float), C.c_int, C.c_int,
                                        C.c_uint, P(C.c_float)]),
}


def spec():
    """ctypes handle of the spec library (helpers.load_spec: rebuilt when a source it is made of is newer)."""
    return h.load_spec("layers", SIGNATURES)


def spec_shade_layers(scene, s, rays, far, image_width, res=None, expect=0):
    """(colour, bright), float32 (n, 4) each, of `rays` (float32 (n, 8)) by the specification.  scene: the tests' tuple (camera,
    objects, count, lights, count, globals) — the camera is not read; res: a resources dict for helpers.host_resources."""
    rays = np.ascontiguousarray(rays, dtype=np.float32)
    col = np.full((len(rays), 4), np.nan, dtype=np.float32)
    br = np.full((len(rays), 4), np.nan, dtype=np.float32)
    r, _keep = h.host_resources(**(res or {}))
    _, objs, no, lights, nl, g = scene[:6]
    st = spec().rmo_spec_shade_layers(objs, no, lights, nl, C.byref(g), C.byref(s), C.byref(r), h.fptr(rays), len(rays), far, image_width,
                                      h.fptr(col), h.fptr(br))
    assert st == expect, f"spec status {st}"
    return col, br


def spec_trace_layers(objs, num_objects, g, s, rays, image_width, mode="closest", expect=0):
    """The RmRayHit rows of `rays` (float32 (n, 8)) by the specification → float32 (n, 8); word 7 holds the int32 object index."""
    rays = np.ascontiguousarray(rays, dtype=np.float32)
    hits = np.full_like(rays, np.nan)
    st = spec().rmo_spec_trace_layers(objs, num_objects, C.byref(g), C.byref(s), h.fptr(rays), len(rays), image_width, T.MODES[mode],
                                      h.fptr(hits))
    assert st == expect, f"spec status {st}"
    return hits


# ---------------------------------------------------------------- the cases
# name → (scene builder, settings overrides, resources): env_scene with reflection and refraction on, sea_scene with reflection on
CASES = {
    "env_sky_terrain": (SB.env_scene, {"features": SKY | TERRAIN, "enableReflection": 1, "enableRefraction": 1}, False),
    "env_cloud_dark": (SB.env_scene, {"features": CLOUD | DARK, "enableReflection": 1, "enableRefraction": 1}, False),
    "env_all": (SB.env_scene, {"features": SKY | TERRAIN | CLOUD | BUMP, "enableReflection": 1, "enableRefraction": 1}, False),
    "env_all_sea": (SB.env_scene, {"features": SKY | TERRAIN | CLOUD | BUMP | SEA, "enableReflection": 1, "enableRefraction": 1}, True),
    "sea_sky": (SB.sea_scene, {"features": SEA | SKY, "enableReflection": 1}, True),
    "sea_terrain": (SB.sea_scene, {"features": SKY | TERRAIN | SEA, "enableReflection": 1}, True),
}
NAMES = list(CASES)


@functools.lru_cache(maxsize=None)
def shared_noise():
    """scene_builders.synthetic_noise(), built once and handed out read-only: the cached cases share it, and tables_of copies it
    before the renderer uploads it."""
    a = SB.synthetic_noise()
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def case(name, W=64, H=36):
    """(scene, settings, resources dict) of a case; W, H only shape the camera."""
    build, over, noise = CASES[name]
    return build(W, H), abi.default_settings(**over), ({"noise": shared_noise()} if noise else {})


def without_layers(s):
    """A copy of the settings with the three layer bits cleared."""
    s = abi.RmSettings.from_buffer_copy(bytes(s))
    s.features &= ~LAYER_BITS
    return s


def with_features(s, features):
    s = abi.RmSettings.from_buffer_copy(bytes(s))
    s.features = features
    return s


@functools.lru_cache(maxsize=None)
def primary_rays(name, W, H):
    """The case's primary rays by the trace specification (read-only, shared): row-major, row 0 at the bottom."""
    rays = T.spec_primary_rays(case(name, W, H)[0][0], W, H)
    rays.setflags(write=False)
    return rays


def camera_position(name):
    """Where the case's camera stands, read back from its primary rays' common origin region."""
    return tuple(float(v) for v in primary_rays(name, 64, 36)[:, 0:3].astype(np.float64).mean(axis=0))


@functools.lru_cache(maxsize=None)
def seeded_rays(name, n=N):
    """n seeded rays (T.seeded_rays: every kind, invalid ones in every wave) placed around the case's camera position, with a
    radius that reaches the layers from there (read-only, shared)."""
    radius = 40.0 if CASES[name][0] is SB.env_scene else 4.0
    rays = T.seeded_rays(np.random.default_rng(4000 + NAMES.index(name)), n, camera_position(name), radius)
    rays.setflags(write=False)
    return rays


def terrain_height(x, z):
    """The oracle's terrain height at (x, z) (rmo_probe_env kind 2) → float32 (n,)."""
    x = np.asarray(x, dtype=np.float32)
    pts = np.ascontiguousarray(np.stack([x, np.zeros_like(x), np.asarray(z, dtype=np.float32)], axis=1))
    out = np.empty((len(pts), 4), dtype=np.float32)
    assert h.oracle().rmo_probe_env(2, C.c_float(0.0), h.fptr(pts), h.fptr(out), len(pts)) == 0
    return out[:, 0]


def sky_of(rays):
    """getSky(rd) of each ray: the specification's colour over an empty table with SKY alone."""
    objs, _ = h.table([])
    scene = (None, objs, 0, None, 0, h.make_globals())
    return spec_shade_layers(scene, abi.default_settings(features=SKY), rays, 100.0, 1)[0][:, 0:3]


tables_of, ids_of, bits, assert_bits = h.tables_of, T.ids_of, h.bits, h.assert_bit_equal


def assert_spec(got, want, what, id_word=None):
    """The GPU's words against the specification's: bit for bit, with the one allowance the numeric contract has (the
    bits of a NaN produced by arithmetic are not defined — the host's and the GPU's differ in sign): a float word that is NaN on
    both sides counts as equal.  id_word: the column that holds an int32 (RmRayHit.objectId), compared as bits only.  Measured:
    the only such words here are the colours of a handful of horizontal axis-aligned rays that start below the sea's surface."""
    got, want = np.asarray(got), np.asarray(want)
    bad = bits(got) != bits(want)
    both_nan = np.isnan(got) & np.isnan(want)
    if id_word is not None:
        both_nan[:, id_word] = False
    assert both_nan.sum() <= max(8, both_nan.size // 500), f"{what}: {both_nan.sum()} NaN words are too many to wave through"
    bad &= ~both_nan
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} words differ; first (ray, word) at {np.argwhere(bad)[:5].tolist()}"
