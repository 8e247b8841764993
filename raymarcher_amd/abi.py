"""ctypes mirror of include/raymarcher_amd.h (the C-ABI PODs and enums).

Field order and types must match the header byte for byte; tests/test_abi.py checks sizeof() of every
struct against the library's own `rm_abi_sizeof`.
"""
import ctypes as C

RM_ABI_VERSION = 5
RM_COUNT_REFERENCE, RM_COUNT_EXECUTED = 1, 2
RM_MAX_LIGHTS = 10
RM_MAX_OBJECTS = 30
RM_MAX_BATCH_FRAMES = 1024  # frames of one rm_render_batch call
RM_MAX_SUBFRAMES = 64  # sub-frames of one output frame of rm_render_accumulated

(RM_CUBE, RM_CONE, RM_CYLINDER, RM_SPHERE, RM_OCTAHEDRON, RM_TORUS, RM_CAPSULE, RM_DEATHSTAR, RM_RECTANGLE,
 RM_MANDELBROT, RM_MANDELBULB, RM_MENGERSPONGE, RM_SIERPINSKI, RM_CUSTOM) = range(14)
PRIMITIVE_NAMES = {
    "cube": RM_CUBE, "cone": RM_CONE, "cylinder": RM_CYLINDER, "sphere": RM_SPHERE, "octahedron": RM_OCTAHEDRON,
    "torus": RM_TORUS, "capsule": RM_CAPSULE, "deathstar": RM_DEATHSTAR, "rectangle": RM_RECTANGLE,
    "mandelbrot": RM_MANDELBROT, "mandelbulb": RM_MANDELBULB, "mengersponge": RM_MENGERSPONGE,
    "sierpinski": RM_SIERPINSKI, "custom": RM_CUSTOM,
}
RM_LIGHT_POINT, RM_LIGHT_DIRECTIONAL, RM_LIGHT_SPOT, RM_LIGHT_AREA = range(4)

RM_FEAT_SKY_BACKGROUND = 1 << 0
RM_FEAT_NIGHTSKY_BACKGROUND = 1 << 1
RM_FEAT_DARK_BACKGROUND = 1 << 2
RM_FEAT_WHITE_BACKGROUND = 1 << 3
RM_FEAT_CLOUD = 1 << 4
RM_FEAT_TERRAIN = 1 << 5
RM_FEAT_SEA = 1 << 6
RM_FEAT_PERLIN_BUMP = 1 << 7
RM_FEAT_BULB_POWER8_ALGEBRAIC = 1 << 8  # opt-in evaluation scheme, see include/raymarcher_amd.h
RM_FEAT_REFERENCE_DEFAULT = RM_FEAT_WHITE_BACKGROUND | RM_FEAT_PERLIN_BUMP

RM_OK, RM_ERR_INVALID_ARGUMENT, RM_ERR_CAPACITY, RM_ERR_UNSUPPORTED, RM_ERR_DEVICE, RM_ERR_IO, RM_ERR_PARSE = range(7)

(RM_FN_SIN, RM_FN_COS, RM_FN_ACOS, RM_FN_ATAN2, RM_FN_LOG2, RM_FN_EXP2, RM_FN_POW, RM_FN_SQRT, RM_FN_DIV,
 RM_FN_PNOISE3, RM_FN_ASIN, RM_FN_Q16, RM_FN_SQRT_FAST, RM_FN_DIVR, RM_FN_RCP, RM_FN_SMOOTHSTEP, RM_FN_MIN, RM_FN_MAX, RM_FN_FRACT,
 RM_FN_MEDIAN_ABS, RM_FN_COUNT) = range(21)

f32 = C.c_float
i32 = C.c_int32


class RmObject(C.Structure):
    _fields_ = [
        ("type", i32), ("invModel", f32 * 16), ("scaleFactor", f32), ("shininess", f32), ("blend", f32),
        ("ior", f32), ("cAmbient", f32 * 3), ("cDiffuse", f32 * 3), ("cSpecular", f32 * 3),
        ("cReflective", f32 * 3), ("cTransparent", f32 * 3), ("texLoc", i32), ("repeatU", f32),
        ("repeatV", f32), ("isEmissive", i32), ("color", f32 * 3), ("lightIdx", i32),
    ]


class RmLight(C.Structure):
    _fields_ = [
        ("type", i32), ("color", f32 * 3), ("dir", f32 * 3), ("pos", f32 * 3), ("func", f32 * 3),
        ("angle", f32), ("penumbra", f32), ("points", (f32 * 3) * 4), ("intensity", f32), ("twoSided", i32),
    ]


RM_MAX_TEXTURES = 10


class RmTexture(C.Structure):
    _fields_ = [("pixels", C.c_void_p), ("width", i32), ("height", i32)]


RM_LTC_SIZE = 64


class RmResources(C.Structure):
    _fields_ = [("textures", C.POINTER(RmTexture)), ("numTextures", i32), ("noise", RmTexture), ("skybox", RmTexture * 6),
                ("ltc1", C.c_void_p), ("ltc2", C.c_void_p)]


class RmCamera(C.Structure):
    _fields_ = [("invProjView", f32 * 16), ("initialFar", f32), ("eyePosition", f32 * 4)]


class RmGlobals(C.Structure):
    _fields_ = [("ka", f32), ("kd", f32), ("ks", f32), ("kt", f32), ("power", f32), ("juliaSeed", f32 * 2),
                ("iTime", f32), ("isTwoD", i32)]


class RmSettings(C.Structure):
    _fields_ = [("enableSoftShadow", i32), ("enableReflection", i32), ("enableRefraction", i32),
                ("enableAmbientOcclusion", i32), ("enableSkyBox", i32), ("maxSteps", i32), ("fractalIters", i32),
                ("mengerLevels", i32), ("numReflection", i32), ("features", C.c_uint32)]


class RmCounters(C.Structure):
    _fields_ = [("sceneEvals", C.c_uint64), ("bulbIters", C.c_uint64), ("hitPixels", C.c_uint64),
                ("shadedPoints", C.c_uint64), ("terrainEvals", C.c_uint64), ("cloudEvals", C.c_uint64), ("shapeEvals", C.c_uint64)]


class RmPostSettings(C.Structure):
    _fields_ = [("enableFXAA", i32), ("enableGammaCorrection", i32), ("enableHDR", i32), ("enableBloom", i32),
                ("exposure", f32)]


class RmHostSettings(C.Structure):
    _fields_ = [("screenWidth", i32), ("screenHeight", i32), ("nearPlane", f32), ("farPlane", f32),
                ("twoDSpace", i32), ("enableSoftShadow", i32), ("enableReflection", i32),
                ("enableRefraction", i32), ("enableAmbientOcculusion", i32), ("power", f32),
                ("juliaSeed", f32 * 2)]


class RmCameraData(C.Structure):
    _fields_ = [("pos", f32 * 4), ("look", f32 * 4), ("up", f32 * 4), ("heightAngle", f32)]


class RmRay(C.Structure):
    _fields_ = [("origin", f32 * 3), ("tMax", f32), ("dir", f32 * 3), ("reserved", i32)]


class RmRayHit(C.Structure):
    _fields_ = [("normal", f32 * 3), ("t", f32), ("position", f32 * 3), ("objectId", i32)]


RM_TRACE_CLOSEST, RM_TRACE_NO_NORMAL, RM_TRACE_OCCLUSION = 0, 1, 2  # mode of rm_trace_rays; NO_NORMAL is a flag on CLOSEST
RM_RAY_INVALID = -2  # RmRayHit.objectId of an invalid ray
RM_PATH_TRACE_RAYS, RM_PATH_SHADE_RAYS = 12, 13  # rm_debug_last_path() behind a launch of rm_trace_rays / rm_shade_rays
RM_HIT_SEA, RM_HIT_TERRAIN = -3, -4  # RmRayHit.objectId of rm_trace_rays_layers where the sea / the terrain is the visible surface
RM_PATH_SHADE_RAYS_LAYERS, RM_PATH_TRACE_RAYS_LAYERS = 14, 15  # … behind rm_shade_rays_layers / rm_trace_rays_layers
RM_PATH_SDF_GRID = 16  # … behind rm_sdf_grid
RM_MAX_LATTICE_DIM = 4096  # points per axis of a lattice of rm_sdf_grid / rm_sdf_mesh
RM_PATH_SDF_BLOCKS_SELECT, RM_PATH_SDF_GRID_BLOCKS = 18, 19  # … behind rm_sdf_blocks_select / rm_sdf_grid_blocks
RM_PATH_SDF_BLOCKS_SELECT_PRUNED = 20  # … behind rm_sdf_blocks_select_pruned
RM_MAX_LATTICE_BLOCKS = 512  # blocks of 8×8×8 cells per axis of a virtual lattice (rm_sdf_blocks_select and its two companions)
RM_MAX_BLOCK_LIST = 1 << 22  # entries of one block list
RM_RAYS_ORDER_TILE = 2048  # keys per workgroup of rm_rays_order's sort
RM_RAYS_MAX_ORIGIN_BITS, RM_RAYS_MAX_DIR_BITS = 10, 11  # the finest key of rm_rays_order


class RmSurfacePoint(C.Structure):
    _fields_ = [("normal", f32 * 3), ("distance", f32), ("position", f32 * 3), ("objectId", i32)]


class RmPointsSettings(C.Structure):
    _fields_ = [("far", f32), ("iso", f32), ("maxMove", f32), ("projectSteps", i32)]


class RmFieldSample(C.Structure):
    _fields_ = [("gradient", f32 * 3), ("value", f32), ("cell", i32 * 3), ("objectId", i32)]


RM_FIELD_OUTSIDE, RM_FIELD_UNLISTED = -5, -6  # RmFieldSample.objectId of a point outside the lattice's box / in an unlisted block
RM_MAX_FIELD_STEPS = 65536  # march steps of one rm_sdf_trace / rm_sdf_trace_blocks call
RM_FIELD_PENUMBRA_K = 8.0  # the k of the penumbra tracker of rm_field_trace's RM_TRACE_OCCLUSION


class RmAmbient(C.Structure):
    _fields_ = [("bent", f32 * 3), ("visibility", f32), ("normal", f32 * 3), ("hits", i32)]


RM_AMBIENT_SOFT, RM_AMBIENT_HARD = 0, 1  # mode of rm_field_ambient: the penumbra factor of every ray, or visible or not
RM_MAX_AMBIENT_DIRS = 256  # directions per point of one rm_field_ambient call, a power of two
RM_MAX_AMBIENT_TABLE = 1024  # numSets * numDirs of its table
class RmProbeDir(C.Structure):
    _fields_ = [("dir", f32 * 3), ("reserved", f32), ("basis", f32 * 9), ("pad", f32 * 3)]


class RmLightProbe(C.Structure):
    _fields_ = [("sh", (f32 * 4) * 9), ("hits", i32), ("reserved", i32 * 3)]


RM_MAX_PROBE_DIRS = 1024  # directions per probe of one rm_light_probes call, a power of two
RM_MAX_PROBE_TABLE = 4096  # numSets * numDirs of its table
RM_PATH_LIGHT_PROBES = 21  # rm_debug_last_path() behind a launch of rm_light_probes


class RmGridLight(C.Structure):
    _fields_ = [("e", f32 * 4), ("weight", f32), ("probes", i32), ("reserved", i32 * 2)]


RM_LIGHT_GRID_FACING = 1  # flag of rm_light_grid_irradiance: DDGI's backface term on every corner's weight
RM_MAX_LIGHT_GRID_DIM = 1024  # probes per axis of the grid of one rm_light_grid_irradiance call, at least 2
RM_MAX_LIGHT_GRID_PROBES = 1 << 24  # and probes of the whole grid


class RmProbeDepth(C.Structure):
    _fields_ = [("moments", (f32 * 2) * 64)]


RM_PROBE_DEPTH_TEXELS = 64  # texels of an RmProbeDepth, an 8×8 octahedral map: tx + 8·ty
RM_LIGHT_GRID_VIS_FLOOR = 1.0e-6  # the least visibility rm_light_grid_irradiance_visible gives a corner that does not see the point
RM_PATH_LIGHT_PROBES_DEPTH = 22  # rm_debug_last_path() behind a launch of rm_light_probes_depth


class RmLightGridRef(C.Structure):
    _fields_ = [("d_probes", C.c_void_p), ("d_depth", C.c_void_p), ("dims", i32 * 3), ("origin", f32 * 3), ("step", f32 * 3),
                ("strength", f32), ("flags", C.c_uint32), ("normalBias", f32)]


RM_INV_PI = 0.3183098733425140380859375  # float32(1/π): k = strength · RM_INV_PI of rm_shade_rays_indirect's term
RM_PATH_SHADE_RAYS_INDIRECT, RM_PATH_LIGHT_PROBES_INDIRECT = 23, 24  # rm_debug_last_path() behind rm_shade_rays_indirect / rm_light_probes_indirect
RM_PATH_SHADE_POINTS = 17  # rm_debug_last_path() behind a launch of rm_shade_points
RM_MAX_PROJECT_STEPS = 16  # projection steps of one rm_shade_points call


def default_settings(**over):
    """RmSettings with the reference's constants (frag:28,29,45,1056; frag:9,15)."""
    s = RmSettings(0, 0, 0, 0, 0, 256, 20, 4, 1, RM_FEAT_REFERENCE_DEFAULT)
    for k, v in over.items():
        setattr(s, k, v)
    return s
