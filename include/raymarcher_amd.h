/*
 * raymarcher_amd.h — C-ABI of the MI355X-native sphere-tracing renderer.
 *
 * This is the drop-in boundary for ONE path of KentaYoshii/Raymarcher: the per-pixel raymarch that
 * the reference runs as a GLSL fragment shader behind one draw call.  The reference has no FFI for
 * that path; its de-facto operator interface is the uniform block of resources/raymarch.frag:245-286
 * plus glDrawArrays in Realtime::rayMarch() (src/realtimerender.cpp:53-87).  Every entry point below
 * names the reference interface it replaces.  All paths are relative to the reference checkout.
 *
 * Conventions
 *  - plain C, no C++/torch types; all structs are PODs with 4-byte members only (no padding surprises);
 *  - matrices are column-major float[16] exactly as glm / glUniformMatrix4fv(…, GL_FALSE, …) hand them over;
 *  - output frames are row-major float RGBA, **row 0 = bottom of the image** (GL convention,
 *    frag:2572-2574); rm_frame_to_rgba8() applies the vertical flip of Realtime::saveViewportImage
 *    (src/realtime.cpp:337-338);
 *  - d_* pointers are DEVICE pointers owned by the caller (hipMalloc / torch tensor storage); render calls are
 *    asynchronous on the caller's stream and act on the calling thread's current device.  Library state is per device
 *    (a ring of 7 KB scene-table slots that grows instead of blocking, timing records) and, for scratch memory, per
 *    (device, stream): rm_post_process and the experimental Mandelbulb pipelines keep a grow-only workspace for each
 *    stream they are called on (≤ 20 B/pixel resp. ≤ 52 B/pixel + 8 B per pixel·light), (re)allocated — with a
 *    synchronise of that stream — only when a larger frame than any before is processed on it.  Calls on different
 *    streams or devices may be issued concurrently from different host threads; calls on ONE stream must come from one
 *    thread at a time (as with any HIP stream);
 *  - every function returns an rm_status; no exception crosses this boundary (the reference throws
 *    std::runtime_error on shader failure, src/utils/shaderloader.h:39,83, and prints + returns on
 *    scene errors, src/raymarch/raymarchscene.cpp:111).
 */
#ifndef RAYMARCHER_AMD_H
#define RAYMARCHER_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RM_ABI_VERSION 5

/* Capacity limits — src/realtime.h:17-27 (MAX_NUM_LIGHTS 10, MAX_NUM_SHAPES 30). */
#define RM_MAX_LIGHTS 10
#define RM_MAX_OBJECTS 30
/* Frames of one rm_render_batch call. */
#define RM_MAX_BATCH_FRAMES 1024
/* Sub-frames (lens samples, shutter times) of one output frame of rm_render_accumulated. */
#define RM_MAX_SUBFRAMES 64

/* Primitive type tags — src/utils/scenedata.h:18-33 == frag:53-68. */
enum {
  RM_CUBE = 0, RM_CONE = 1, RM_CYLINDER = 2, RM_SPHERE = 3, RM_OCTAHEDRON = 4, RM_TORUS = 5,
  RM_CAPSULE = 6, RM_DEATHSTAR = 7, RM_RECTANGLE = 8, RM_MANDELBROT = 9, RM_MANDELBULB = 10,
  RM_MENGERSPONGE = 11, RM_SIERPINSKI = 12, RM_CUSTOM = 13
};
/* Light type tags — src/utils/scenedata.h:10-15 == frag:72-75. */
enum { RM_LIGHT_POINT = 0, RM_LIGHT_DIRECTIONAL = 1, RM_LIGHT_SPOT = 2, RM_LIGHT_AREA = 3 };

/* Compile-time #defines of the reference shader (frag:4-15) as a runtime feature mask. */
enum {
  RM_FEAT_SKY_BACKGROUND = 1u << 0,      /* frag:5  */
  RM_FEAT_NIGHTSKY_BACKGROUND = 1u << 1, /* frag:6  (samples RmResources.noise) */
  RM_FEAT_DARK_BACKGROUND = 1u << 2,     /* frag:8  */
  RM_FEAT_WHITE_BACKGROUND = 1u << 3,    /* frag:9  */
  RM_FEAT_CLOUD = 1u << 4,               /* frag:12 */
  RM_FEAT_TERRAIN = 1u << 5,             /* frag:13 */
  RM_FEAT_SEA = 1u << 6,                 /* frag:14 (samples RmResources.noise) */
  RM_FEAT_PERLIN_BUMP = 1u << 7,         /* frag:15 */
  /* Not a reference #define — an opt-in evaluation scheme.  When set and power == 8 exactly, the Mandelbulb step
   * w ← c + r^8·(sin 8θ sin 8φ, cos 8θ, sin 8θ cos 8φ) (frag:789-793) is evaluated by three complex squarings of
   * (y + iρ) and of (z + ix)/ρ, ρ = |w.xz|, instead of acos/atan/sin/cos/pow, and m^3.5 as m³·√m: the same function
   * (angle-multiplication identities), different rounding (≈1e-6 relative per step), ≈3.5× fewer instructions.
   * Oracle and kernels implement it identically, so CPU/GPU parity stays bit-exact.  Any other power ignores the bit. */
  RM_FEAT_BULB_POWER8_ALGEBRAIC = 1u << 8
};
/* The checked-in shader's state: WHITE_BACKGROUND + PERLIN_BUMP (frag:9,15). */
#define RM_FEAT_REFERENCE_DEFAULT (RM_FEAT_WHITE_BACKGROUND | RM_FEAT_PERLIN_BUMP)

typedef enum rm_status {
  RM_OK = 0,
  RM_ERR_INVALID_ARGUMENT = 1, /* null pointer, bad size, rows out of range */
  RM_ERR_CAPACITY = 2,         /* > RM_MAX_OBJECTS / RM_MAX_LIGHTS (reference silently drops: realtimerender.cpp:662,737) */
  RM_ERR_UNSUPPORTED = 3,      /* CUSTOM objects; a feature whose resource (texture, noise, skybox, LTC table) was not supplied */
  RM_ERR_DEVICE = 4,           /* HIP runtime error; see rm_last_error() */
  RM_ERR_IO = 5,               /* file missing / unreadable */
  RM_ERR_PARSE = 6             /* scenefile schema violation */
} rm_status;

/* struct RayMarchObject — frag:135-168; uploaded by configureShapesUniforms, realtimerender.cpp:732-811. */
typedef struct RmObject {
  int32_t type;          /* RM_CUBE … RM_CUSTOM */
  float invModel[16];    /* world → object, column-major (obj.m_ctmInv) */
  float scaleFactor;     /* min diag of accumulated scale (realtimerender.cpp:749-751) */
  float shininess;
  float blend;
  float ior;
  float cAmbient[3];
  float cDiffuse[3];
  float cSpecular[3];
  float cReflective[3];
  float cTransparent[3];
  int32_t texLoc;        /* -1 = untextured; 0..numTextures-1 = index into RmResources.textures (rm_render_ex / rm_render_res) */
  float repeatU;
  float repeatV;
  int32_t isEmissive;    /* the rectangle drawn for an area light (raymarchscene.cpp:121-133): rendered as `color` */
  float color[3];
  int32_t lightIdx;
} RmObject;

/* struct LightSource — frag:212-230; uploaded by configureLightsUniforms, realtimerender.cpp:651-704. */
typedef struct RmLight {
  int32_t type;          /* RM_LIGHT_* */
  float color[3];
  float dir[3];          /* ctm·dir, NOT normalised (shader normalises) */
  float pos[3];
  float func[3];         /* attenuation (c0, c1, c2) */
  float angle;           /* spot outer angle, radians */
  float penumbra;        /* radians */
  float points[4][3];    /* area light corners tl,tr,br,bl in world space (realtimerender.cpp:688-693) */
  float intensity;
  int32_t twoSided;
} RmLight;

/* One object texture — objTextures[i] (frag:265), uploaded by initShapesTextures (realtimerender.cpp:267-303):
 * RGBA8, GL_LINEAR min/mag filter, GL_REPEAT wrap, no mipmaps; rows bottom-up (the reference mirrors the image
 * at load, raymarchscene.cpp:208).  `pixels` is a DEVICE pointer for rm_render_ex. */
#define RM_MAX_TEXTURES 10 /* src/realtime.h:17-27 */
typedef struct RmTexture {
  const uint8_t *pixels;
  int32_t width, height;
} RmTexture;

/*
 * Every sampler the shader reads, as the reference leaves them in GPU memory.  All images are RGBA8 with
 * GL_LINEAR filtering in binary32 weights; `pixels` are DEVICE pointers, rows in glTexImage2D order (row 0 = t 0).
 * A member with pixels == NULL is "not supplied"; rendering a scene that needs it fails with RM_ERR_UNSUPPORTED.
 */
#define RM_LTC_SIZE 64 /* LUT_SIZE, frag:47 */
typedef struct RmResources {
  const RmTexture *textures; /* objTextures[] (frag:265), GL_REPEAT */
  int32_t numTextures;
  RmTexture noise;           /* `noise` (frag:270; realtimerender.cpp:378-395: noise_texture_1.png, 256×256), GL_REPEAT;
                              * read by noiseV (frag:591-598) for NIGHTSKY_BACKGROUND and SEA */
  RmTexture skybox[6];       /* `skybox` cube map faces +X,−X,+Y,−Y,+Z,−Z (frag:267; initCubeMap,
                              * realtimerender.cpp:557-589), GL_CLAMP_TO_EDGE, filtered within a face
                              * (GL_TEXTURE_CUBE_MAP_SEAMLESS is never enabled); used when enableSkyBox */
  const uint8_t *ltc1;       /* LTC1 / LTC2 (frag:268-269): RM_LTC_SIZE² RGBA8 texels each.  The reference uploads   */
  const uint8_t *ltc2;       /* float tables with the unsized GL_RGBA internal format (realtimerender.cpp:908, 925), */
                             /* i.e. clamped to [0,1] and stored as 8-bit; rm_ltc_quantise() does that conversion.   */
} RmResources;
/* clamp(x,0,1)·255 rounded to nearest: float RGBA table → the 8-bit texels the reference's upload leaves. */
void rm_ltc_quantise(const float *table, uint8_t *out, int texels);

/* Camera uniforms — configureCameraUniforms, realtimerender.cpp:596-615. */
typedef struct RmCamera {
  float invProjView[16]; /* inverse(proj·view), column-major */
  float initialFar;      /* far plane (frag:247, 2425) */
  float eyePosition[4];  /* declared by the shader, unused by it (frag:245) */
} RmCamera;

/* Scalar uniforms — frag:248-255, 274, 282-283; realtimerender.cpp:621-645, 651-661, 809-810. */
typedef struct RmGlobals {
  float ka, kd, ks, kt;
  float power;           /* Mandelbulb power (settings.h:47, default 8) */
  float juliaSeed[2];
  float iTime;           /* seconds; 0 for offline frames */
  int32_t isTwoD;        /* 2-D Mandelbrot mode (frag:2431) */
} RmGlobals;

/* Option uniforms (frag:277-281) + the shader's compile-time constants as runtime knobs. */
typedef struct RmSettings {
  int32_t enableSoftShadow;
  int32_t enableReflection;
  int32_t enableRefraction;
  int32_t enableAmbientOcclusion;
  int32_t enableSkyBox;  /* frag:281, 2327: rays that miss every object sample RmResources.skybox */
  int32_t maxSteps;      /* MAX_STEPS, frag:28 (reference 256) */
  int32_t fractalIters;  /* MAX_STEPS_FRACTALS, frag:29 (reference 20) */
  int32_t mengerLevels;  /* loop bound of frag:1056 (reference 4) */
  int32_t numReflection; /* NUM_REFLECTION, frag:45 (reference 1) */
  uint32_t features;     /* RM_FEAT_* mask (reference: RM_FEAT_REFERENCE_DEFAULT) */
} RmSettings;

/* Fill *s with the reference's constants (256 steps, 20 fractal iterations, 4 Menger levels, 1 bounce,
 * WHITE_BACKGROUND|PERLIN_BUMP, all options off). */
void rm_settings_default(RmSettings *s);

/* ---- library / device ---------------------------------------------------------------------- */
int rm_abi_version(void);
/* sizeof() of ABI struct `which` as compiled into the library (0 RmObject, 1 RmLight, 2 RmCamera, 3 RmGlobals,
 * 4 RmSettings, 5 RmCounters, 6 RmHostSettings, 7 RmCameraData, 8 RmTexture, 9 RmPostSettings, 10 RmResources, 11 RmRay, 12 RmRayHit; -1 otherwise) so bindings can verify
 * layout. */
int rm_abi_sizeof(int which);
const char *rm_status_string(int status);
/* Thread-local text of the last failure in this thread ("" if none). */
const char *rm_last_error(void);
/* Number of HIP devices; <0 on error. */
int rm_device_count(void);
/* hipSetDevice for the calling thread. */
int rm_set_device(int device);

/* ---- the hot path -------------------------------------------------------------------------- */
/*
 * rm_render — replaces Realtime::rayMarch(): the five configure*Uniforms calls + glDrawArrays
 * (src/realtimerender.cpp:53-87) and everything resources/raymarch.{vert,frag} do per pixel.
 * Renders rows [rowBegin,rowEnd) of a W×H frame.  d_rgba receives (rowEnd-rowBegin)·W float4
 * (fragColor, frag:18), d_bright the same for BrightColor (frag:19) or NULL.  Asynchronous on
 * `stream` (a hipStream_t, NULL = default stream).  Host structs are copied before return.
 */
int rm_render(const RmCamera *cam, const RmObject *objs, int numObjects, const RmLight *lights,
              int numLights, const RmGlobals *g, const RmSettings *s, int W, int H, int rowBegin,
              int rowEnd, float *d_rgba, float *d_bright, void *stream);

/*
 * rm_render_ex — rm_render with object textures: objects whose texLoc is 0..numTextures-1 take their diffuse
 * colour from textures[texLoc] through the reference's uv maps (cube, cone, cylinder, sphere: frag:1299-1398) and
 * getDiffuse's blend (frag:1746-1781).  Other textured primitive types are rejected (the reference indexes
 * customTextures[texLoc-15] out of bounds for them).
 */
int rm_render_ex(const RmCamera *cam, const RmObject *objs, int numObjects, const RmLight *lights, int numLights,
                 const RmGlobals *g, const RmSettings *s, const RmTexture *textures, int numTextures, int W, int H,
                 int rowBegin, int rowEnd, float *d_rgba, float *d_bright, void *stream);

/*
 * rm_render_res — rm_render with every sampler the shader can read (RmResources): object textures, the noise
 * texture of the night sky / sea, the sky-box cube map and the LTC tables of area lights.  `res` may be NULL.
 */
int rm_render_res(const RmCamera *cam, const RmObject *objs, int numObjects, const RmLight *lights, int numLights,
                  const RmGlobals *g, const RmSettings *s, const RmResources *res, int W, int H, int rowBegin,
                  int rowEnd, float *d_rgba, float *d_bright, void *stream);

/*
 * rm_render_batch — numFrames whole W×H frames of ONE scene in one kernel launch (no reference counterpart; the reference
 * renders a sequence one draw call per frame, src/realtime.cpp:235-281): turntables, animation export, thumbnails, multi-view
 * sets, and frames too small to fill the GPU on their own.  Frame f has its own camera cams[f] and its own globals — globals[f]
 * when numGlobals == numFrames, globals[0] for every frame when numGlobals == 1 — (iTime, power, Julia seed, 2-D mode); the
 * object, light, settings and resource tables (res may be NULL) are shared.  Frame f is written to d_rgba + f·H·W·4, rows
 * bottom-up exactly as rm_render writes a whole frame; d_bright the same or NULL.  Every frame is bit-identical to rm_render of
 * the same camera and globals.  Asynchronous on `stream`; host arrays are copied before return.
 * numFrames == 0: RM_OK, nothing written.  RM_ERR_INVALID_ARGUMENT: numFrames < 0, numGlobals neither 1 nor numFrames, null
 * cams / globals, W or H <= 0; RM_ERR_CAPACITY: numFrames > RM_MAX_BATCH_FRAMES; the tables, resources and device pointers are
 * checked as rm_render_res checks them.
 * Schedule: the frames share one launch of the one-lane-per-pixel kernel (rm_debug_last_path() = 6) in raster tile order, 8×8
 * tiles unless rm_debug_set_tile_shape / RM_TILE_SHAPE pins a shape, no light split; a batch neither reads nor changes the
 * per-stream tuner and tile-order state of single-frame renders.  A frame that rm_render would give the wavefront pipeline
 * (path 5) is rendered as rm_render renders it, after the batched launch, in frame order on the same stream.  The scene blocks
 * of a batch (≈9.7 KB per frame, pinned on the host and on the device) live in a ring of up to 4 grow-only slots per device.
 */
int rm_render_batch(const RmCamera *cams, const RmGlobals *globals, int numGlobals, int numFrames, const RmObject *objs,
                    int numObjects, const RmLight *lights, int numLights, const RmSettings *s, const RmResources *res, int W,
                    int H, float *d_rgba, float *d_bright, void *stream);

/*
 * rm_render_supersampled — rm_render_batch with ss × ss samples per pixel, resolved inside the render kernel (no reference
 * counterpart: the reference's only anti-aliasing is FXAA, a blur over the finished 8-bit image).  The shape and every rule of
 * rm_render_batch — one scene, cams[f] and globals[f] (or globals[0]) per frame, numFrames == 1 for a still, numFrames·H·W float4
 * per output with rows bottom-up, d_bright may be NULL, asynchronous on `stream`, host arrays copied before return — plus `ss`,
 * the samples per pixel along each axis: 1, 2 or 4.  ss == 1 is rm_render_batch, exactly.
 * Definition of a pixel.  Let S be the frame rm_render_res writes for the same camera, globals, tables and settings at
 * ss·W × ss·H: sample (i, j) of output pixel (X, Y) is pixel (ss·X + i, ss·Y + j) of S.  fragColor and BrightColor, all four
 * channels, are reduced over the pixel's ss × ss block of S by a fixed tree of binary32 round-to-nearest adds (denormals kept),
 * one level of which is: x pairs first, a(x, y) = S(2x, y) + S(2x + 1, y), then y pairs, b(x, y) = a(x, 2y) + a(x, 2y + 1).
 * ss = 2 applies one level, ss = 4 applies the level twice (to S, then to its result); the sum is then multiplied by
 * 1.0f / (ss·ss) (0.25f or 0.0625f).  In NumPy, on float32 arrays: a = S[:, 0::2] + S[:, 1::2]; b = a[0::2] + a[1::2], repeated
 * for ss = 4, then b * np.float32(1 / ss**2).  The result is defined bit for bit; no ss·W × ss·H image exists in memory.
 * RM_ERR_INVALID_ARGUMENT: ss not 1, 2 or 4; ss·W or ss·H above INT_MAX / 8, or more samples than one launch can index (more
 * than 65535 rows of 8×8 sample tiles, or more than INT_MAX tiles per frame); everything rm_render_batch refuses, with its codes
 * (numFrames > RM_MAX_BATCH_FRAMES: RM_ERR_CAPACITY; numFrames == 0: RM_OK).  All of these are checked before any HIP call.
 * Schedule: ONE launch of the supersampling kernel over every frame (rm_debug_last_path() = 7, rm_debug_last_split() = 0), 8×8
 * sample tiles in raster order: no wavefront pipeline (rm_set_kernel_path is not consulted), no light split, no tile-shape pin, no
 * library workspace; it uses the batch ring of scene blocks (one block per frame, not per sample) and neither reads nor changes
 * the per-stream tuner and tile-order state of single-frame renders.  With rm_set_timing(1) it counts as one launch, all stage 1.
 * Added without a change of RM_ABI_VERSION (a new symbol and nothing else): bindings detect it by symbol lookup.
 */
int rm_render_supersampled(const RmCamera *cams, const RmGlobals *globals, int numGlobals, int numFrames, const RmObject *objs,
                           int numObjects, const RmLight *lights, int numLights, const RmSettings *s, const RmResources *res,
                           int W, int H, int ss, float *d_rgba, float *d_bright, void *stream);

/*
 * rm_render_adaptive — rm_render_supersampled for the pixels that show contrast, rm_render_batch for the rest (no reference
 * counterpart).  The shape and every rule of rm_render_supersampled — one scene, cams[f] and globals[f] (or globals[0]) per frame,
 * numFrames·H·W float4 per output with rows bottom-up, d_bright may be NULL, asynchronous on `stream`, host arrays copied before
 * return, ss = 1, 2 or 4 — plus a threshold and two optional outputs.
 * Definition of a pixel.  For frame f let F, Fb be the fragColor / BrightColor that rm_render_batch writes for it at W×H, and R,
 * Rb what rm_render_supersampled writes for it at the same W×H and ss (for ss = 1: R = F).  M(X, Y) is true iff for some
 * 4-neighbour N of (X, Y) inside the frame (left, right, below, above; border pixels have fewer) and some channel c of r, g, b of
 * fragColor: not (|F(X,Y).c − F(N).c| <= threshold), the subtraction one binary32 round-to-nearest operation, denormals kept.
 * Written with "not <=" so that a NaN difference flags the pixel.  Alpha and BrightColor are not looked at.  The relation is
 * symmetric: both pixels of a contrasting pair are flagged.  Then out(X, Y) = M ? R : F and bright(X, Y) = M ? Rb : Fb, all four
 * channels, bit for bit.  In NumPy on the float32 frame, c = F[..., :3]: dx = (~(abs(c[:, 1:] − c[:, :-1]) <= thr)).any(-1), the
 * same for rows, and each of dx, dy OR-ed into both pixels it separates.
 * d_mask (NULL, or numFrames·H·W bytes, frame-major, rows bottom-up) receives 1 where M, 0 elsewhere; d_refined (NULL, or
 * numFrames 32-bit words) receives the number of flagged pixels of each frame.  Both are device-accessible memory.
 * threshold: any value but NaN.  +inf flags nothing (unless a difference is NaN): the output is rm_render_batch's.  A negative
 * value flags every pixel of a frame larger than 1×1: the output is rm_render_supersampled's.  A 1×1 frame has no neighbour and is
 * never flagged.  The result does not depend on the order in which flagged pixels are refined.
 * RM_ERR_INVALID_ARGUMENT: threshold NaN; more than INT_MAX pixels per frame; everything rm_render_supersampled refuses, with its
 * codes (ss not 1, 2 or 4, the size limits — for ss = 1 too —, numFrames < 0, null arrays, numGlobals; numFrames >
 * RM_MAX_BATCH_FRAMES: RM_ERR_CAPACITY; numFrames == 0: RM_OK); d_mask or d_refined not device-accessible.  All of these but the
 * device-pointer checks are made before any HIP call.
 * Schedule: rm_debug_last_path() = 8, rm_debug_last_split() = 0.  Per chunk of frames three steps on `stream`: the
 * one-lane-per-pixel kernel as rm_render_batch launches it (raster order, 8×8 tiles) into the outputs, a classify kernel (mask,
 * lists of flagged pixels, counts), and for ss > 1 a refine kernel that supersamples the listed pixels and overwrites them.  No
 * wavefront pipeline (rm_set_kernel_path is not consulted), no light split, no tile-shape pin, no tile order; the per-stream tuner
 * and tile-order state of single-frame renders is neither read nor changed.  One slot of the batch ring holds the scene blocks of
 * the whole call.  No host synchronisation and no read-back inside the call: the number of flagged pixels stays on the device.
 * Workspace: per (device, stream) a grow-only list of 4 B per pixel of a chunk and a block of counters; frames go through the
 * three steps in chunks of k = min(numFrames, max(1, cap / (4·W·H))) frames, cap = the rm_set_workspace_limit value when set, else
 * 256 MiB (the rule of rm_post_process_batch).  A single frame over a set limit: RM_ERR_DEVICE.  rm_release_workspaces frees it.
 * With rm_set_timing(1) the whole call counts as one launch, all stage 1.
 * Added without a change of RM_ABI_VERSION (a new symbol and nothing else): bindings detect it by symbol lookup.
 */
int rm_render_adaptive(const RmCamera *cams, const RmGlobals *globals, int numGlobals, int numFrames, const RmObject *objs,
                       int numObjects, const RmLight *lights, int numLights, const RmSettings *s, const RmResources *res, int W,
                       int H, int ss, float threshold, float *d_rgba, float *d_bright, uint8_t *d_mask, uint32_t *d_refined,
                       void *stream);

/*
 * rm_render_accumulated — the mean of subFrames renders per output frame, taken inside the render kernel: depth of field (the
 * cameras of rm_camera_lens_samples), motion blur (globals with iTime across the shutter interval), or both (no reference
 * counterpart: the reference's scenefiles carry aperture and focalLength, and no shader reads them).  The shape and every rule of
 * rm_render_batch — one scene, numFrames·H·W float4 per output with rows bottom-up, d_bright may be NULL, asynchronous on `stream`,
 * host arrays copied before return — with subFrames cameras per output frame: cams holds numFrames·subFrames of them, sub-frame j
 * of output frame f is cams[f·subFrames + j], and numGlobals is 1 (globals[0] for every sub-frame) or numFrames·subFrames with the
 * same indexing.
 * Definition of a pixel.  Let S_j be the frame rm_render_batch writes for sub-frame j of f.  With n = subFrames: acc = S_0, then
 * acc = acc + S_j for j = 1 … n − 1 in that order, each add one binary32 round-to-nearest add, denormals kept, all four channels,
 * fragColor and BrightColor alike; then out = acc · c, c the binary32 value of 1.0f / (float)n (one IEEE division, then one
 * multiply).  In NumPy on float32 arrays: acc = S[0].copy(); for j in 1 … n − 1: acc = acc + S[j];
 * out = acc * (np.float32(1) / np.float32(n)).  The order is sequential on purpose: a wave loops over the sub-frames with one
 * wave-uniform scene block at a time and one running sum per channel.  subFrames == 1 is rm_render_batch, exactly (c = 1).  The
 * result is defined bit for bit, and no subFrames-sized image exists in device memory: the caller's numFrames outputs are all the
 * pixels there are, where rm_render_batch of every sub-frame plus a reduction needs 32 B per pixel per sub-frame with d_bright
 * (4.2 GB for a 3840×2160 still of 16 lens samples).
 * RM_ERR_INVALID_ARGUMENT: subFrames < 1 or > RM_MAX_SUBFRAMES; numGlobals neither 1 nor numFrames·subFrames; W or H above
 * INT_MAX / 8, or more 8×8 tiles than one launch can index (more than 65535 rows of them, or more than INT_MAX per frame);
 * RM_ERR_CAPACITY: numFrames·subFrames > RM_MAX_BATCH_FRAMES (one scene block is staged per sub-frame); numFrames == 0: RM_OK;
 * everything rm_render_batch refuses, with its codes.  All of these are checked before any HIP call.
 * Schedule: ONE launch of the accumulating kernel over every output frame (rm_debug_last_path() = 9, rm_debug_last_split() = 0), 8×8
 * tiles in raster order: no wavefront pipeline (rm_set_kernel_path is not consulted), no light split, no tile-shape pin, no tile
 * order, no library workspace; it uses the batch ring of scene blocks (one block per sub-frame — the only memory that grows with
 * subFrames, ≈9.7 KB each) and neither reads nor changes the per-stream tuner and tile-order state of single-frame renders.  With
 * rm_set_timing(1) it counts as one launch, all stage 1.
 * Added without a change of RM_ABI_VERSION (a new symbol and nothing else): bindings detect it by symbol lookup.
 */
int rm_render_accumulated(const RmCamera *cams, const RmGlobals *globals, int numGlobals, int numFrames, int subFrames,
                          const RmObject *objs, int numObjects, const RmLight *lights, int numLights, const RmSettings *s,
                          const RmResources *res, int W, int H, float *d_rgba, float *d_bright, void *stream);

/*
 * rm_render_animated — rm_render_accumulated where every sub-frame may have an object table and a light table of its own: objects and
 * lights that move, appear or change material from frame to frame (animation export in one launch) and during the shutter interval
 * (motion blur of what moves, not only of what iTime drives) — no reference counterpart.  The shape and every rule of
 * rm_render_accumulated — numFrames·H·W float4 per output with rows bottom-up, d_bright may be NULL, asynchronous on `stream`, host
 * arrays copied before return — with blocks = numFrames·subFrames and block b = f·subFrames + j for sub-frame j of output frame f:
 * cams holds `blocks` cameras; numGlobals, numObjectTables and numLightTables are each 1 (entry 0 for every block) or `blocks`;
 * object table b is objs + b·numObjects, light table b is lights + b·numLights.  numObjects and numLights are the same for every
 * block; everything inside an entry may differ between blocks (type, transform, materials, texLoc, emissive flag, light kind).
 * Settings and resources are shared.  rm_object_translated moves an object; a light moves by writing its pos / dir / points.
 * Definition of a pixel.  Let S_b be the frame rm_render_res writes for block b's camera, globals, object table and light table.
 * Output frame f is the rm_render_accumulated reduction of S_{f·n} … S_{f·n + n − 1}, n = subFrames: acc = S_{f·n}, then
 * acc = acc + S_{f·n + j} for j = 1 … n − 1 in that order, each add one binary32 round-to-nearest add, denormals kept, all four
 * channels, fragColor and BrightColor alike; then out = acc · c, c the binary32 value of 1.0f / (float)n.  subFrames == 1 gives
 * frame f = S_f.  The result is defined bit for bit.  numObjectTables == numLightTables == 1 is rm_render_accumulated, exactly
 * (for subFrames == 1: rm_render_batch), and one table repeated `blocks` times gives the same bits as passing it once.
 * RM_ERR_INVALID_ARGUMENT: numObjectTables or numLightTables neither 1 nor numFrames·subFrames; null objs / lights where the count
 * needs them; everything rm_render_accumulated refuses, with its codes (subFrames < 1 or > RM_MAX_SUBFRAMES, numGlobals, the size
 * limits; numFrames·subFrames > RM_MAX_BATCH_FRAMES: RM_ERR_CAPACITY; numFrames == 0: RM_OK).  The tables of EVERY block are checked
 * as rm_render_res checks them (a CUSTOM object, a texLoc without its texture, an area light without the LTC tables in any block:
 * RM_ERR_UNSUPPORTED); the error text names the block.  All of these are checked before any HIP call.
 * Schedule: ONE launch (rm_debug_last_path() = 10, rm_debug_last_split() = 0), 8×8 tiles in raster order, of the kernel class the
 * most general block needs — samplers if any block reads one, secondary rays if any block can fire them, the single-Mandelbulb
 * classes only if every block is a lone Mandelbulb (its plain form only if every block has it); the classes are specialisations
 * with identical pixels.  subFrames == 1 launches the one-lane-per-pixel kernel over the blocks; subFrames > 1 the animated kernel,
 * whose workgroups stage the object table again (two barriers) only ahead of a sub-frame whose table differs from the one before it:
 * shared object tables (depth of field, moving lights) pay nothing beyond rm_render_accumulated.  No wavefront pipeline
 * (rm_set_kernel_path is not consulted), no light split, no tile-shape pin, no tile order, no library workspace; it uses one slot of
 * the batch ring of scene blocks (one block per sub-frame, ≈9.7 KB each) and neither reads nor changes the per-stream tuner and
 * tile-order state of single-frame renders.  With rm_set_timing(1) it counts as one launch, all stage 1.
 * Added without a change of RM_ABI_VERSION (a new symbol and nothing else): bindings detect it by symbol lookup.
 */
int rm_render_animated(const RmCamera *cams, const RmGlobals *globals, int numGlobals, const RmObject *objs, int numObjects,
                       int numObjectTables, const RmLight *lights, int numLights, int numLightTables, int numFrames, int subFrames,
                       const RmSettings *s, const RmResources *res, int W, int H, float *d_rgba, float *d_bright, void *stream);

/*
 * rm_render_gbuffer — what the primary ray of every pixel HIT instead of the colour shading makes of it: surface normal, depth,
 * object index and, optionally, the surface point (no reference counterpart: the shader keeps these in locals).  For compositing
 * and depth-aware post effects, denoiser and edge guides, picking and masks, and a cheap geometry-only preview.  The call shape is
 * rm_render_batch's without lights and resources: numFrames whole W×H frames of ONE object table in one launch, frame f with its own
 * camera cams[f] and globals (globals[f] when numGlobals == numFrames, globals[0] when numGlobals == 1).  Frame f starts at f·W·H
 * elements of each output; rows bottom-up.  Asynchronous on `stream`; host arrays are copied before return.
 * Definition, bit for bit.  The G-buffer of a frame is the RayMarchRes / IntersectionInfo of main's first render call
 * (frag:2388-2392, 2443, 2318-2337, 1453-1484, 1436-1444, 1679-1691).  For pixel (x, y): ro, rd = the primary ray of rm_render —
 * the varyings interpolated from the ray planes, the divisions by w, normalize; far = cam->initialFar;
 * res = raymarch(ro, rd, far, OUTSIDE) with the call's maxSteps.  Hit (res.intersectObj != -1): objectId = res.intersectObj — the
 * march's index, so the emissive rectangle of an area light reports its own index, not the −1 that `info` keeps —; depth = res.d,
 * the distance along the normalised rd from ro on the near plane (not a view-space z); p = rd·res.d + ro in render's fused form;
 * n = getNormal(p), then bumpNormal(n, p, 10, 2) when RM_FEAT_PERLIN_BUMP is set: the normal render hands getPhong.  Miss:
 * objectId = −1, depth = far (RenderInfo.d of a miss, frag:2328, not the march's ray depth), n = (0, 0, 0), p = (0, 0, 0).
 * d_normalDepth: float4 (n.x, n.y, n.z, depth) per pixel; d_objectId: int32 per pixel; d_position: float4 (p.x, p.y, p.z,
 * hit ? 1 : 0) per pixel, or NULL: nothing is written for it and the other two outputs are the same bits.
 * Of RmSettings the call reads maxSteps, the bounds of the fractals' loops (fractalIters, mengerLevels, the power-8 form) and
 * RM_FEAT_PERLIN_BUMP.  Lights, textures, sky box, LTC tables, shadows, ambient occlusion, reflection and refraction play no part:
 * a texLoc or enableSkyBox without its sampler is not an error here.
 * numFrames == 0: RM_OK, nothing written.  RM_ERR_INVALID_ARGUMENT: numFrames < 0, numGlobals neither 1 nor numFrames, null cams /
 * globals, W or H <= 0 or above INT_MAX / 8 or more tiles than one launch can index, null s or objs, a negative loop bound, a null
 * d_normalDepth / d_objectId, an output that is not device memory; RM_ERR_CAPACITY: numFrames > RM_MAX_BATCH_FRAMES, numObjects >
 * RM_MAX_OBJECTS; RM_ERR_UNSUPPORTED, rather than a G-buffer that would lie: RM_FEAT_TERRAIN, RM_FEAT_CLOUD or RM_FEAT_SEA in the
 * settings (a layer may cover the object table), isTwoD in any frame's globals (the error text names the frame), a CUSTOM object.
 * All of these are checked, in this order, before any HIP call.
 * Schedule: ONE launch of the G-buffer kernel of the table's march class (rm_debug_last_path() = 11, rm_debug_last_split() = 0), 8×8
 * tiles in raster order: no wavefront pipeline (rm_set_kernel_path is not consulted), no light split, no tile-shape pin, no tile
 * order, no library workspace; it uses one slot of the batch ring of scene blocks and neither reads nor changes the per-stream tuner
 * and tile-order state of single-frame renders.  With rm_set_timing(1) it counts as one launch, all stage 1.
 * Added without a change of RM_ABI_VERSION (a new symbol and nothing else): bindings detect it by symbol lookup.
 */
int rm_render_gbuffer(const RmCamera *cams, const RmGlobals *globals, int numGlobals, int numFrames, const RmObject *objs,
                      int numObjects, const RmSettings *s, int W, int H, float *d_normalDepth, int32_t *d_objectId,
                      float *d_position, void *stream);

/*
 * rm_trace_rays — what ARBITRARY rays hit: the closest hit of each ray, or the renderer's own shadow march along it (no reference
 * counterpart: the shader only traces the rays it makes itself).  For picking the object under the mouse, keeping a fly-through
 * camera out of the scene, finding the distance to focus rm_camera_lens_samples at, and line-of-sight / soft-visibility tests
 * between two points.  d_rays: numRays RmRay in device memory; d_hits: numRays RmRayHit in device memory (both 16-byte aligned);
 * the object table, g and s are host memory, copied before return.  Asynchronous on `stream`.
 * Definition, bit for bit.  dir is used as given, NOT normalised: t is in units of |dir|, and a ray that copies primaryRay's ro
 * and rd (rm_camera_rays) reproduces rm_render_gbuffer exactly.
 * RM_TRACE_CLOSEST: res = raymarch(origin, dir, tMax, OUTSIDE) (frag:1453-1484) with the call's maxSteps.  Hit (res.intersectObj !=
 * -1): objectId = res.intersectObj — the march's index, an emissive rectangle reports its own —; t = res.d; position = dir·t +
 * origin in render's fused form (frag:2318-2337); normal = getNormal(position) (frag:1436-1444), then bumpNormal(normal, position,
 * 10, 2) (frag:1679-1691) when RM_FEAT_PERLIN_BUMP is set.  With RM_TRACE_NO_NORMAL normal and position are stored as zeros and no
 * tap is evaluated; objectId and t are the same bits.  Miss: objectId = −1, t = tMax as given (not the march's ray depth — the
 * choice of rm_render_gbuffer's depth = far), normal and position zeros.
 * RM_TRACE_OCCLUSION: r = softshadow(origin, dir, 0, tMax, 8) (frag:1703-1725), lightTerm's shadow march.  objectId =
 * r.intersectObj (−1: nothing in the way), t = r.d = the penumbra factor, tracked whatever s->enableSoftShadow says; normal and
 * position zeros.  What lightTerm reads as visibility is objectId == −1 ? t : 0.
 * Invalid ray: a non-finite component of origin or dir, dir all zeros, tMax NaN or negative (+inf is valid).  It stores objectId =
 * RM_RAY_INVALID, t = 0 and zeros, and evaluates nothing.  Rays are device data: the host cannot refuse them.  `reserved` is not
 * read.
 * Of RmSettings the call reads maxSteps, the bounds of the fractals' loops (fractalIters, mengerLevels, the power-8 form) and
 * RM_FEAT_PERLIN_BUMP; of RmGlobals power, juliaSeed and iTime.  Lights, samplers and cameras play no part.  The result of a ray
 * does not depend on which other rays share its call.
 * numRays == 0: RM_OK, nothing read or written.  RM_ERR_INVALID_ARGUMENT: numRays < 0 (every non-negative int fits one launch),
 * null g or s, a null table with numObjects > 0 or numObjects < 0, mode bits other than the three below or RM_TRACE_NO_NORMAL
 * together with RM_TRACE_OCCLUSION, a negative loop bound, null or misaligned d_rays / d_hits, an array that is not device memory;
 * RM_ERR_CAPACITY: numObjects > RM_MAX_OBJECTS; RM_ERR_UNSUPPORTED: RM_FEAT_TERRAIN, RM_FEAT_CLOUD or RM_FEAT_SEA in the settings
 * (rays through the layers are not defined here), g->isTwoD, a CUSTOM or unknown object type.  All of these but the device-memory
 * check of the two arrays are made, in this order, before any HIP call.
 * Schedule: ONE launch, one lane per ray, of the trace kernel of the table's march class (rm_debug_last_path() = 12,
 * rm_debug_last_split() = 0); it uses one slot of the batch ring of scene blocks and neither reads nor changes the per-stream tuner
 * and tile-order state of single-frame renders, and no library workspace.  With rm_set_timing(1) it counts as one launch, all
 * stage 1.  Rays that share a wave (64 consecutive rays) and go different ways cost what the longest of them costs: a caller with
 * many rays does well to keep neighbours together (for a camera's rays, 8×8 pixel tiles).
 * Added without a change of RM_ABI_VERSION (new symbols and nothing else): bindings detect them by symbol lookup.
 */
typedef struct RmRay { float origin[3]; float tMax; float dir[3]; int32_t reserved; } RmRay;            /* 32 bytes */
typedef struct RmRayHit { float normal[3]; float t; float position[3]; int32_t objectId; } RmRayHit;   /* 32 bytes */
#define RM_TRACE_CLOSEST 0u   /* nearest hit, with normal and position */
#define RM_TRACE_NO_NORMAL 1u /* flag on CLOSEST: id and t only, normal and position stored as zeros */
#define RM_TRACE_OCCLUSION 2u /* the renderer's own shadow march: occluder id and penumbra factor */
#define RM_RAY_INVALID (-2)
int rm_trace_rays(const RmRay *d_rays, int numRays, const RmObject *objs, int numObjects, const RmGlobals *g, const RmSettings *s,
                  unsigned mode, RmRayHit *d_hits, void *stream);
/*
 * rm_camera_rays — the primary rays of pixels of a W×H frame of `cam`, on the host (no HIP call, no GPU): origin and dir are bit
 * for bit the ro and rd of rm_render and rm_render_gbuffer for that pixel (the ray planes of raymarch.vert:23-24 interpolated to
 * the pixel centre, the divisions by w, normalize: frag:2388-2392), tMax = cam->initialFar, reserved = 0.  xy: n pairs (x, y), y =
 * 0 the bottom row; or NULL, then n must be W·H and the rays come out row-major, row 0 at the bottom.  RM_ERR_INVALID_ARGUMENT: a
 * null cam or out, W or H <= 0, n < 0, n != W·H without xy, a pixel outside the frame (nothing is written then).
 */
int rm_camera_rays(const RmCamera *cam, int W, int H, const int32_t *xy, int n, RmRay *out);
/*
 * rm_shade_rays — the renderer's full COLOUR for arbitrary rays: the shader's whole main, from the background colour to BrightColor,
 * for rays from device memory (no reference counterpart: the shader only shades the rays of its one pinhole camera).  For 360°
 * panoramas and fisheyes, the faces of an environment probe, stereo pairs, and the colour along a handful of rays (a mirror preview,
 * a light probe).  d_rays: numRays RmRay in device memory; d_rgba and d_bright (may be NULL): numRays float4 each in device memory
 * (all three 16-byte aligned); the tables, g, s and res (may be NULL) are host memory, copied before return.  Asynchronous on
 * `stream`.
 * Definition, bit for bit.  The colour of ray i is what main computes for a pixel whose primary ray is ro = origin, rd = dir, with
 * far = the call's `far`: the background colour for rd (frag:2405-2419: sky, night sky, white, dark, later bits overriding earlier
 * ones); render(ro, rd, OUTSIDE, far, bg) (frag:2443, 2318-2375), the sky box on a miss; the reflection loop (frag:2491-2524) and the
 * refraction pair (frag:2526-2570); fragColor = phong + refl + refr with its alpha 1 + bounces (frag:2572); bright = BrightColor of
 * it (frag:1938-1946), (0, 0, 0, 1) for a ray that hit nothing.  dir is used as given, NOT normalised, which is rm_trace_rays'
 * rule: a ray that copies primaryRay's ro and rd (rm_camera_rays) reproduces rm_render's pixel in every bit, colour and bright.  The
 * shader's Phong (the view vector, the specular term) assumes a unit rd: pass unit directions unless a scaled one is meant.
 * `far` is ONE value per call, as the shader has one per frame; RmRay.tMax is NOT read (nor is `reserved`).  Every device function
 * reads far as uniform over the wave, and the bulb class marches a pixel's shadow rays on whichever lane is idle.
 * Invalid ray: a non-finite component of origin or dir, or dir all zeros.  It stores (0, 0, 0, 0) in both outputs and evaluates
 * nothing; a valid ray's alpha is >= 1, so alpha 0 marks it.  Rays are device data: the host cannot refuse them.  The result of a ray
 * does not depend on which other rays share its call.
 * numRays == 0: RM_OK, nothing read or written.  Otherwise, in this order and all but the last before any HIP call:
 * RM_ERR_INVALID_ARGUMENT: numRays < 0, null g or s, a null table with a positive count or a negative count, far NaN, negative or
 * infinite; RM_ERR_UNSUPPORTED: RM_FEAT_TERRAIN, RM_FEAT_CLOUD or RM_FEAT_SEA (rays through the layers are not defined here),
 * g->isTwoD; then rm_render_res's checks of the scene with its statuses: a bad texture table, RM_ERR_CAPACITY beyond RM_MAX_OBJECTS /
 * RM_MAX_LIGHTS / RM_MAX_TEXTURES, a negative loop bound, RM_ERR_UNSUPPORTED for a night sky, sky box, texLoc or area light without
 * its sampler and for a CUSTOM or unknown object or light type; RM_ERR_INVALID_ARGUMENT: null or misaligned d_rays / d_rgba, a
 * misaligned d_bright; an array or a sampler's pixels that are not device memory.
 * Schedule: ONE launch, one lane per ray, of the shade kernel of the scene's class (the twelve classes of the render kernels;
 * rm_debug_last_path() = 13, rm_debug_last_split() = 0); it uses one slot of the batch ring of scene blocks and neither reads nor
 * changes the per-stream tuner and tile-order state of single-frame renders, and no library workspace: no wavefront pipeline, no
 * light split.  With rm_set_timing(1) it counts as one launch, all stage 1.  Rays that share a wave (64 consecutive rays) and go
 * different ways cost what the longest of them costs: keep neighbours together (for an image, 8×8 pixel tiles).
 * Added without a change of RM_ABI_VERSION (a new symbol and nothing else): bindings detect it by symbol lookup.
 */
int rm_shade_rays(const RmRay *d_rays, int numRays, float far, const RmObject *objs, int numObjects, const RmLight *lights, int numLights,
                  const RmGlobals *g, const RmSettings *s, const RmResources *res /* may be NULL */, float *d_rgba,
                  float *d_bright /* may be NULL */, void *stream);
/*
 * rm_shade_rays_layers — rm_shade_rays THROUGH the procedural layers: terrain, sea and clouds (RM_FEAT_TERRAIN, RM_FEAT_SEA,
 * RM_FEAT_CLOUD), which rm_shade_rays refuses.  For landscape panoramas and environment-probe faces: terrain below, clouds and sky
 * above, the sea to the horizon.  The arguments are rm_shade_rays' with imageWidth behind `far`.
 * imageWidth: the width in pixels of the image the rays belong to — the frame's W for a camera's rays, the panorama's W for a
 * panorama.  It is the one quantity of a frame a ray does not carry: seaRender divides the epsilon of the sea normal by
 * iResolution.x (frag:2284-2310), and nothing else reads it.  It must be >= 1 in every call, whatever the feature mask.
 * Definition, bit for bit: rm_shade_rays' with the layer lines of main no longer left out.  Behind render(ro, rd, OUTSIDE, far, bg)
 * come sea, then terrain, then cloud (frag:2444-2456): the sea bounded by the render's distance, the terrain by the sea's, the cloud
 * by the terrain's.  Precedence (frag:2459-2475): cloud over terrain over sea over the object hit; a layer hit returns the layer's
 * colour with alpha 1 and BrightColor of it, and fires no secondary rays.  The same three layers apply behind every reflection
 * bounce (frag:2506-2518: terrain and cloud end the bounce loop, the sea does not) and behind the refraction exit (frag:2555-2567).
 * With RM_FEAT_CLOUD the call's `far` is validated but NOT read: the shader sets far = 2000 (frag:2422-2426), and the equality with
 * rm_render is the anchor.  A ray that copies rm_camera_rays' origin and dir, with imageWidth = W and far = cam->initialFar, gives
 * rm_render_res's pixel in every bit, colour and bright, for every feature mask.  With no layer bit in s->features the output is
 * rm_shade_rays' in every bit (the same kernels run).
 * Invalid rays, dir used as given, ONE far per call, RmRay.tMax not read: as rm_shade_rays has them.
 * numRays == 0: RM_OK.  Otherwise rm_shade_rays' checks in its order, all but the last before any HIP call, with two differences: no
 * refusal of the layers, and imageWidth < 1 is RM_ERR_INVALID_ARGUMENT right after `far`.  The scene checks are rm_render_res's, so
 * RM_FEAT_SEA without the noise sampler is RM_ERR_UNSUPPORTED with its text.  g->isTwoD stays RM_ERR_UNSUPPORTED.
 * Schedule: ONE launch, one lane per ray (rm_debug_last_path() = 14, rm_debug_last_split() = 0): with a layer bit the layers' shade
 * kernel of the scene's class (textured or not, secondary rays or not), without one rm_shade_rays' kernel.  One slot of the batch
 * ring of scene blocks; no tuner, tile-order or workspace state is read or changed.  With rm_set_timing(1) one launch, all stage 1.
 * Added without a change of RM_ABI_VERSION (new symbols and nothing else): bindings detect them by symbol lookup.
 */
int rm_shade_rays_layers(const RmRay *d_rays, int numRays, float far, int imageWidth, const RmObject *objs, int numObjects,
                         const RmLight *lights, int numLights, const RmGlobals *g, const RmSettings *s,
                         const RmResources *res /* may be NULL */, float *d_rgba, float *d_bright /* may be NULL */, void *stream);
/*
 * rm_light_probes — SH9 radiance probes, shaded and reduced in ONE launch: numDirs rays from each of numProbes positions along the
 * rows of a direction table, each shaded by rm_shade_rays' own code, its colour and hit flag multiplied into the row's nine basis
 * values and summed per probe inside the kernel by a fixed binary32 tree.  For a grid of irradiance probes that lights moving objects
 * in a static scene.  No device memory proportional to numProbes·numDirs exists at any time: the caller who composes the same from
 * rm_shade_rays writes 32 B per ray, reads 16 B per ray back and projects them in passes of their own, for 160 B per probe.
 * rm_sphere_directions fills a table on the host.
 * d_positions: numProbes float4 in device memory (w is not read); d_dirs: numSets·numDirs RmProbeDir in device memory; d_out:
 * numProbes RmLightProbe in device memory (all three 16-byte aligned); the tables, g, s and res (may be NULL) are host memory, copied
 * before return.  Asynchronous on `stream`.
 * Definition, bit for bit.  Probe i uses rows (i mod numSets)·numDirs + k, for k = 0 … numDirs − 1; numDirs is a power of two in
 * 1 … RM_MAX_PROBE_DIRS.  For row e: let (c, hit) belong to the ray origin = position_i, dir = e.dir (used as given, NOT normalised),
 * with the call's `far`: c is the r, g, b that rm_shade_rays stores for that ray, and hit is whether main's primary march found a
 * surface — observable as rm_trace_rays(RM_TRACE_CLOSEST | RM_TRACE_NO_NORMAL) with tMax = far giving objectId >= 0.  A row whose dir
 * is invalid by rm_shade_rays' rule (a non-finite component, or all three zero) gives c = 0, hit = false, and evaluates nothing.  Let
 * h = hit ? 1.0f : 0.0f.  The leaf of row k is leaf[j] = (e.basis[j]·c.r, e.basis[j]·c.g, e.basis[j]·c.b, e.basis[j]·h) for j = 0 … 8,
 * each ONE binary32 multiplication, unfused.  sh[j] is the pairwise tree over the leaf index, level by level: s[m] = s[2m] + s[2m + 1],
 * which is rm_field_ambient's tree.  hits is the number of rays with hit.  The record's `reserved` is stored as zeros.
 * A probe with a non-finite position stores hits = RM_RAY_INVALID and zeros in every other word, and evaluates nothing.  Positions and
 * rows are device data: the host cannot refuse them.  `reserved` and `pad` of a row are not read.  The result of a probe does not
 * depend on which other probes share its call.  The contract covers finite tables: a non-finite basis value may put a NaN into the
 * sums; its sign and payload are not specified.
 * The w channel is the projection of "something is there within far": 1 − that is the probe's directional sky visibility.
 * rm_sphere_directions(numDirs, numSets, out), host only (no HIP call): for set s and index k, in binary64 and then rounded once to
 * binary32, z = 1 − (2k + 1) / numDirs, r = sqrt(1 − z²), φ = 2π·frac(k·0.6180339887498949 + s·0.7548776662466927), dir = (r cos φ,
 * r sin φ, z) — spherical Fibonacci points, one rotation about z per set — and basis[j] = (4π / numDirs)·Y_j(dir), evaluated on the
 * binary64 direction and rounded once: the Monte-Carlo weight of a uniform direction times the nine real spherical harmonics of
 * bands 0 to 2 in the usual order,
 *   Y0 = sqrt(1/4π);  Y1 = sqrt(3/4π)·y;  Y2 = sqrt(3/4π)·z;  Y3 = sqrt(3/4π)·x;  Y4 = sqrt(15/4π)·x·y;  Y5 = sqrt(15/4π)·y·z;
 *   Y6 = sqrt(5/16π)·(3z² − 1);  Y7 = sqrt(15/4π)·x·z;  Y8 = sqrt(15/16π)·(x² − y²).
 * reserved and pad are written as zeros.  With that table sh[j].rgb are the probe's radiance coefficients and Σ_j A_j·sh[j]·Y_j(n), A =
 * π, 2π/3, π/4 per band, its irradiance (Ramamoorthi & Hanrahan 2001).  A caller may pass any table of their own — an ambient cube,
 * fewer bands, importance-weighted directions: the kernel only multiplies and adds.  It refuses numDirs and numSets as below, then a
 * null out.
 * rm_light_probes refuses, in this order and all but the last before any HIP call: RM_ERR_INVALID_ARGUMENT: numProbes < 0; numDirs
 * not a power of two in 1 … RM_MAX_PROBE_DIRS; numSets below 1 or numSets·numDirs above RM_MAX_PROBE_TABLE.  Then numProbes == 0:
 * RM_OK, nothing read or written.  Then RM_ERR_INVALID_ARGUMENT: numProbes·numDirs above INT_MAX; null g or s, a null table with a
 * positive count or a negative count; far NaN, negative or infinite; RM_ERR_UNSUPPORTED: RM_FEAT_TERRAIN, RM_FEAT_CLOUD or
 * RM_FEAT_SEA (rays through the layers are not defined here), g->isTwoD; then rm_render_res's checks of the scene with its statuses,
 * as rm_shade_rays has them; RM_ERR_INVALID_ARGUMENT: a null or misaligned d_positions, d_dirs or d_out (16 bytes); an array or a
 * sampler's pixels that are not device memory.
 * Schedule: ONE launch of the probe kernel of the scene's class (the twelve classes of the render kernels; rm_debug_last_path() = 21,
 * rm_debug_last_split() = 0), 256-lane workgroups, (probe, row) pairs flattened over lanes so that lane mod numDirs is the row: up to
 * 64 directions a wave holds 64 / numDirs probes and folds each segment by log2(numDirs) xor-shuffle levels over the 36 words of the
 * leaf; more are numDirs / 64 passes of 64 by one wave on one probe, whose sums join in leaf order with one pending sum per level.
 * binary32 addition is commutative in every bit, so the butterfly has the tree's words.  A lane reads its own 64-byte row; a record
 * is ten 16-byte stores.  One slot of the batch ring of scene blocks; no tuner, tile-order or workspace state is read or changed, and
 * nothing is allocated.  With rm_set_timing(1) it counts as one launch, all stage 1.  The rays of a wave share an origin or
 * neighbouring ones and go every way: a wave costs what its longest ray costs.
 * Added without a change of RM_ABI_VERSION (new symbols and nothing else): bindings detect them by symbol lookup.
 */
typedef struct RmProbeDir   { float dir[3]; float reserved; float basis[9]; float pad[3]; } RmProbeDir;   /* 64 bytes */
typedef struct RmLightProbe { float sh[9][4]; int32_t hits; int32_t reserved[3]; } RmLightProbe;           /* 160 bytes */
#define RM_MAX_PROBE_DIRS  1024
#define RM_MAX_PROBE_TABLE 4096   /* numSets * numDirs */
int rm_sphere_directions(int numDirs, int numSets, RmProbeDir *out /* host */);
int rm_light_probes(const float *d_positions /* float4 each, w not read */, int numProbes,
                    const RmProbeDir *d_dirs, int numDirs, int numSets, float far,
                    const RmObject *objs, int numObjects, const RmLight *lights, int numLights,
                    const RmGlobals *g, const RmSettings *s, const RmResources *res /* may be NULL */,
                    RmLightProbe *d_out, void *stream);
/*
 * rm_light_grid_irradiance — light at POINTS from a grid of rm_light_probes' SH9 records, ONE launch: the query half of the probes.
 * Per point the eight probes around it are blended trilinearly, probes inside geometry (hits < 0) are left out, DDGI's backface
 * term (Majercik et al. 2019) keeps light from behind the surface away, and each probe's radiance is convolved with the clamped
 * cosine lobe of the point's normal (Ramamoorthi & Hanrahan 2001).  For the hit points of a G-buffer, mesh vertices and particles.
 * No memory proportional to numPoints exists but the result: the caller who composes the same in array arithmetic gathers eight
 * probes per point, 1152 B, and blends in passes of their own.
 * d_probes: dims[0]·dims[1]·dims[2] RmLightProbe in device memory, exactly as rm_light_probes stores them, consumed where they lie:
 * the probe at (i, j, k) is at index i + dims[0]·(j + dims[1]·k) and its world position is origin_a + (float)index_a·step_a,
 * unfused.  Byte offsets are 64-bit.  d_points, d_normals: numPoints float4 each in device memory (w is not read); d_out: numPoints
 * RmGridLight in device memory (all four 16-byte aligned); dims, origin and step are host memory, copied before return.
 * Asynchronous on `stream`.
 * Definition, bit for bit.  Every operation is ONE binary32 operation as written, unfused; division and sqrt are the correctly
 * rounded ones (rm_light_grid.h is this text in C++).  Per point p with normal n:
 *  1. p or n with a non-finite component, or n all zeros: the record is probes = RM_RAY_INVALID and zeros elsewhere, and nothing is
 *     evaluated.  n is used as given, NOT normalised (rm_light_probes' rule for its directions).
 *  2. Per axis a: u_a = (p_a − origin_a) / step_a, clamped to [0, dims_a − 1]: a u_a not greater than 0 becomes +0, a u_a above
 *     dims_a − 1 becomes dims_a − 1, an infinite u_a clamps like any other — a point outside the box takes the border's light, it is
 *     not refused.  cell_a = min((int)floor(u_a), dims_a − 2), f_a = u_a − (float)cell_a.
 *  3. Corner c = cx + 2·cy + 4·cz is probe cell + (cx, cy, cz); its trilinear weight is t_c = (wx·wy)·wz with w_a = c_a ? f_a : 1 − f_a.
 *  4. A corner probe is valid iff its hits >= 0.  Of an invalid probe only hits is read: its sh words may hold anything, NaNs
 *     included, and never reach a sum.
 *  5. With RM_LIGHT_GRID_FACING, per valid corner: d = probePosition − p per component, len = sqrt((dx·dx + dy·dy) + dz·dz);
 *     len == 0 gives face = 1, otherwise cosv = ((dx·nx + dy·ny) + dz·nz) / len, b = (cosv + 1)·0.5, face = b·b + 0.2.  Without the
 *     flag face = 1 and none of this is evaluated.  w_c = t_c·face for a valid probe and +0 for an invalid one.
 *  6. W = ((w0 + w1) + (w2 + w3)) + ((w4 + w5) + (w6 + w7)).  probes = the number of valid corners with w_c > 0.  probes == 0: the
 *     record is probes = 0, weight = W and zeros in e, and no sh word is read.
 *  7. The cosine-lobe weights of n, once per point, from constants evaluated in binary64 and rounded once to binary32,
 *     K0 = π·sqrt(1/4π), K1 = (2π/3)·sqrt(3/4π), K2 = (π/4)·sqrt(15/4π), K6 = (π/4)·sqrt(5/16π), K8 = (π/4)·sqrt(15/16π):
 *     k0 = K0; k1 = K1·y; k2 = K1·z; k3 = K1·x; k4 = K2·(x·y); k5 = K2·(y·z); k6 = K6·(3·(z·z) − 1); k7 = K2·(x·z);
 *     k8 = K8·(x·x − y·y), with (x, y, z) = n — rm_sphere_directions' order of Y0 … Y8.
 *  8. Per valid corner and channel ch = 0 … 3: E_c[ch] = k0·sh[0][ch], then E_c[ch] = E_c[ch] + k_j·sh[j][ch] for j = 1 … 8 in
 *     order.  e[ch] = T(w_c·E_c[ch]) / W, T the three-level tree of step 6 over the corners; an invalid corner's leaf is +0, a
 *     valid corner of weight zero has the leaf 0·E_c[ch].  e is not clamped: SH ringing may make it negative.  e[3] is the same
 *     convolution of "something is there within far", so 1 − e[3]/π is the cosine-weighted sky visibility at the point.
 *  9. weight = W; reserved is stored as zeros.
 * A point's record does not depend on which points share its call.  The contract covers finite probe records: a non-finite
 * coefficient of a valid probe, or a point so far off that step 5 overflows, may put a NaN into the sums; its sign and payload are
 * not specified.
 * rm_light_grid_irradiance refuses, in this order and all but the last before any HIP call: RM_ERR_INVALID_ARGUMENT: numPoints < 0;
 * null dims, origin or step; a dimension below 2 or above RM_MAX_LIGHT_GRID_DIM; dims[0]·dims[1]·dims[2] above
 * RM_MAX_LIGHT_GRID_PROBES; a non-finite origin component; a step component that is not finite or not greater than 0; flag bits
 * other than RM_LIGHT_GRID_FACING.  Then numPoints == 0: RM_OK, nothing read or written.  Then RM_ERR_INVALID_ARGUMENT: a null or
 * misaligned d_probes, d_points, d_normals or d_out (16 bytes); last, an array that is not device memory.
 * Schedule: ONE launch, one lane per point, 256-lane workgroups.  A lane reads its two 16-byte inputs, the hits word of each of its
 * eight corners, then the nine float4 of every valid corner, keeps four sums per corner and stores the record as two 16-byte
 * stores.  This is not a render launch: like the field queries, rm_debug_last_path() keeps its value, rm_set_timing does not time
 * it, no scene block, tuner or workspace state is touched, and nothing is allocated.
 * Added without a change of RM_ABI_VERSION (new symbols and nothing else): bindings detect them by symbol lookup.
 */
typedef struct RmGridLight { float e[4]; float weight; int32_t probes; int32_t reserved[2]; } RmGridLight;   /* 32 bytes */
#define RM_LIGHT_GRID_FACING 1u
#define RM_MAX_LIGHT_GRID_DIM    1024
#define RM_MAX_LIGHT_GRID_PROBES (1 << 24)
int rm_light_grid_irradiance(const RmLightProbe *d_probes, const int dims[3], const float origin[3], const float step[3],
                             const float *d_points /* float4 each, w not read */, const float *d_normals /* float4 each, w not read */,
                             int numPoints, uint32_t flags, RmGridLight *d_out, void *stream);
/*
 * rm_light_probes_depth, rm_probe_depth_weights, rm_light_grid_irradiance_visible — a visibility term per probe, so that a light
 * grid does not leak through walls: DDGI's depth moments (Majercik et al. 2019).  A trilinear blend takes light from probes on the
 * far side of an occluder, and RM_LIGHT_GRID_FACING only removes probes behind the SURFACE.  Per probe an 8×8 octahedral map holds
 * the mean distance to the scene and the mean squared distance per direction; the lookup weighs every corner by a Chebyshev bound
 * of the chance that the point is seen from the probe.
 *
 * The map.  Texel x = tx + 8·ty (tx, ty = 0 … 7) has the centre direction c_x = octDecode(((tx + 0.5)/8)·2 − 1, ((ty + 0.5)/8)·2 − 1),
 * octDecode(u, v) = normalize(X, Y, Z) with Z = 1 − |u| − |v| and (X, Y) = (u, v) for Z >= 0, ((1 − |v|)·sign(u), (1 − |u|)·sign(v))
 * for Z < 0, sign(±0) = +1: the unit octahedron |x| + |y| + |z| = 1 unfolded onto [−1, 1]², upper half in the inner diamond.
 *
 * rm_probe_depth_weights(dirs, numDirs, numSets, sharpness, out), host only (no HIP call): out is numSets·numDirs rows of
 * RM_PROBE_DEPTH_TEXELS floats, row s·numDirs + k the weights of table row k of set s on the 64 texels.  In binary64 from the
 * binary32 dir: d = dir/|dir| with |dir| = sqrt((x·x + y·y) + z·z), dot = (c_x.x·d.x + c_x.y·d.y) + c_x.z·d.z, raw = pow(max(0, dot),
 * sharpness) (pow(0, 0) = 1), sum = Σ raw over the set's rows in ascending k, out = raw/sum rounded ONCE to binary32.  A texel whose
 * sum is 0 (few directions, a high sharpness) gives the row with the largest dot weight 1 and the others +0, ties to the lowest k:
 * no texel is ever empty.  A row whose dir is invalid by rm_shade_rays' rule gets +0 on every texel and takes no part in sums or
 * ties.  It refuses numDirs and numSets as rm_sphere_directions does, then a null dirs or out, then a sharpness that is not finite
 * or is below 0.
 *
 * rm_light_probes_depth — the bake, ONE launch.  d_positions, d_dirs, numDirs, numSets: as rm_light_probes takes them, the same
 * table (the basis of a row is not read); d_weights: numSets·numDirs rows of 64 floats in device memory, 16-byte aligned —
 * rm_probe_depth_weights' or the caller's own; d_out: numProbes RmProbeDepth in device memory, 16-byte aligned.  Lights and
 * resources are no arguments: a march reads no material.  Asynchronous on `stream`.
 * Definition, bit for bit.  Probe i uses rows (i mod numSets)·numDirs + k, for k = 0 … numDirs − 1.  r_k is the t that
 * rm_trace_rays(RM_TRACE_CLOSEST | RM_TRACE_NO_NORMAL) stores for the ray origin = position_i, dir = row.dir (used as given),
 * tMax = maxDistance: the hit's t, or maxDistance on a miss.  A row whose dir is invalid gives r_k = +0 and evaluates nothing.  Per
 * texel x: moments[x][0] = T_k(w[k][x]·r_k) and moments[x][1] = T_k(w[k][x]·(r_k·r_k)), every product ONE binary32 multiplication,
 * unfused, T the pairwise tree of rm_light_probes over k, level by level: s[m] = s[2m] + s[2m + 1].  A probe with a non-finite
 * position stores 512 bytes of zeros and evaluates nothing.  A probe's record does not depend on which probes share its call.  The
 * contract covers finite weights: a non-finite one may put a NaN into the sums; its sign and payload are not specified.
 * It refuses in rm_light_probes' order with maxDistance in the place of far, all but the last before any HIP call:
 * RM_ERR_INVALID_ARGUMENT: numProbes < 0; numDirs not a power of two in 1 … RM_MAX_PROBE_DIRS; numSets below 1 or numSets·numDirs
 * above RM_MAX_PROBE_TABLE.  Then numProbes == 0: RM_OK.  Then RM_ERR_INVALID_ARGUMENT: numProbes·numDirs above INT_MAX; null g or s,
 * a null table with a positive count or a negative count; maxDistance NaN, infinite or not greater than 0; RM_ERR_UNSUPPORTED:
 * RM_FEAT_TERRAIN, RM_FEAT_CLOUD or RM_FEAT_SEA, g->isTwoD; then rm_trace_rays' checks of the object table;
 * RM_ERR_INVALID_ARGUMENT: a null or misaligned d_positions, d_dirs, d_weights or d_out (16 bytes); an array that is not device memory.
 * Schedule: ONE launch of the depth kernel of the table's march class (the table walk, the general Mandelbulb, its plain form;
 * rm_debug_last_path() = 22, rm_debug_last_split() = 0), 256-lane workgroups.  The march is rm_light_probes' flattening: lane mod
 * numDirs is the row, 64 / numDirs probes per wave up to 64 directions, passes of 64 above.  Then the wave leaves its 64 (r, r·r) in
 * LDS and lane x becomes texel x: it reads row k's weights — one 256-byte line per row for the wave —, forms the two leaves and folds
 * the leaves of the pass in tree order by itself; a serial walk adds the same operands in the same pairs as the tree, so it has
 * the tree's words.  The passes of a probe join with one pending pair per level and lane.  A record is 512 contiguous bytes of one
 * wave.  One slot of the batch ring of scene blocks; no tuner, tile-order or workspace state is read or changed, nothing is allocated.
 *
 * rm_light_grid_irradiance_visible — the lookup, ONE launch, one lane per point: rm_light_grid_irradiance's arguments with d_depth —
 * the grid's RmProbeDepth records, index as d_probes — behind d_probes and normalBias behind flags.  Its steps 1 to 9 with one step
 * between 5 and 6; binary32, unfused, division and sqrt correctly rounded (rm_light_grid.h is this text in C++).
 *  5a. Once per point q = p + normalBias·n per component, one multiplication and one addition.  Per valid corner: v = q −
 *      probePosition per component, r = sqrt((vx·vx + vy·vy) + vz·vz).  r == 0 gives vis = 1 and no depth word is read.  Otherwise
 *      l1 = (|vx| + |vy|) + |vz|, (ox, oy) = (vx/l1, vy/l1), and for vz < 0 the fold (ox, oy) = ((1 − |oy|)·sign(ox), (1 − |ox|)·sign(oy))
 *      of the unfolded pair, sign(±0) = +1.  Per axis u_a = o_a·4 + 3.5 clamped to [0, 7] (a u_a not greater than 0 becomes +0),
 *      i_a = min((int)floor(u_a), 6), f_a = u_a − (float)i_a.  With a, b, c, d the texels (ix, iy), (ix + 1, iy), (ix, iy + 1),
 *      (ix + 1, iy + 1): m = (a·(1 − fx) + b·fx)·(1 − fy) + (c·(1 − fx) + d·fx)·fy on moments[·][0], m2 the same on moments[·][1].
 *      The blend clamps at the map's edge: the octahedral wrap is NOT followed, directions near the z = 0 seam blend with the edge
 *      texel alone.  r <= m gives vis = 1.  Otherwise var = |m2 − m·m|, dd = r − m, den = var + dd·dd, c = var/den (1 for den == 0),
 *      vis = max((c·c)·c, RM_LIGHT_GRID_VIS_FLOOR).  w_c = (t_c·face)·vis.  Of an invalid probe neither sh nor depth words are read.
 * Depth records whose every mean is at least every r give vis = 1 exactly, and x·1.0f is x: the record then equals
 * rm_light_grid_irradiance's IN EVERY WORD.  The floor keeps a point that no probe sees lit by all of them rather than black.
 * It refuses as rm_light_grid_irradiance does, a non-finite normalBias behind the step, d_depth beside d_probes.  Not a render
 * launch: rm_debug_last_path() keeps its value, no scene block, tuner or workspace state is touched, nothing is allocated.
 * Added without a change of RM_ABI_VERSION (new symbols and nothing else): bindings detect them by symbol lookup.
 */
#define RM_PROBE_DEPTH_TEXELS 64
typedef struct RmProbeDepth { float moments[64][2]; } RmProbeDepth;   /* 512 bytes: mean, mean of squares per texel */
#define RM_LIGHT_GRID_VIS_FLOOR 1.0e-6f
int rm_probe_depth_weights(const RmProbeDir *dirs /* host */, int numDirs, int numSets, float sharpness, float *out /* host */);
int rm_light_probes_depth(const float *d_positions /* float4 each, w not read */, int numProbes, const RmProbeDir *d_dirs,
                          const float *d_weights, int numDirs, int numSets, float maxDistance,
                          const RmObject *objs, int numObjects, const RmGlobals *g, const RmSettings *s,
                          RmProbeDepth *d_out, void *stream);
int rm_light_grid_irradiance_visible(const RmLightProbe *d_probes, const RmProbeDepth *d_depth, const int dims[3],
                                     const float origin[3], const float step[3],
                                     const float *d_points /* float4 each, w not read */, const float *d_normals /* float4 each, w not read */,
                                     int numPoints, uint32_t flags, float normalBias, RmGridLight *d_out, void *stream);
/*
 * rm_shade_rays_indirect, rm_light_probes_indirect — the diffuse term of a light grid at the hit of a shaded ray, computed inside
 * the shading kernel: what a multi-bounce bake feeds back (DDGI: each probe ray adds albedo · E_grid(hit, normal) / π at its hit) and
 * what a frame lit by a grid adds per pixel.  Inside the kernel the hit point, the bumped normal, getDiffuse's texture blend and the
 * march's orbit trap all exist; no other entry hands out the last two.
 *
 * The grid is ONE host struct, RmLightGridRef, copied before the call returns: d_probes and dims, origin, step as
 * rm_light_grid_irradiance takes them; d_depth the grid's RmProbeDepth records or NULL; flags and normalBias as
 * rm_light_grid_irradiance_visible takes them (normalBias is not read by the lookup without d_depth, but is checked); strength.
 *
 * The term, bit for bit, for a ray (ro, rd).  Every operation is ONE binary32 operation as written, unfused (rm_indirect.h is the
 * arithmetic behind the hit in C++).
 *   colour is what rm_shade_rays stores for the ray, in every word.
 *   (n, t, p, obj) is what rm_trace_rays(RM_TRACE_CLOSEST) stores for the same ray with tMax = far.
 *   NO TERM — colour's words are stored unchanged and no addition is performed, not even of +0 — where the ray is invalid (zeros, as
 *   rm_shade_rays), where the primary march misses, where the hit object isEmissive, and where probes <= 0 in the grid record below.
 *   Otherwise e is RmGridLight.e of the record that rm_light_grid_irradiance_visible stores at (p, n) with flags and normalBias
 *   where d_depth is not NULL, rm_light_grid_irradiance's where it is NULL, word for word;
 *     ec[ch] = e[ch] > 0 ? e[ch] : +0          (ringing of the clamped-cosine lobe, −0 and NaN become +0)
 *     k      = strength · RM_INV_PI            (one multiplication, on the host)
 *     dif    = getDiffuse at p for the hit object, the value render() puts into mat.dif: kd·cDiffuse, or its blend with the texture
 *     x[ch]  = (dif[ch] · ec[ch]) · k
 *   and the palette multiplies the term as it multiplies Phong: Mandelbulb ind = c · (x · 8) with
 *   c = bulbTrapColor(trap.y, trap.z, trap.w); Menger sponge ind = c · x with the cosine palette of trap.z; every other type ind = x.
 *   trap is the primary march's; in a table with a fractal behind the hit one, UB3's rule (the trap of the last fractal evaluated)
 *   holds here as in render().
 *     out.rgb = colour.rgb + ind, one addition per channel; alpha is colour's.
 * The term lights the PRIMARY HIT ONLY: reflection and refraction bounces get none, and ambient occlusion does not multiply it.
 * There is no bright output.  The result of a ray does not depend on the rays it shares a call with.
 *
 * rm_shade_rays_indirect — ONE launch, one lane per ray: rm_shade_rays' arguments without d_bright, `grid` behind res; rm_shade_rays'
 * classes and staging (rm_debug_last_path() = 23, rm_debug_last_split() = 0).  It refuses in this order, all but the last before any
 * HIP call: rm_shade_rays' own refusals up to and with the alignment of d_rays and d_rgba (numRays == 0 is RM_OK there); then
 * RM_ERR_INVALID_ARGUMENT: a null grid; a dimension below 2 or above RM_MAX_LIGHT_GRID_DIM; more than RM_MAX_LIGHT_GRID_PROBES probes;
 * a non-finite origin component; a step component that is not finite or not greater than 0; a non-finite normalBias; flag bits other
 * than RM_LIGHT_GRID_FACING; a null d_probes (d_depth may be NULL); a misaligned d_probes or d_depth (16 bytes); a non-finite
 * strength; last, an array that is not device memory (d_rays, the resources' pixels and d_rgba, d_probes, d_depth).  RM_FEAT_TERRAIN,
 * RM_FEAT_CLOUD and RM_FEAT_SEA are RM_ERR_UNSUPPORTED, as for rm_shade_rays.
 *
 * rm_light_probes_indirect — ONE launch: rm_light_probes with every ray's colour replaced by out.rgb above; the hit flag, the leaves,
 * the tree, the flattening and the multi-pass fold are unchanged, so a record equals rm_shade_rays_indirect on the numProbes·numDirs
 * rays through rm_light_probes' tree in every word (rm_debug_last_path() = 24).  rm_light_probes' arguments with `grid` behind res.
 * It refuses rm_light_probes' own up to and with the alignment of its arrays (numProbes == 0 is RM_OK there), then the grid and the
 * strength as above, then RM_ERR_INVALID_ARGUMENT: [d_out, d_out + numProbes·160) overlaps the grid's probe records — a bake must
 * not read the grid it writes; ping-pong two buffers —, last the device-memory checks.
 * Schedule: shade_rays_kernel's and light_probes_kernel's, with the grid (64 bytes) by value in the kernel's arguments.  Behind its
 * primary hit a lane reads its cell's eight hits words, the nine float4 of every valid corner and, with d_depth, four texels of each.
 * One slot of the batch ring of scene blocks; no tuner, tile-order or workspace state is read or changed, nothing is allocated.
 * Added without a change of RM_ABI_VERSION (new symbols and nothing else): bindings detect them by symbol lookup.
 */
#define RM_INV_PI ((float)0.31830988618379067)   /* 1/π in binary64, rounded once to binary32 */
typedef struct RmLightGridRef {
  const RmLightProbe *d_probes; const RmProbeDepth *d_depth /* may be NULL */;
  int dims[3]; float origin[3]; float step[3];
  float strength; uint32_t flags; float normalBias;
} RmLightGridRef;   /* 64 bytes */
int rm_shade_rays_indirect(const RmRay *d_rays, int numRays, float far,
                           const RmObject *objs, int numObjects, const RmLight *lights, int numLights,
                           const RmGlobals *g, const RmSettings *s, const RmResources *res /* may be NULL */,
                           const RmLightGridRef *grid, float *d_rgba, void *stream);
int rm_light_probes_indirect(const float *d_positions /* float4 each, w not read */, int numProbes,
                             const RmProbeDir *d_dirs, int numDirs, int numSets, float far,
                             const RmObject *objs, int numObjects, const RmLight *lights, int numLights,
                             const RmGlobals *g, const RmSettings *s, const RmResources *res /* may be NULL */,
                             const RmLightGridRef *grid, RmLightProbe *d_out, void *stream);
/*
 * rm_trace_rays_layers — rm_trace_rays THROUGH terrain and sea: the closest VISIBLE SURFACE along each ray, by the rules main
 * applies to its own rays.  For keeping a fly-through camera above the terrain, and for picking on a landscape.  The arguments are
 * rm_trace_rays' with imageWidth (as above, >= 1 in every call) behind numRays.
 * Definition, bit for bit:
 *   res = raymarch(origin, dir, tMax, OUTSIDE), rm_trace_rays' closest hit; d0 = hit ? res.d : tMax
 *   RM_FEAT_SEA: the geometric part of seaRender(origin, dir, maxT = d0) (frag:2284-2291, 2252-2282): seaHit, t_s, p_s;
 *     d1 = seaHit ? t_s : d0
 *   RM_FEAT_TERRAIN: the geometric part of terrainRender(origin, dir, maxT = d1) (frag:2128-2135, 2060-2090; tmin = 15):
 *     terrainHit, t_t
 * Terrain hit: objectId = RM_HIT_TERRAIN (−4), t = t_t, position = dir·t_t + origin in terrainRender's fused form, normal =
 * terrainNormal(position.x, position.z) (frag:2106-2111).  That is the SURFACE's own normal, not the fbm-perturbed `nor` the
 * terrain's lighting builds from it (frag:2141): a collision response needs the surface.
 * Sea hit and no terrain hit: objectId = RM_HIT_SEA (−3), t = t_s, position = p_s as seaMapHeight leaves it, normal =
 * getSeaNormal(p_s, (dot(d, d)·0.1) / imageWidth) with d = p_s − origin (frag:2243-2250, 2296): the shader's normal.
 * Neither: the object hit, or the miss, exactly as rm_trace_rays stores it, bump included.
 * RM_FEAT_CLOUD is accepted and ignored: a volume has no closest hit.  RM_TRACE_NO_NORMAL works as before: objectId and t only,
 * zeros elsewhere, no normal taps.  RM_TRACE_OCCLUSION together with a layer bit is RM_ERR_UNSUPPORTED: the objects' shadow march
 * does not see the layers; without a layer bit it is rm_trace_rays' occlusion.  With no layer bit every mode gives rm_trace_rays'
 * output in every bit (the same kernels run).  Per-ray tMax and the invalid-ray rule stay; the result of a ray does not depend on
 * which other rays share its call.  No resources are read: the sea's geometry does not touch the noise texture.
 * numRays == 0: RM_OK.  Otherwise rm_trace_rays' checks in its order, all but the last before any HIP call, with two differences:
 * imageWidth < 1 is RM_ERR_INVALID_ARGUMENT right after the mode bits, and in place of the refusal of the layers stands the refusal
 * of RM_TRACE_OCCLUSION with one.
 * Schedule: ONE launch, one lane per ray (rm_debug_last_path() = 15, rm_debug_last_split() = 0): with RM_FEAT_SEA or
 * RM_FEAT_TERRAIN the layers' trace kernel of the table's march class, otherwise rm_trace_rays' kernel.  One slot of the batch ring
 * of scene blocks; no tuner, tile-order or workspace state is read or changed.  With rm_set_timing(1) one launch, all stage 1.
 * Added without a change of RM_ABI_VERSION (new symbols and nothing else): bindings detect them by symbol lookup.
 */
#define RM_HIT_SEA (-3)
#define RM_HIT_TERRAIN (-4)
int rm_trace_rays_layers(const RmRay *d_rays, int numRays, int imageWidth, const RmObject *objs, int numObjects, const RmGlobals *g,
                         const RmSettings *s, unsigned mode, RmRayHit *d_hits, void *stream);

/*
 * rm_rays_order — a COHERENCE ORDERING of an RmRay array, on the device (no reference counterpart).  rm_trace_rays, rm_shade_rays
 * and their _layers twins run one lane per ray, 64 consecutive rays per wave, and a wave costs what its longest ray costs: rays that
 * come in no order — secondary and ambient-occlusion rays from hit points, light probes, line-of-sight queries, rays read back from
 * another tracer — pay several times what the same rays cost in the order of a picture's 8×8 tiles.  This entry sorts them so that
 * the rays of a wave start close together and go the same way; rm_rays_restore puts results back in the caller's order.  Since the
 * result of a ray does not depend on which other rays share its call, sorting changes no result bit.
 * d_rays: numRays RmRay; d_order: numRays int32, required; d_sorted (may be NULL): numRays RmRay; d_keys (may be NULL): numRays
 * uint64; all device memory.  Asynchronous on `stream`.
 * Definition, bit for bit (raymarcher_amd/csrc/rm_ray_key.h is the same text as code).  All arithmetic is binary32, round to nearest
 * even, denormals kept, nothing fused, `/` correctly rounded.
 * VALID for ordering: every component of origin and dir is finite and dir is not all zeros.  tMax and `reserved` are NOT read: a ray
 * that only rm_trace_rays calls invalid, by its tMax, is ordered by its geometry.
 * Direction coordinates of a valid ray, an octahedral map: s = (|dx| + |dy|) + |dz|; px = dx / s; py = dy / s; if dz < 0: u = (1 −
 * |py|) · sgn(px) and v = (1 − |px|) · sgn(py), sgn being −1 where the sign bit is set and +1 otherwise; else u = px, v = py.  Where s
 * overflows to +inf, px = py = 0: that is the definition, and harmless.
 * Bounds: lo and hi of each of the five coordinates ox, oy, oz, u, v over the valid rays of the call — an exact minimum and maximum,
 * so they do not depend on an order.  Which of −0 and +0 becomes a bound where both occur changes no key.
 * Quantise x to b bits: 0 unless hi > lo; else t = (x − lo) / (hi − lo), three rounded operations, and q = t >= 1 ? 2^b − 1 : (t > 0
 * ? (uint)(t · 2^b) : 0); a NaN t (inf / inf) gives 0.
 * Key, with originBits in 0 … 10 and dirBits in 0 … 11: morton3(q_ox, q_oy, q_oz) << (2·dirBits) | morton2(q_u, q_v), x the lowest
 * bit of each origin triple and u the lowest bit of each direction pair.  A ray that is not valid gets 1 << (3·originBits +
 * 2·dirBits), above every valid key: such rays end together in the last waves.
 * Order: the STABLE ascending sort of the keys.  d_order[k] = the input index of the ray at sorted position k; equal keys keep
 * their input order.  d_sorted[k] = d_rays[d_order[k]], all 32 bytes verbatim, tMax and `reserved` included.  d_keys receives the
 * keys in INPUT order (for callers who merge orderings).  Every output holds the same bits whichever of the others are NULL.
 * In this order, and all but the last before any HIP call: RM_ERR_INVALID_ARGUMENT: numRays < 0; originBits or dirBits out of
 * range.  Then numRays == 0: RM_OK, nothing read or written.  RM_ERR_INVALID_ARGUMENT: null d_rays or d_order; a misaligned pointer
 * (16 bytes for d_rays and d_sorted, 8 for d_keys, 4 for d_order); d_sorted == d_rays; an array that is not device memory.
 * Schedule: the bounds (per workgroup: lanes, the wave, LDS; one partial per workgroup, then a one-workgroup merge — no float
 * atomic), the keys, then a least-significant-digit radix sort of (key, index) pairs, 8 bits per pass over the 3·originBits +
 * 2·dirBits + 1 key bits: per pass a histogram per tile of RM_RAYS_ORDER_TILE keys, a scan (a launch of its own) and a stable
 * scatter; a pass whose digit is the same in every key is skipped (with ONE origin for all rays every origin digit is); then the
 * gather of d_sorted.  No kernel waits for another workgroup.  Workspace, grow-only and per (device, stream): 24 B per ray (two key
 * and two index buffers) + 1 KB per tile + 24 KB; rm_set_workspace_limit applies (over a set limit, or when the allocation fails:
 * RM_ERR_DEVICE, as rm_sdf_blocks_select has it, and HIP's error state is left clean), rm_release_workspaces frees it.  Not a render
 * launch: rm_debug_last_path() and rm_debug_last_split() keep their values and rm_set_timing does not time it.
 * Added without a change of RM_ABI_VERSION (new symbols and nothing else): bindings detect them by symbol lookup.
 */
#define RM_RAYS_ORDER_TILE 2048 /* keys per workgroup of the sort */
int rm_rays_order(const RmRay *d_rays, int numRays, int originBits, int dirBits, int32_t *d_order, RmRay *d_sorted /* may be NULL */,
                  uint64_t *d_keys /* may be NULL */, void *stream);
/*
 * rm_rays_restore — the inverse of an ordering, for results: d_out[d_order[k]] = d_rows[k] for k < numRows.  rowBytes is 16 (a float4
 * colour of rm_shade_rays) or 32 (RmRayHit, RmSurfacePoint).  An entry of d_order outside [0, numRows) is skipped and that row is
 * not written: the order is device data, the host cannot refuse it.  With a permutation — rm_rays_order's d_order — every row of
 * d_out is written once.  Asynchronous on `stream`; one launch, one lane per 16 bytes; no workspace; not a render launch.
 * In this order, and all but the last before any HIP call: RM_ERR_INVALID_ARGUMENT: numRows < 0; rowBytes other than 16 or 32.  Then
 * numRows == 0: RM_OK, nothing read or written.  RM_ERR_INVALID_ARGUMENT: null d_rows, d_order or d_out; a misaligned pointer (16
 * bytes for d_rows and d_out, 4 for d_order); d_out == d_rows; an array that is not device memory.
 */
int rm_rays_restore(const void *d_rows, const int32_t *d_order, int numRows, int rowBytes, void *d_out, void *stream);

/*
 * rm_sdf_grid — WHERE the surface is: sdScene on a dense lattice (no reference counterpart: the shader evaluates its distance
 * function only along its own rays).  For a 3-D texture of the field (physics, particles, a caller's own ambient occlusion, keeping
 * a camera out of the scene without a ray) and as the input of rm_sdf_mesh.  d_dist: nx·ny·nz floats in device memory, d_objectId
 * (may be NULL): as many int32; the object table, g, s, origin and step are host memory, copied before return.  Asynchronous on
 * `stream`.
 * Definition, bit for bit.  Lattice point (i, j, k) is p.x = origin[0] + (float)i · step[0], and likewise y and z: one binary32
 * multiply, then one binary32 add, never fused (NumPy: origin + np.arange(n, dtype=float32) · step).  d_dist[(k·ny + j)·nx + i] — x
 * fastest, a 64-bit index — is the minD that sdScene(p) returns (frag:1406-1430), d_objectId at the same index its minObjIdx (−1
 * for an empty table): exactly what rm_probe_sdscene stores in components 0 and 1 for that point.  Nothing is written to a NULL
 * d_objectId, and d_dist is the same bits without it.  The sign is the scene's: negative inside an object whose distance function is
 * signed; a Mandelbulb's estimate is 0 or above, and below 0.001 — the march's hit threshold — only close to its surface.
 * Of RmSettings the call reads fractalIters, mengerLevels and the power-8 form bit; of RmGlobals power, juliaSeed and iTime.  Lights,
 * samplers, cameras and the march's settings play no part.  The value of a point does not depend on which other points share its
 * call.
 * In this order, and all but the last before any HIP call: RM_ERR_INVALID_ARGUMENT: null g, s, origin or step, a null table with a
 * positive count or a negative count, an origin component that is not finite, a step component that is not finite or not greater
 * than 0, a dimension below 1 or above RM_MAX_LATTICE_DIM, more than INT_MAX points; RM_ERR_UNSUPPORTED: RM_FEAT_TERRAIN,
 * RM_FEAT_CLOUD or RM_FEAT_SEA in the settings (the lattice holds the object table only), g->isTwoD; rm_trace_rays' checks of the
 * table: RM_ERR_CAPACITY beyond RM_MAX_OBJECTS, a negative loop bound, RM_ERR_UNSUPPORTED for a CUSTOM or unknown object type;
 * RM_ERR_INVALID_ARGUMENT: a null d_dist, an output that is not device memory.  There is no empty lattice: every dimension is at
 * least 1.
 * Schedule: ONE launch, one lane per lattice point, of the grid kernel of the table's march class — the table walk, the general
 * Mandelbulb, or its plain form where rm_debug_bulb_plain says 1 (rm_debug_last_path() = 16, rm_debug_last_split() = 0).  A wave
 * owns a brick of 4×4×4 points, so the lanes of a wave are neighbours in space and a Mandelbulb's iteration counts differ as little
 * as they can; a workgroup is four bricks along x.  It uses one slot of the batch ring of scene blocks and neither reads nor changes
 * the per-stream tuner and tile-order state of single-frame renders, and no library workspace.  With rm_set_timing(1) it counts as
 * one launch, all stage 1.
 * Added without a change of RM_ABI_VERSION (new symbols and nothing else): bindings detect them by symbol lookup.
 */
#define RM_MAX_LATTICE_DIM 4096
int rm_sdf_grid(const RmObject *objs, int numObjects, const RmGlobals *g, const RmSettings *s, const float origin[3],
                const float step[3], int nx, int ny, int nz, float *d_dist, int32_t *d_objectId /* may be NULL */, void *stream);
/*
 * rm_sdf_mesh — a QUAD MESH of the surface {v = iso} of any lattice of floats, by naive surface nets: one vertex per cell the surface
 * passes through, one quad per lattice edge it crosses (no reference counterpart).  For the Mandelbulb or the sponge as a mesh: 3-D
 * printing, a DCC tool, collision geometry.  d_dist: nx·ny·nz floats in rm_sdf_grid's layout, from rm_sdf_grid or from anywhere else
 * (smoothed, clipped, two lattices combined); d_objectId (may be NULL): as many int32.  Outputs, all device memory: d_vertices, 4
 * floats per vertex; d_vertexObject (may be NULL), one int32 per vertex; d_quads, 4 vertex numbers per quad; d_counts, 2 words.
 * origin and step are host memory, copied before return.  Asynchronous on `stream`; no host synchronisation and no read-back.
 * Definition, bit for bit.  inside(v) = v < iso; a NaN is outside.
 * Cells: cell (i, j, k), 0 <= i < nx − 1 and so on, has the corners c = cx + 2·cy + 4·cz at lattice point (i + cx, j + cy, k + cz)
 * and twelve edges in this order: the x-edges (0,1) (2,3) (4,5) (6,7), the y-edges (0,2) (1,3) (4,6) (5,7), the z-edges (0,4) (1,5)
 * (2,6) (3,7).  A cell is active iff its corners are neither all inside nor all outside.
 * Vertex of an active cell: acc = (+0, +0, +0), n = 0; for each edge (a, b), in order, whose ends differ in inside: t = (iso − v_a) /
 * (v_b − v_a) — one subtraction each, one IEEE division —, t = 0.5f unless (t >= 0 && t <= 1); the crossing is corner a's (cx, cy,
 * cz) as floats with the edge's axis component replaced by t; acc += crossing, component by component; ++n.  local = acc · (1.0f /
 * (float)n); vertex.x = origin[0] + ((float)i + local.x) · step[0] — add, multiply, add, unfused —, y and z alike, vertex.w = 0.
 * d_vertexObject, where it and d_objectId are both given, is the id at the cell's first inside corner in corner order; −1 without
 * d_objectId.
 * Vertex order: the cells' linear order (k·(ny − 1) + j)·(nx − 1) + i; a vertex's number is the count of active cells before its own.
 * Quads: the lattice edge from P = (i, j, k) to P + e_axis gives one quad iff its ends differ in inside and it is interior in the
 * other two axes (x: 1 <= j <= ny − 2 and 1 <= k <= nz − 2), over the four cells around it — x: (i,j−1,k−1) (i,j,k−1) (i,j,k)
 * (i,j−1,k); y: (i−1,j,k−1) (i−1,j,k) (i,j,k) (i,j,k−1); z: (i−1,j−1,k) (i,j−1,k) (i,j,k) (i−1,j,k) — in that order when P is inside,
 * as (c0, c3, c2, c1) otherwise: the normal points to the outside.  All four cells are active.  A surface that leaves the lattice is
 * left open there.  Quad order: by P's lattice index (k·ny + j)·nx + i, then by axis x, y, z.
 * Counts and capacity: d_counts[0] and d_counts[1] always receive the FULL number of vertices and quads (the quads' saturates at
 * 2^32 − 1); only vertices numbered below maxVertices and quads numbered below maxQuads are stored, so a stored quad may name a
 * vertex that was not: compare the counts with the capacities.  maxVertices = maxQuads = 0 with null outputs is the counting call.
 * A lattice with a dimension of 1 has no cell: RM_OK, both counts 0.
 * In this order, and all but the last before any HIP call, RM_ERR_INVALID_ARGUMENT: null origin or step, an origin component that is
 * not finite, a step component that is not finite or not greater than 0, a dimension below 1 or above RM_MAX_LATTICE_DIM, more than
 * INT_MAX points (rm_sdf_grid's rules); iso not finite; a negative capacity; a null d_vertices or d_quads with its capacity above 0;
 * a null d_dist or d_counts; an array that is not device memory.
 * Schedule: a count of active cells and crossed edges per workgroup of 1024 lattice points, an exclusive scan of the counts that
 * also stores d_counts, then — unless both capacities are 0 — the vertices and each active cell's vertex number, and the quads from
 * those numbers: two launches for the counting call, up to four otherwise.  The numbers live in a grow-only workspace per (device,
 * stream) of 4 B per cell + 12 B per 1024 lattice points: rm_set_workspace_limit applies (a lattice over a set limit: RM_ERR_DEVICE),
 * rm_release_workspaces frees it.  Not a render launch: rm_debug_last_path() keeps its value and rm_set_timing does not time it.
 */
int rm_sdf_mesh(const float *d_dist, const int32_t *d_objectId /* may be NULL */, int nx, int ny, int nz, const float origin[3],
                const float step[3], float iso, int maxVertices, int maxQuads, float *d_vertices /* float4 each */,
                int32_t *d_vertexObject /* may be NULL */, int32_t *d_quads /* int4 each */, uint32_t *d_counts /* 2 words */,
                void *stream);

/*
 * Block-sparse lattices — rm_sdf_grid and rm_sdf_mesh beyond the dense lattice's limits (no reference counterpart).  A dense lattice
 * holds 4 B per point of distances, of ids and of vertex numbers and at most INT_MAX points, to find a surface that passes through a
 * few per cent of its cells.  The three entry points below keep only the blocks the surface passes through.
 * Terms.  A BLOCK is 8×8×8 cells: 9×9×9 lattice points.  The VIRTUAL LATTICE has mx × my × mz blocks, each dimension 1 …
 * RM_MAX_LATTICE_BLOCKS, so 8·m + 1 points per axis; lattice point (i, j, k) is origin + (float)i · step per axis, rm_sdf_grid's
 * formula exactly, and there is no INT_MAX rule on the number of points.  A BLOCK LIST is numBlocks entries of int32[4], (bi, bj, bk,
 * unused), in device memory, numBlocks 0 … RM_MAX_BLOCK_LIST (2^31 cells: vertex numbers fit 32 bits).  An entry is VOID if a
 * coordinate lies outside [0, m) or an earlier entry has the same coordinates — of equal entries the first counts.  Lists are device
 * data, which the host cannot refuse: void entries are skipped everywhere.
 * All three: asynchronous on `stream`; the table, g, s, origin and step are host memory, copied before return; added without a change
 * of RM_ABI_VERSION (new symbols and nothing else): bindings detect them by symbol lookup.
 */
#define RM_MAX_LATTICE_BLOCKS 512
#define RM_MAX_BLOCK_LIST (1 << 22)
/*
 * rm_sdf_blocks_select — WHICH blocks hold surface.  Block (bi, bj, bk) is ACTIVE iff inside(v) = v < iso (a NaN is outside) is not
 * the same for all 729 of its lattice points, v being sdScene(p).minD in rm_sdf_grid's bits.  That is equivalent to "one of its 512
 * cells is active in rm_sdf_mesh's sense" (a cell is active iff its eight corners differ in inside; the block's points are connected
 * through its cells' edges, so two points that differ have a cell between them whose corners differ) — decided exactly, from the
 * block's own points, with no Lipschitz bound, which the estimators do not honour.  The active blocks are listed in their linear order
 * (bk·my + bj)·mx + bi, as (bi, bj, bk, 0).  d_count always receives the FULL number of active blocks; only the first maxBlocks
 * entries are stored.  maxBlocks = 0 with a null d_blocks is the counting call.  Nothing of the lattice is stored: every point is
 * evaluated once, in every block that has it, and only a flag per block is kept.
 * In this order, and all but the last before any HIP call: RM_ERR_INVALID_ARGUMENT: null g, s, origin or step, a null table with a
 * positive count or a negative count, an origin component that is not finite, a step component that is not finite or not greater
 * than 0, a block dimension below 1 or above RM_MAX_LATTICE_BLOCKS, iso not finite, a negative maxBlocks; RM_ERR_UNSUPPORTED:
 * RM_FEAT_TERRAIN, RM_FEAT_CLOUD or RM_FEAT_SEA in the settings, g->isTwoD; rm_trace_rays' checks of the table (rm_sdf_grid's);
 * RM_ERR_INVALID_ARGUMENT: a null d_count, a null d_blocks with maxBlocks above 0, an output that is not device memory.
 * Schedule: staging is rm_sdf_grid's.  One workgroup per block of the virtual lattice and one lane per point of it, in runs of 64 of
 * the block's x-fastest order: twelve waves, the evaluator of rm_sdf_grid's kernel of the table's march class; a lane outside the 729
 * points leaves before the evaluation, so a point's value does not depend on its wave.  Per block the waves' ballots of inside and of
 * !inside are ORed: active iff both are non-empty.  Then a count / scan / emit compaction of the flags in linear order
 * (rm_debug_last_path() = 18, rm_debug_last_split() = 0; with rm_set_timing(1) it counts as one launch, all stage 1).  Workspace, grow-
 * only per (device, stream), shared with the two entry points below: 4 B per block of the virtual lattice + 8 B per 1024 blocks;
 * rm_set_workspace_limit applies (a lattice over a set limit: RM_ERR_DEVICE), rm_release_workspaces frees it.
 */
int rm_sdf_blocks_select(const RmObject *objs, int numObjects, const RmGlobals *g, const RmSettings *s, const float origin[3],
                         const float step[3], int mx, int my, int mz, float iso, int maxBlocks, int32_t *d_blocks /* int4 each */,
                         uint32_t *d_count /* 1 word */, void *stream);
/*
 * rm_sdf_blocks_select_pruned — rm_sdf_blocks_select without the sweep over blocks far from the surface.  The surface passes through
 * under 1 % of the blocks of a large lattice; this entry evaluates the block corners first and the 729 points only of the blocks
 * the corners do not rule out.
 * Definition.  c(i, j, k), i in 0 … mx (j, k likewise), is sdScene(p).minD at lattice point (8i, 8j, 8k), in rm_sdf_grid's bits
 * (origin + (float)(8i) · step).  h = 4 · sqrt((sx·sx + sy·sy) + sz·sz), half a block's diagonal, every operation rounded to binary32
 * with no contraction and the square root correctly rounded (computed on the host); bOut = lipschitzOut · h and bIn = lipschitzIn ·
 * h, one rounded multiplication each; a NaN bound (0 · inf) discards nothing.  For a corner value c: d = c − iso, farOut = d > bOut,
 * farIn = d < −bIn; a NaN c is neither, a value exactly at a bound is not far.  A block is DISCARDED iff farOut holds at all eight of
 * its corners, or farIn holds at all eight; every other block is a CANDIDATE.  The list is the candidates that are ACTIVE by
 * rm_sdf_blocks_select's exact rule, decided from the block's own 729 points: the same linear order (bk·my + bj)·mx + bi, the same
 * rows (bi, bj, bk, 0).  d_count[0] receives the FULL number of listed blocks, as in rm_sdf_blocks_select, and maxBlocks = 0 with a
 * null d_blocks is the counting call; d_count[1] receives the number of candidates, saturated at 2^32 − 1.
 * Properties.  The list is a sub-sequence of rm_sdf_blocks_select's list.  With both constants +INFINITY the two lists and d_count[0]
 * are equal in every word.  They are also equal whenever every lattice point p of a block and every corner q of it satisfy v(p) ≥
 * v(q) − lipschitzOut·|p − q| on the outside, and the mirrored condition with lipschitzIn on the inside (|p − q| ≤ h for the nearest
 * corner, so a block with all corners far on one side has all 729 points on that side).  A true distance function honours this with
 * 1.  The Mandelbulb's estimate on the outside exceeds the distance near fine structure: measured on the headline bulb, 1 loses
 * nothing up to 2049 points per axis and 16 of a million blocks at 4097, 2 loses none (profiles/sdf_prune.md); the Python layer
 * passes 4.  The fractal estimators' interior honours no constant — the Mandelbulb's reports one value that is no distance, and a Julia
 * set has pockets of escaping points inside — so lipschitzIn = +INFINITY is what a caller who wants the exact list of a fractal
 * passes.  The rule is flat on purpose: a hierarchy of single probes fails on estimators that return a huge value at one point.
 * In this order, and all but the last before any HIP call: rm_sdf_blocks_select's refusals in its order, with one more between "iso
 * not finite" and "a negative maxBlocks": RM_ERR_INVALID_ARGUMENT for a lipschitzOut or lipschitzIn that is NaN or below 0
 * (+INFINITY and 0 are valid).
 * Schedule: staging is rm_sdf_grid's; asynchronous on `stream` with no host synchronisation inside the call.  (1) The corner lattice,
 * (mx + 1)(my + 1)(mz + 1) values, one lane per corner with the evaluator of rm_sdf_grid's kernel of the table's march class; a lane
 * past the last corner leaves before the evaluation, so a corner's value does not depend on its wave.  (2) One lane per block reads
 * its eight corners and writes the block's flag; count / scan / emit turn the flags into the list of candidates.  (3) Workgroups of
 * rm_sdf_blocks_select's shape loop over that list, whose length they read from device memory, and turn each candidate's flag into
 * its active flag; the grid is sized from the device's compute units.  (4) rm_sdf_blocks_select's compaction of the flags
 * (rm_debug_last_path() = 20, rm_debug_last_split() = 0; with rm_set_timing(1) it counts as one launch, all stage 1).  Workspace, the
 * one of rm_sdf_blocks_select: 4 B per corner + 8 B per block of the virtual lattice + 8 B per 1024 blocks, which is at most 12 B per
 * block of a lattice with many blocks per axis; rm_set_workspace_limit applies (a lattice over a set limit: RM_ERR_DEVICE),
 * rm_release_workspaces frees it.  Added without a change of RM_ABI_VERSION, as the entries around it.
 */
int rm_sdf_blocks_select_pruned(const RmObject *objs, int numObjects, const RmGlobals *g, const RmSettings *s, const float origin[3],
                                const float step[3], int mx, int my, int mz, float iso, float lipschitzOut, float lipschitzIn,
                                int maxBlocks, int32_t *d_blocks /* int4 each */, uint32_t *d_count /* 2 words */, void *stream);
/*
 * rm_sdf_grid_blocks — the lattice, stored only where listed.  Entry n owns floats [n·729, (n + 1)·729) of d_dist (and as many int32
 * of d_objectId, which may be NULL); its local point (a, b, c), each 0 … 8, is stored at (c·9 + b)·9 + a and holds the value at
 * lattice point (8·bi + a, 8·bj + b, 8·bk + c): the bits rm_sdf_grid stores for that point of the dense lattice.  Points on shared
 * faces are stored once per block that has them (1.42× the storage): blocks are independent, rm_sdf_mesh_blocks needs no
 * neighbour's values.  A void entry's slot is not written.  numBlocks = 0: RM_OK, nothing is read or written.
 * In this order, and all but the last before any HIP call: rm_sdf_blocks_select's refusals up to the block dimensions;
 * RM_ERR_INVALID_ARGUMENT: numBlocks below 0 or above RM_MAX_BLOCK_LIST; the layers, the 2-D mode and the table's checks as above;
 * then, with numBlocks above 0, RM_ERR_INVALID_ARGUMENT: a null d_blocks or d_dist, an array that is not device memory.
 * Schedule: staging is rm_sdf_grid's.  The block map of the list — 4 B per block of the virtual lattice in the workspace above, filled
 * by a scatter that keeps the smallest list position, which is what makes a later equal entry void — then ONE launch of
 * rm_sdf_blocks_select's evaluation kernel, a workgroup per entry (rm_debug_last_path() = 19, rm_debug_last_split() = 0).
 */
int rm_sdf_grid_blocks(const RmObject *objs, int numObjects, const RmGlobals *g, const RmSettings *s, const float origin[3],
                       const float step[3], int mx, int my, int mz, const int32_t *d_blocks /* int4 each */, int numBlocks,
                       float *d_dist /* numBlocks·729 */, int32_t *d_objectId /* may be NULL */, void *stream);
/*
 * rm_sdf_mesh_blocks — surface nets over a block list: rm_sdf_mesh's mesh of the virtual lattice, restricted to the listed blocks and
 * renumbered.  d_dist and d_objectId (may be NULL) in rm_sdf_grid_blocks' layout, from there or from anywhere else.
 * Cells and vertices: cell (i, j, k) of a block that is not void reads that block's own 729 values; its corner mask, whether it is
 * active, its vertex and its vertex object are rm_sdf_mesh's, computed with the GLOBAL cell index: a vertex has the bits rm_sdf_mesh
 * gives that cell on the dense lattice.  Vertex order: by list position of the block, then by local cell index (c·8 + b)·8 + a.
 * Quads: the lattice edge from P along an axis gives a quad under rm_sdf_mesh's rule — its ends differ in inside and it is interior in
 * the other two axes of the VIRTUAL lattice —, over the same four cells in the same orientation.  P is always corner 0 of an existing
 * cell, and that cell's block owns the edge.  The quad is stored iff all four cells lie in listed blocks that are not void.  Quad
 * order: by list position of the owning block, then by P's local index (c·8 + b)·8 + a, then by axis x, y, z.
 * d_counts: [0] the number of vertices and [1] the number of quads, FULL numbers whatever the capacities (the quads' saturates at
 * 2^32 − 1); [2] the number of OPEN vertices: active cells of listed blocks with at least one crossed, quad-giving edge one of whose
 * four cells lies in an unlisted block — the listed vertices of the dense mesh's quads that this list drops.  [2] = 0 means that every
 * component of the dense mesh that has a vertex in the list is complete; with the list of rm_sdf_blocks_select at the same iso it is 0
 * and the mesh is the whole dense mesh.  Capacities and the counting call (maxVertices = maxQuads = 0, null outputs) are rm_sdf_mesh's.
 * numBlocks = 0: RM_OK, all three counts 0.
 * Precondition: a point on a face that two listed blocks share holds equal bits in both, which rm_sdf_grid_blocks guarantees.
 * Otherwise the result is unspecified but memory-safe: stored vertex numbers stay below d_counts[0].
 * In this order, and all but the last before any HIP call, RM_ERR_INVALID_ARGUMENT: null origin or step, an origin component that is
 * not finite, a step component that is not finite or not greater than 0, a block dimension below 1 or above RM_MAX_LATTICE_BLOCKS;
 * iso not finite; numBlocks below 0 or above RM_MAX_BLOCK_LIST; a negative capacity; a null d_vertices or d_quads with its capacity
 * above 0; a null d_counts, or a null d_dist or d_blocks with numBlocks above 0; an array that is not device memory.
 * Schedule: the block map; one workgroup per list entry that counts its active cells, stored quads and open vertices and keeps the
 * 512-bit mask of its active cells; an exclusive scan over the entries that also stores d_counts; then — unless both capacities are 0
 * — one workgroup per entry for its vertices and quads, a cell's vertex number being its block's base + the mask's bits below the
 * cell: 68 B per entry in place of rm_sdf_mesh's 4 B per cell.  Workspace (the one above): 4 B per block of the virtual lattice + 88 B
 * per list entry.  Not a render launch: rm_debug_last_path() keeps its value and rm_set_timing does not time it.
 */
int rm_sdf_mesh_blocks(const float *d_dist, const int32_t *d_objectId /* may be NULL */, const int32_t *d_blocks /* int4 each */,
                       int numBlocks, int mx, int my, int mz, const float origin[3], const float step[3], float iso, int maxVertices,
                       int maxQuads, float *d_vertices /* float4 each */, int32_t *d_vertexObject /* may be NULL */,
                       int32_t *d_quads /* int4 each */, uint32_t *d_counts /* 3 words */, void *stream);

/*
 * Lattice queries — rm_sdf_sample, rm_sdf_sample_blocks, rm_sdf_trace, rm_sdf_trace_blocks: READ a baked lattice back at arbitrary
 * points and MARCH rays through it (no reference counterpart).  For what is asked over and over of one static scene: particle
 * collision (distance and gradient at many points per tick), line of sight, picking, camera collision, a caller's own ambient
 * occlusion or shadow rays.  A march step costs eight loads and seven lerps instead of an evaluation of the scene.  d_dist and
 * d_objectId (may be NULL) are a lattice in rm_sdf_grid's layout (x fastest) or in rm_sdf_grid_blocks' (729 values per list entry,
 * void entries skipped, of equal entries the first counts), from there or from anywhere else.  d_points: numPoints float4 (w is not
 * read); d_rays: numRays RmRay; d_samples: numPoints RmFieldSample; d_hits: numRays RmRayHit.  origin and step are host memory,
 * copied before return.  Asynchronous on `stream`.
 * Definition, bit for bit.  Every operation is one binary32 operation, never fused; division and square root are correctly rounded.
 * min(a, b) = a < b ? a : b, max(a, b) = a > b ? a : b, clamp(x, lo, hi) = min(max(x, lo), hi) with max(x, lo) = x > lo ? x : lo: a
 * NaN clamps to lo.
 * Lattice coordinates.  The extent per axis is N_a = n_a − 1 (dense) or 8·m_a (blocks).  A point has u_a = (p_a − origin_a) / step_a;
 * a ray has uo_a = (ro_a − origin_a) / step_a, ud_a = rd_a / step_a and u(t)_a = uo_a + ud_a · t.
 * Cell sample — of cell (i, j, k) with its eight values v[c], c = cx + 2·cy + 4·cz as in rm_sdf_mesh, at u: f_a = u_a − (float)cell_a;
 * lerp(a, b, w) = a + w·(b − a).  value: lerp along x on the four x-edges (v0,v1) (v2,v3) (v4,v5) (v6,v7), then along y on the
 * pairs (0,1) (2,3) of those results, then along z.  gradient: that interpolant's derivative in world units,
 *   gx = lerp(lerp(v1−v0, v3−v2, fy), lerp(v5−v4, v7−v6, fy), fz) / step_x
 *   gy = lerp(lerp(v2−v0, v3−v1, fx), lerp(v6−v4, v7−v5, fx), fz) / step_y
 *   gz = lerp(lerp(v4−v0, v5−v1, fx), lerp(v6−v2, v7−v3, fx), fy) / step_z
 * object id: with d_objectId the id stored at the corner (fx >= 0.5, fy >= 0.5, fz >= 0.5); without it −1 for a sample and 0 for a ray
 * hit.  NaN and infinite lattice values get no special case: the arithmetic is as written (WHICH NaN an operation returns, its sign
 * and payload, is the hardware's; that a word is a NaN is defined).  A cell needs only its own eight values, which in the block
 * layout all live in one entry's slot: no neighbour is looked up.
 * rm_sdf_sample.  Invalid point: a non-finite component; it stores objectId = RM_RAY_INVALID and zeros.  Inside iff 0 <= u_a <= N_a on
 * every axis, decided on the floats (a NaN or infinite u is outside); an outside point stores objectId = RM_FIELD_OUTSIDE and zeros.
 * An inside point has cell_a = min((int)floor(u_a), N_a − 1) and stores the cell sample: gradient, value, cell, objectId.
 * rm_sdf_sample_blocks.  The same, and: block b_a = min(cell_a >> 3, m_a − 1); where no entry that counts names b it stores objectId =
 * RM_FIELD_UNLISTED with `cell` filled and value and gradient zeros; otherwise it reads local cell cell − 8·b of the slot of the first
 * entry that names b.  Wherever the block is listed the record is rm_sdf_sample's on the dense lattice in every bit.
 * rm_sdf_trace_blocks.
 * 1. Invalid ray: rm_trace_rays' rules (a non-finite component of origin or dir, dir all zeros, tMax NaN or negative), or a component
 *    of uo or ud that is not finite, or ud all zeros (a dir that underflows in lattice units).  It stores objectId = RM_RAY_INVALID,
 *    t = 0 and zeros.
 * 2. Box entry by slabs on [0, N_a].  near = −inf, far = +inf; for each axis with ud_a != 0: t1 = (0 − uo_a) / ud_a, t2 = ((float)N_a −
 *    uo_a) / ud_a, near = max(near, min(t1, t2)), far = min(far, max(t1, t2)); an axis with ud_a == 0 makes the ray miss if uo_a < 0 or
 *    uo_a > N_a.  t = max(near, 0) (a near of −0 or below gives +0), tEnd = min(tMax, far).  The ray misses unless t <= tEnd.
 * 3. forced = false; then maxSteps times at most: miss if t > tEnd.  u_a = uo_a + ud_a · t.  If not forced: u_a = clamp(u_a, 0, N_a)
 *    and b_a = min((int)floor(u_a) >> 3, m_a − 1).  If forced: b stays and u_a = clamp(u_a, 8·b_a, 8·b_a + 8).
 *    Listed block: cell_a = min((int)floor(u_a), 8·b_a + 7); the cell's value at u; forced = false; HIT iff value < iso (rm_sdf_mesh's
 *    inside: a NaN is no hit); otherwise t = t + value (the renderer's march step: t is in units of |dir|).
 *    Unlisted block: skip to its exit.  For each axis with ud_a != 0: F_a = (float)(8·(b_a + (ud_a > 0 ? 1 : 0))), ta = (F_a − uo_a) /
 *    ud_a.  The exit axis is the one with the smallest ta, the first in x, y, z order on a tie; b[axis] += (ud_axis > 0 ? 1 : −1), an
 *    exact integer step; miss if that leaves [0, m_axis); t = max(ta, t) (ta > t ? ta : t); forced = true.
 *    Every skip changes an integer block coordinate, so a ray cannot stall on a rounded boundary; a skip costs one of the maxSteps
 *    iterations.
 * 4. Hit: t as it is; position_a = ro_a + rd_a · t, unfused; normal = g / sqrt((gx·gx + gy·gy) + gz·gz) with g the cell sample's
 *    gradient, zeros where that length is 0 or not finite; objectId as in the cell sample.  With RM_TRACE_NO_NORMAL normal and position
 *    are zeros; objectId and t are the same bits.
 * 5. Miss, exhausted steps included: rm_trace_rays' miss, objectId = −1, t = tMax as given, zeros.
 * rm_sdf_trace is the same loop on ONE region in which everything is listed: the clamp is to [0, n_a − 1] and cell_a = min((int)floor(
 * u_a), n_a − 2).  With n = 8·m + 1 and a list of every block the two give equal bits.
 * The sparse march knows nothing about the inside of unlisted blocks: a ray that starts inside an object in an unlisted block reports
 * the first listed sample below iso, not t = 0.  With the list of rm_sdf_blocks_select at the same iso a ray that starts outside the
 * surface meets it where the dense march does.  The result of a point or ray does not depend on which others share its call.
 * In this order, and all but the last before any HIP call, RM_ERR_INVALID_ARGUMENT: a negative numPoints / numRays; null origin or
 * step, an origin component that is not finite, a step component that is not finite or not greater than 0; dense: a dimension above
 * RM_MAX_LATTICE_DIM or more than INT_MAX points (rm_sdf_mesh's rules) or a dimension below 2 (these entries need a cell); blocks: a
 * block dimension below 1 or above RM_MAX_LATTICE_BLOCKS, then numBlocks below 0 or above RM_MAX_BLOCK_LIST; the marches: iso not
 * finite, maxSteps outside 0 … RM_MAX_FIELD_STEPS, mode bits other than RM_TRACE_NO_NORMAL.  Then a count of 0: RM_OK, nothing read or
 * written.  RM_ERR_INVALID_ARGUMENT: a null d_points / d_rays or d_samples / d_hits, a null d_dist or d_blocks with numBlocks above 0; a
 * misaligned pointer (16 bytes for points, rays, samples and hits, 4 for the rest); an array that is not device memory.  numBlocks =
 * 0 with points or rays is valid: every point in the box is RM_FIELD_UNLISTED, every valid ray misses.
 * Schedule: ONE launch, one lane per point or ray, 256-lane workgroups; the block entries build the block map of the list first (4 B
 * per block of the virtual lattice in the workspace of rm_sdf_blocks_select: rm_set_workspace_limit and rm_release_workspaces apply;
 * it is rebuilt on every call).  A marching lane keeps the slot of its current block while the block does not change.  No scene is
 * staged and no slot of the ring of scene blocks is used.  Not render launches: rm_debug_last_path() keeps its value and
 * rm_set_timing does not time them.  Rays that share a wave cost what the longest of them costs: keep neighbours together
 * (rm_rays_order).
 * Added without a change of RM_ABI_VERSION (new symbols and nothing else): bindings detect them by symbol lookup.
 */
typedef struct RmFieldSample { float gradient[3]; float value; int32_t cell[3]; int32_t objectId; } RmFieldSample; /* 32 bytes */
#define RM_FIELD_OUTSIDE (-5)  /* RmFieldSample.objectId of a point outside the lattice's box */
#define RM_FIELD_UNLISTED (-6) /* … of a point in a block that no entry of the list names */
#define RM_MAX_FIELD_STEPS 65536
int rm_sdf_sample(const float *d_points /* float4 each, w not read */, int numPoints, const float *d_dist,
                  const int32_t *d_objectId /* may be NULL */, int nx, int ny, int nz, const float origin[3], const float step[3],
                  RmFieldSample *d_samples, void *stream);
int rm_sdf_sample_blocks(const float *d_points /* float4 each, w not read */, int numPoints, const float *d_dist,
                         const int32_t *d_objectId /* may be NULL */, const int32_t *d_blocks /* int4 each */, int numBlocks, int mx,
                         int my, int mz, const float origin[3], const float step[3], RmFieldSample *d_samples, void *stream);
int rm_sdf_trace(const RmRay *d_rays, int numRays, const float *d_dist, const int32_t *d_objectId /* may be NULL */, int nx, int ny,
                 int nz, const float origin[3], const float step[3], float iso, int maxSteps,
                 unsigned mode /* 0 or RM_TRACE_NO_NORMAL */, RmRayHit *d_hits, void *stream);
int rm_sdf_trace_blocks(const RmRay *d_rays, int numRays, const float *d_dist, const int32_t *d_objectId /* may be NULL */,
                        const int32_t *d_blocks /* int4 each */, int numBlocks, int mx, int my, int mz, const float origin[3],
                        const float step[3], float iso, int maxSteps, unsigned mode /* 0 or RM_TRACE_NO_NORMAL */, RmRayHit *d_hits,
                        void *stream);

/*
 * Lattice handles — rm_field_create, rm_field_create_blocks, rm_field_destroy, rm_field_sample, rm_field_trace: the lattice queries
 * above for a caller that asks ONE lattice again and again (particle collision every tick, a frame's shadow rays).  An RmField is
 * built once and owns what is derived from the block list, so a query is one launch and nothing else; and its march takes
 * RM_TRACE_OCCLUSION, which rm_sdf_trace and rm_sdf_trace_blocks refuse.
 * Ownership and lifetime.  The handle borrows d_dist and d_objectId (may be NULL): they are not copied, the caller keeps them alive
 * until rm_field_destroy, and may rewrite the VALUES in place between calls (ordered against the queries by the caller's streams); a
 * query reads what is there when it runs.  The handle consumes d_blocks: rm_field_create_blocks enqueues its build on `stream` and
 * synchronises that stream before it returns, so the list may be freed at once and the handle is usable on any stream afterwards.
 * The handle owns its block map (4 B per block of the virtual lattice) and its coarse level (8 B per group of 4×4×4 blocks) in device
 * memory of its own, from plain hipMalloc and not the kWsBlocks workspace: rm_set_workspace_limit and rm_release_workspaces do not
 * apply to it, and only rm_field_destroy frees it.  A dense handle owns no device memory.  origin and step are host memory, copied.
 * The handle records the device current at create; a query with another device current is RM_ERR_INVALID_ARGUMENT.  A magic word in
 * the struct guards against a destroyed or garbage handle — best effort only: a pointer that was never a handle may fault, and a
 * destroyed handle's memory may be reused.  Queries of one handle may run concurrently from several threads and streams;
 * rm_field_destroy may not run beside them, and the caller synchronises the streams that still use the handle first.
 * rm_field_sample is rm_sdf_sample (dense handle) / rm_sdf_sample_blocks (block handle) on the handle's lattice, in every bit.
 * rm_field_trace, modes RM_TRACE_CLOSEST and RM_TRACE_NO_NORMAL, on a dense handle is rm_sdf_trace in every bit, for every maxSteps.
 * On a block handle the march is rm_sdf_trace_blocks' state machine (its step 3) with ONE change: maxSteps counts samples only, a
 * skip is free.  samples = 0; then repeat: miss if t > tEnd; u and b as in step 3, forced or not; if the block is unlisted, the skip
 * of step 3 exactly as written (exit axis by the smallest ta, x before y before z; the integer step; miss if it leaves the lattice;
 * t = max(ta, t); forced = true) and start over; otherwise miss if samples == maxSteps; samples += 1; the cell's value at u; forced
 * = false; HIT iff value < iso; else t = t + value.  A run of skips between two samples is at most mx + my + mz long, so the loop ends.
 * Wherever rm_sdf_trace_blocks with the same list needed no more than its budget, skips included, and this march no more than
 * maxSteps samples, the two records are equal in every word.  The coarse level (Schedule, below) is an implementation detail: what
 * it does in one step has the bits of the run of skips written here, and a build without it (-DRM_FIELD_COARSE=0) gives the same words.
 * RM_TRACE_OCCLUSION, dense or blocks: the same loop with the renderer's penumbra tracker (softshadow, frag:1703-1725, k =
 * RM_FIELD_PENUMBRA_K).  res = 1 before the loop.  At every sample that is not a hit, BEFORE t advances: q = (8·value) / t, unfused,
 * the division correctly rounded, t as it stands (a first sample at t = 0 gives ±inf or NaN); res = q < res ? q : res, so a NaN q
 * never enters.  Hit: objectId as the cell sample has it (0 without ids), t = res.  Miss — a missed box, the box, the lattice or tMax
 * left, the samples used up —: objectId = −1, t = res; a ray that never sampled stores 1.  normal and position are zeros in both.
 * Invalid ray: as in the closest march.  What a caller reads as visibility is objectId == −1 ? t : 0, as with rm_trace_rays.  The t
 * sequence is the closest march's, so occlusion hits iff closest hits, with the same objectId.
 * rm_field_create / rm_field_create_blocks refuse, in this order and all but the last before any HIP call, with *field = NULL on every
 * failure, RM_ERR_INVALID_ARGUMENT: what rm_sdf_sample / rm_sdf_sample_blocks refuse about the lattice, with their messages (null
 * origin or step, origin, step; dense: the dimensions, INT_MAX points, a dimension below 2; blocks: the block dimensions, then
 * numBlocks); a null `field`; a null d_dist (unless numBlocks == 0) or a null d_blocks with numBlocks above 0; a misaligned d_dist,
 * d_objectId or d_blocks (4 bytes); an array that is not device memory.  A HIP failure (no memory for the map) is RM_ERR_DEVICE.
 * rm_field_destroy(NULL) is a no-op.
 * rm_field_sample / rm_field_trace refuse, in this order, RM_ERR_INVALID_ARGUMENT: a null or bad handle; a negative numPoints /
 * numRays; the march: iso not finite, maxSteps outside 0 … RM_MAX_FIELD_STEPS, mode bits other than RM_TRACE_NO_NORMAL and
 * RM_TRACE_OCCLUSION, or both of them together (rm_trace_rays' rule).  Then a count of 0: RM_OK, nothing read or written.  Then a null
 * d_points / d_rays or d_samples / d_hits; a misaligned one (16 bytes); — from here on with HIP calls — another device current than
 * the handle's; an array that is not device memory.
 * Schedule: ONE launch per query, one lane per point or ray, 256-lane workgroups, two 16-byte stores per record.  At create a block
 * handle builds, beside the block map, one 64-bit occupancy mask per group of 4×4×4 blocks (bit (bx&3) | (by&3)<<2 | (bz&3)<<4; the
 * groups at the high faces are ragged).  A marching lane keeps its group's mask in registers while the group does not change and
 * loads the block map only for a listed block whose slot it does not hold: one 8-byte load per group crossed instead of one
 * dependent 4-byte load per block crossed.  A group whose mask is 0 is left in ONE step: the run of skips that crosses it is the
 * stable merge of the three axes' face sequences by (ta, axis), each of them sorted because a rounded subtraction and a correctly
 * rounded division by a fixed ud are monotone; so the run leaves on the axis whose last face inside the group (clipped to the
 * lattice) has the smallest (ta, axis) = (T, A), every other axis c has by then crossed its faces inside the group with (ta, c) <
 * (T, A), at most three; the run's t = ta > t ? ta : t, skip after skip, is T > t ? T : t in every bit as long as T is not ±0 (equal
 * binary32 numbers have equal bits unless they are zeros of two signs), and for T = ±0 the step is not taken: the fine skips run
 * (rm_field_skip.h has the argument, tests/test_field_handle_spec.py the proof by campaign against the build without the level).  No scene is staged and no slot of the ring of scene blocks is used.  Not render launches:
 * rm_debug_last_path() keeps its value and rm_set_timing does not time them.
 * Added without a change of RM_ABI_VERSION (new symbols and nothing else): bindings detect them by symbol lookup.
 */
typedef struct RmField RmField;   /* opaque */
#define RM_FIELD_PENUMBRA_K 8.0f  /* the k of lightTerm's softshadow, rm_trace_rays' */
int  rm_field_create(const float *d_dist, const int32_t *d_objectId /* may be NULL */, int nx, int ny, int nz,
                     const float origin[3], const float step[3], RmField **field);
int  rm_field_create_blocks(const float *d_dist, const int32_t *d_objectId /* may be NULL */, const int32_t *d_blocks, int numBlocks,
                            int mx, int my, int mz, const float origin[3], const float step[3], void *stream, RmField **field);
void rm_field_destroy(RmField *field);   /* NULL is a no-op */
int  rm_field_sample(const RmField *field, const float *d_points, int numPoints, RmFieldSample *d_samples, void *stream);
int  rm_field_trace(const RmField *field, const RmRay *d_rays, int numRays, float iso, int maxSteps,
                    unsigned mode /* RM_TRACE_CLOSEST, | RM_TRACE_NO_NORMAL, or RM_TRACE_OCCLUSION */, RmRayHit *d_hits, void *stream);

/*
 * rm_field_ambient — hemisphere occlusion and the bent normal at POINTS of a baked lattice, one launch: numDirs rays per point from a
 * table of directions, each marched by rm_field_trace's own march, summed inside the kernel by a fixed binary32 tree.  No device
 * memory proportional to numPoints·numDirs exists at any time: the caller who composes the same from rm_field_trace writes 32 B per
 * ray and reads 32 B per ray back.  rm_hemisphere_directions fills a table on the host.
 * d_points: numPoints float4 in device memory (w is not read); d_normals: as many float4 (w is not read) or NULL, the lattice's own
 * gradient then; d_dirs: numSets·numDirs float4 in device memory, (x, y, z) in the point's frame with z along its normal and w the
 * ray's weight; point i uses set i mod numSets.  d_out: numPoints RmAmbient.  Asynchronous on `stream`.
 * Definition for point i, bit for bit: every operation below is ONE binary32 operation, unfused, in the order written, division and
 * sqrt correctly rounded (rm_field_ambient.h is this text in C++).  p = points[i].xyz.  The record starts as zeros.
 * a. A non-finite component of p: hits = RM_RAY_INVALID, the rest zeros.
 * b. The normal n.  With d_normals: normals[i].xyz as given — unit length is the caller's duty —; a non-finite component or all three
 *    zero: hits = RM_RAY_INVALID.  Without: s = rm_field_sample's record at p; RM_FIELD_OUTSIDE or RM_FIELD_UNLISTED there goes to hits;
 *    otherwise len = sqrt((gx·gx + gy·gy) + gz·gz) and n = g / len, component by component; len zero or not finite: hits =
 *    RM_RAY_INVALID.  In every refused case the rest of the record stays zero, `normal` included.
 * c. The frame (Duff et al. 2017, "Building an orthonormal basis, revisited"): s = copysign(1, n.z); a = −1 / (s + n.z); b = (n.x·n.y)·a;
 *    T = (1 + (s·(n.x·n.x))·a, s·b, (−s)·n.x); B = (b, s + (n.y·n.y)·a, −n.y).  No direction is singular: n.z = −1 gives a = 0.5.
 * d. For k = 0 … numDirs − 1: e = dirs[(i mod numSets)·numDirs + k]; d[c] = (e.x·T[c] + e.y·B[c]) + e.z·n[c]; o[c] = p[c] + n[c]·bias;
 *    h = rm_field_trace's march of the ray (o, tMax = maxDistance, d) with iso and maxSteps — RM_AMBIENT_SOFT: its RM_TRACE_OCCLUSION
 *    march; RM_AMBIENT_HARD: its RM_TRACE_NO_NORMAL march.  v = 0 if h.objectId != −1 (a hit, an invalid ray); on a miss SOFT has v =
 *    h.t > 0 ? h.t : 0 — the penumbra factor starts at 1 and only falls, so v lies in [0, 1] on a finite lattice and no infinity or
 *    NaN enters a sum — and HARD has v = 1.  A hit (objectId neither −1 nor RM_RAY_INVALID) adds 1 to hits.  c = e.w·v, and leaf k =
 *    (c·d.x, c·d.y, c·d.z, c).
 * e. The four components are summed over the leaves by the pairwise tree, level by level: s[j] = s[2j] + s[2j + 1], numDirs a power
 *    of two.  bent = the first three sums, not normalised; visibility = the fourth; normal = the n used; hits = the count.
 * f. The contract covers finite tables and lattices.  A non-finite d_dirs entry may put a NaN into the sums; its sign and payload
 *    are not specified.
 * bias moves the origins off the surface and must exceed iso by a margin: at p + bias·n the field is about bias, and a first sample
 * below iso is a hit at t = 0.  With rm_hemisphere_directions' table, visibility is the cosine-weighted open fraction of the
 * hemisphere within maxDistance.
 * rm_hemisphere_directions(numDirs, numSets, out4), host only: for set s and index k, in double and then rounded to float, u = (k +
 * 0.5) / numDirs, r = sqrt(u), z = sqrt(1 − u), φ = 2π·frac(k·0.6180339887498949 + s·0.7548776662466927), entry (r cos φ, r sin φ, z,
 * 1 / numDirs): a cosine-weighted spiral, one rotation per set.  It refuses numDirs and numSets as below, then a null out4.
 * rm_field_ambient refuses, in this order, RM_ERR_INVALID_ARGUMENT: a null or bad handle; a negative numPoints; numDirs not a power of
 * two in 1 … RM_MAX_AMBIENT_DIRS; numSets below 1 or numSets·numDirs above RM_MAX_AMBIENT_TABLE; bias, maxDistance or iso not finite or
 * maxDistance below 0; maxSteps outside 0 … RM_MAX_FIELD_STEPS; mode bits other than RM_AMBIENT_HARD.  Then numPoints == 0: RM_OK,
 * nothing read or written.  Then a null d_points, d_dirs or d_out; a misaligned one (16 bytes), d_normals included when it is given;
 * — from here on with HIP calls — another device current than the handle's; an array that is not device memory.
 * Schedule: ONE launch, 256-lane workgroups, (point, direction) pairs flattened over lanes so that lane mod numDirs is the direction:
 * up to 64 directions a wave holds 64 / numDirs points and folds each segment by log2(numDirs) xor-shuffle levels; 128 and 256 are 2
 * or 4 passes of 64 by one wave, folded by the same tree.  binary32 addition is commutative in every bit, so the butterfly has the
 * tree's words.  The table, at most 16 KB, is staged into LDS once per workgroup; a record is two 16-byte stores.  Not a render
 * launch: rm_debug_last_path() keeps its value.  Added without a change of RM_ABI_VERSION: bindings detect it by symbol lookup.
 */
typedef struct RmAmbient { float bent[3]; float visibility; float normal[3]; int32_t hits; } RmAmbient;   /* 32 bytes */
#define RM_AMBIENT_SOFT 0u      /* every ray is rm_field_trace's RM_TRACE_OCCLUSION march */
#define RM_AMBIENT_HARD 1u      /* every ray is its RM_TRACE_NO_NORMAL march: visible or not */
#define RM_MAX_AMBIENT_DIRS 256
#define RM_MAX_AMBIENT_TABLE 1024   /* numSets * numDirs */
int rm_hemisphere_directions(int numDirs, int numSets, float *out4 /* host, numSets*numDirs float4 */);
int rm_field_ambient(const RmField *field, const float *d_points /* float4 each, w not read */,
                     const float *d_normals /* float4 each, w not read; may be NULL */, int numPoints,
                     const float *d_dirs /* float4 each: local x, y, z, weight */, int numDirs, int numSets,
                     float bias, float maxDistance, float iso, int maxSteps, unsigned mode,
                     RmAmbient *d_out, void *stream);

/*
 * rm_shade_points — what the renderer thinks of POINTS the caller already has: the scene's distance and object at each point, its
 * normal, its ambient occlusion and its shaded colour, with the point optionally projected onto the iso-surface first (no reference
 * counterpart: the shader reaches a surface point only at the end of a ray of its own).  The points counterpart of rm_trace_rays /
 * rm_shade_rays.  For the vertices of rm_sdf_mesh — normals, AO, baked colours, and vertices moved from the mean of their cell's
 * edge crossings onto the surface —, particles and decals placed on a surface, a physics engine's contact normal, lighting baked
 * into any point cloud.  d_points: numPoints float4 in device memory, rm_sdf_mesh's d_vertices as they are (w is not read); d_view
 * (may be NULL): numPoints float4, the direction the point is seen along, rm_shade_rays' dir (w is not read).  Outputs, each may be
 * NULL but not all three: d_surface, numPoints RmSurfacePoint; d_ao, a float each; d_rgba, a float4 each.  The tables, ps, g, s and
 * res (may be NULL) are host memory, copied before return.  Asynchronous on `stream`.
 * Definition for point i, bit for bit (the oracle's functions under the rm_math contract; madd is render's fused a·s + b).
 * 1. p = points[i].xyz; with d_view, rd = view[i].xyz.  Invalid point: a non-finite component of p or, with d_view, a non-finite
 *    component of rd or rd all zeros.  It stores objectId = RM_RAY_INVALID and zeros in the rest of d_surface, 0 in d_ao, (0, 0, 0, 0)
 *    in d_rgba, and evaluates nothing.  Points are device data: the host cannot refuse them.
 * 2. Projection.  p0 = p; projectSteps times: sc = sdScene(p) (frag:1406-1430), stop if sc.minObjIdx == −1; e = sc.minD − iso; N =
 *    getNormal(p) (frag:1436-1444, never bumped); q = madd(N, −e, p); stop if a component of q is not finite; m = q − p0; stop unless
 *    dot(m, m) <= maxMove·maxMove (one binary32 product; +inf admits every finite q); p = q.  A stop keeps the last accepted p.
 * 3. sc = sdScene(p) with the shader's trap (UB3: the trap of the last fractal evaluated, as the primary march has it); distance =
 *    sc.minD, objectId = sc.minObjIdx, position = p.  objectId == −1 (an empty table, a NaN estimate): normal zeros, ao 0, colour
 *    (0, 0, 0, 0), done.
 * 4. N = getNormal(p) (frag:1436-1444), then bumpNormal(N, p, 10, 2) (frag:1679-1691) under RM_FEAT_PERLIN_BUMP; normal = N.
 * 5. With d_ao: calcAO(p, N) (frag:1729-1740), whatever s->enableAmbientOcclusion says.
 * 6. With d_rgba: rd = view[i].xyz if d_view is given, else −N (the point seen head-on: the view-independent bake).  Then render()
 *    from behind its march (frag:2337-2375) with res.intersectObj = objectId, res.trap = sc.trap and maxT = ps->far: an emissive
 *    object gives (color, 1); otherwise getPhong(N, objectId, p, rd, far) (frag:1842-1933; ambient occlusion under
 *    s->enableAmbientOcclusion, shadow rays, area lights) times the Mandelbulb's or the sponge's trap palette (frag:2354-2365), alpha
 *    1.  No reflection and no refraction: those are rays, rm_shade_rays' business.  A hit point of rm_trace_rays with view = the ray's
 *    dir gives rm_shade_rays' colour where that ray fires no secondary ray and the march's object is sdScene's at the hit point
 *    (on a Mandelbulb or a sponge up to the orbit trap, which the march has from its last evaluated point, res.d short of the hit).
 *    An area light seen head-on is degenerate where V = N in every bit — LTC_Evaluate (frag:368-424) normalises V − N·(N·V), a zero
 *    vector — and the colour is NaN there, as it is for a ray that meets a surface exactly along its normal: pass d_view with area lights.
 * Work follows the outputs: d_surface alone costs 1 + 4 evaluations of sdScene plus 5 per projection step; d_ao adds AO's taps;
 * only d_rgba marches shadow rays and reads lights and samplers (without it `lights` may be NULL and the samplers are not checked).
 * The result of a point does not depend on which points share its call, and every output holds the same bits whichever of the
 * others are NULL.  `far` is ONE value per call, as rm_shade_rays has it.
 * numPoints == 0: RM_OK, nothing read or written.  Otherwise, in this order and all but the last before any HIP call:
 * RM_ERR_INVALID_ARGUMENT: numPoints < 0; null ps, g or s, a null table with a positive count (the lights' only with d_rgba) or a
 * negative count; far NaN, negative or infinite; iso not finite; maxMove NaN or negative (+inf is valid); projectSteps outside 0 …
 * RM_MAX_PROJECT_STEPS; all three outputs NULL.  RM_ERR_UNSUPPORTED: RM_FEAT_TERRAIN, RM_FEAT_CLOUD or RM_FEAT_SEA, g->isTwoD.  Then
 * the scene: with d_rgba rm_render_res's checks with its statuses (rm_shade_rays' list), without it rm_trace_rays' checks of the
 * table.  RM_ERR_INVALID_ARGUMENT: null or misaligned d_points, a misaligned d_view, d_surface or d_rgba (16 bytes) or d_ao (4
 * bytes); an array or, with d_rgba, a sampler's pixels that are not device memory.
 * Schedule: ONE launch, one lane per point, 256-lane workgroups, of the points kernel of the scene's class — the table walk, the
 * general Mandelbulb, its plain form, or the samplers' (rm_debug_last_path() = 17, rm_debug_last_split() = 0); the Mandelbulb
 * classes march hard shadows from directional lights in the wave's shadow pool, as rm_shade_rays does.  It uses one slot of the batch
 * ring of scene blocks and neither reads nor changes the per-stream tuner and tile-order state of single-frame renders, and no
 * library workspace.  With rm_set_timing(1) it counts as one launch, all stage 1.  Points that share a wave (64 consecutive points)
 * cost what the dearest of them costs: keep neighbours together (rm_sdf_mesh's vertex order does).
 * Added without a change of RM_ABI_VERSION (new symbols and nothing else): bindings detect them by symbol lookup.
 */
typedef struct RmSurfacePoint { float normal[3]; float distance; float position[3]; int32_t objectId; } RmSurfacePoint; /* 32 bytes, RmRayHit's shape */
typedef struct RmPointsSettings { float far; float iso; float maxMove; int32_t projectSteps; } RmPointsSettings;
void rm_points_settings_default(RmPointsSettings *ps);   /* far 100, iso 0.001 (the march's hit threshold), maxMove +inf, projectSteps 0 */
#define RM_MAX_PROJECT_STEPS 16
int rm_shade_points(const float *d_points /* float4 each: rm_sdf_mesh's d_vertices as they are; w is not read */,
                    const float *d_view /* float4 each, may be NULL */, int numPoints, const RmPointsSettings *ps,
                    const RmObject *objs, int numObjects, const RmLight *lights, int numLights, const RmGlobals *g,
                    const RmSettings *s, const RmResources *res /* may be NULL */,
                    RmSurfacePoint *d_surface /* may be NULL */, float *d_ao /* 1 float each, may be NULL */,
                    float *d_rgba /* float4 each, may be NULL */, void *stream);

/*
 * rm_render_tiles — the multi-GPU shard of the same frame (no reference counterpart; the reference
 * renders whole frames on one GPU).  The frame is cut into tiles of `tileRows` rows; this call renders
 * tiles t with t % numShards == shard, packed contiguously in tile order into d_rgba
 * (rm_shard_rows() rows × W float4).  Interleaving balances the centre-heavy cost across GPUs.
 */
int rm_render_tiles(const RmCamera *cam, const RmObject *objs, int numObjects, const RmLight *lights,
                    int numLights, const RmGlobals *g, const RmSettings *s, int W, int H, int tileRows,
                    int shard, int numShards, float *d_rgba, float *d_bright, void *stream);
/* rm_render_tiles with the samplers of rm_render_res (`res` may be NULL): every shard passes the same resources, each
 * GPU holding its own copy of the images. */
int rm_render_tiles_res(const RmCamera *cam, const RmObject *objs, int numObjects, const RmLight *lights, int numLights,
                        const RmGlobals *g, const RmSettings *s, const RmResources *res, int W, int H, int tileRows,
                        int shard, int numShards, float *d_rgba, float *d_bright, void *stream);
/* The row-tile partition.  Default (root relief 0): tile t belongs to shard t mod numShards.  rm_set_root_relief(K), K in 2..64:
 * the deal runs in cycles of numShards·K − 1 tiles — K − 1 full rounds, then one round that leaves shard 0 out — so shard 0, the
 * gather's root (which also receives numShards − 1 slots and de-interleaves the whole frame every frame), renders (K − 1)/K of a
 * peer's tiles.  The setting is PROCESS-WIDE and every entry point that deals tiles reads it (rm_render_tiles*, rm_shard_rows,
 * rm_shard_row_to_frame, rm_deinterleave*, rm_gather_*): every rank of a job sets the same value before rendering.  With relief
 * the largest shard is shard 1, not shard 0: size gather slots by rm_gather_slot_rows.  0 switches it off. */
int rm_set_root_relief(int K);
int rm_get_root_relief(void);
/* Rows owned by `shard` under the rm_render_tiles partition. */
int rm_shard_rows(int H, int tileRows, int shard, int numShards);
/* Frame row of the shard's packed row `localRow` (inverse map used when de-interleaving a gather). */
int rm_shard_row_to_frame(int H, int tileRows, int shard, int numShards, int localRow);
/*
 * rm_deinterleave — scatter the concatenation of all shards' packed rows (shard 0 first, the layout an
 * RCCL gather produces) into frame order.  Shard k's rows start at row k·shardStrideRows of d_gathered
 * (equal-sized gather slots, padded at the end); shardStrideRows = 0 means tightly packed.
 * d_frame: H·W float4, device, distinct from d_gathered.
 */
int rm_deinterleave(const float *d_gathered, float *d_frame, int W, int H, int tileRows, int numShards,
                    int shardStrideRows, void *stream);

/*
 * rm_gather_* — the gather of a sharded frame, for a host that drives all GPUs of a node from ONE process (no reference
 * counterpart).  devices[k] renders shard k of numDevices (rm_render_tiles on a stream of that device);
 * rm_gather_tiles then moves every shard's packed rows into slot k of d_gathered on devices[root] — one grouped
 * ncclSend / ncclRecv pair per peer over RCCL (xGMI: each peer has its own link to the root), the root's own tiles by a
 * device copy — asynchronously: the send of shard k is enqueued on streams[k] (behind its render), the receives on
 * streams[root], where rm_deinterleave(d_gathered, d_frame, W, H, tileRows, numDevices, rm_gather_slot_rows(...),
 * streams[root]) follows.  Slots are rm_gather_slot_rows(H, tileRows, numDevices) rows each (the largest shard), so
 * d_gathered holds numDevices · slotRows · W float4.  librccl is loaded on first use (RM_ERR_UNSUPPORTED if absent);
 * with one device no communicator is created.  One process per GPU (torch.distributed / MPI hosts) does not need this:
 * raymarcher_amd/dist.py gathers with the process group's own RCCL.
 */
typedef struct RmGather RmGather;
int rm_gather_create(const int *devices, int numDevices, RmGather **out);
/* flags: RM_GATHER_FORCE_COMM builds the RCCL communicator(s) even for ONE device and sends the root's own tiles to itself
 * through ncclSend / ncclRecv instead of a device copy — the whole RCCL path (library load, ncclCommInitAll, a grouped
 * send / receive pair) on a one-GPU box; tests and bring-up.  A grouped call that fails aborts the communicators
 * (ncclCommAbort: no unmatched send is left on a stream) and the object refuses further use. */
enum { RM_GATHER_FORCE_COMM = 1u };
int rm_gather_create_ex(const int *devices, int numDevices, unsigned flags, RmGather **out);
void rm_gather_destroy(RmGather *g);
int rm_gather_slot_rows(int H, int tileRows, int numShards);
int rm_gather_tiles(RmGather *g, const float *const *d_tiles, float *d_gathered, int W, int H, int tileRows, int root,
                    void *const *streams);
/* The same gather with 4 bytes per pixel instead of 16, for hosts that only need the 8-bit image (saveViewportImage writes
 * a PNG, src/realtime.cpp:284-350): every shard converts its packed tiles with rm_tiles_to_rgba8 (clamp → ×255 → round, no
 * flip) on its own stream, rm_gather_tiles_rgba8 moves them (a quarter of the xGMI traffic into the root), and
 * rm_deinterleave_rgba8 writes the frame — rows in frame order, or flipped top-down like rm_frame_to_rgba8 (flip != 0). */
int rm_tiles_to_rgba8(const float *d_tiles, uint8_t *d_tiles8, int W, int rows, void *stream);
int rm_gather_tiles_rgba8(RmGather *g, const uint8_t *const *d_tiles8, uint8_t *d_gathered8, int W, int H, int tileRows, int root,
                          void *const *streams);
int rm_deinterleave_rgba8(const uint8_t *d_gathered8, uint8_t *d_frame8, int W, int H, int tileRows, int numShards,
                          int shardStrideRows, int flip, void *stream);

/* Fractal / shading work counters of the last counted render (debug/roofline accounting). */
typedef struct RmCounters {
  uint64_t sceneEvals;    /* sdScene evaluations (frag:1406) */
  uint64_t bulbIters;     /* Mandelbulb inner iterations (frag:785-799) */
  uint64_t hitPixels;     /* pixels whose primary ray hit */
  uint64_t shadedPoints;  /* surface points shaded by render() (frag:2333-2373): primary hits and reflection / refraction hits */
  uint64_t terrainEvals;  /* fbm_9 evaluations (frag:630-644): terrain height samples of the TERRAIN layer */
  uint64_t cloudEvals;    /* fbmd_8 evaluations (frag:647-667): cloud density samples (CLOUD) and the terrain's bump / cloud shadow */
  uint64_t shapeEvals;    /* sdMatch evaluations (frag:1262-1293): objects evaluated, summed over the sdScene evaluations — numObjects
                             per evaluation as the shader is written; fewer in RM_COUNT_EXECUTED where the table walk passes over objects */
} RmCounters;
/* Same as rm_render but also accumulates counters with device atomics (slower; synchronises).  Counts the REFERENCE's
 * work: every evaluation the shader as written performs, i.e. without the bit-identical shortcuts of the production
 * kernels (marches ended at the scene's bounding ball, no shadow march for a light that N·L <= 0.005 drops anyway). */
int rm_render_counted(const RmCamera *cam, const RmObject *objs, int numObjects, const RmLight *lights,
                      int numLights, const RmGlobals *g, const RmSettings *s, int W, int H, int rowBegin,
                      int rowEnd, float *d_rgba, float *d_bright, RmCounters *out);
/* mode RM_COUNT_REFERENCE = rm_render_counted; RM_COUNT_EXECUTED counts the work the production kernel really executes
 * (shortcuts honoured) — the pair gives the algorithmic and the executed figure of the roofline. */
enum { RM_COUNT_REFERENCE = 1, RM_COUNT_EXECUTED = 2 };
/* rm_render_counted_ex with samplers (res may be NULL): scenes with procedural layers or samplers are counted in mode
 * RM_COUNT_REFERENCE only (their kernels have no bit-identical shortcuts to tell apart). */
int rm_render_counted_res(const RmCamera *cam, const RmObject *objs, int numObjects, const RmLight *lights,
                          int numLights, const RmGlobals *g, const RmSettings *s, const RmResources *res, int W, int H,
                          int rowBegin, int rowEnd, float *d_rgba, float *d_bright, int mode, RmCounters *out);
int rm_render_counted_ex(const RmCamera *cam, const RmObject *objs, int numObjects, const RmLight *lights,
                         int numLights, const RmGlobals *g, const RmSettings *s, int W, int H, int rowBegin,
                         int rowEnd, float *d_rgba, float *d_bright, int mode, RmCounters *out);
/* Diagnostic build of the single-Mandelbulb kernel and of the plain table-walk kernel (no samplers, no procedural layers;
 * RM_ERR_UNSUPPORTED otherwise): production code + s_memtime / s_memrealtime stamps per wave, written to a buffer of their own: renders the whole frame once, synchronises and returns the shader clock the chip held under
 * this kernel's own load, in MHz (Σ cycle spans ÷ Σ 100 MHz-tick spans over all waves).  Call it after a few back-to-back
 * renders so that the clock has settled.  d_waveSpans (device, may be NULL): 2 words per wave — its first and last
 * s_memrealtime stamp (100 MHz ticks) — indexed tile·w + wave with w = waves per workgroup (1 unless RM_WAVES_PER_BLOCK
 * overrides) and ceil(W / (8·w)) tiles per tile row: size it for (ceil(W/8) + 3)·ceil(H/8) waves; for occupancy timelines. */
int rm_render_clocked(const RmCamera *cam, const RmObject *objs, int numObjects, const RmLight *lights, int numLights,
                      const RmGlobals *g, const RmSettings *s, int W, int H, float *d_rgba, double *shaderMHz,
                      unsigned long long *d_waveSpans);

/* Average device time in ms of the `rm_render*` launches made on the CURRENT device since rm_set_timing(1), timed with
 * hipEvents on their own stream; rm_get_* reads and resets that device's records (the on/off switch is process-wide).
 * rm_set_timing acts on the PROCESS: launches of every thread on every device are recorded while it is on, each in its device's
 * list, and rm_get_timing returns the launches of all threads on the current device. */
int rm_set_timing(int on);
int rm_get_timing(double *avgKernelMs, int *launches);
/* Same, split by role, both averaged over ALL the launches (total = stage 0 + stage 1): stage 1 = the render (the one-lane-per-pixel
 * kernel, or all kernels of the wavefront pipeline), stage 0 = the tile-ordering launches that preceded it in the launches that had
 * them (rm_set_tile_order: a new picture and the first repeats of one; a settled picture, a small frame or raster order has none).
 * A batch of rm_render_batch counts as one launch, all of it stage 1 (its wavefront frames as launches of their own); so does a
 * launch of rm_render_supersampled, rm_render_accumulated, rm_render_animated, rm_render_gbuffer, rm_trace_rays, rm_shade_rays,
 * rm_shade_rays_layers, rm_trace_rays_layers or rm_sdf_grid, and so does a whole call of rm_render_adaptive.
 * Stages 2-3 are zero. */
int rm_get_stage_timing(double *avgTotalMs, double avgStageMs[4], int *launches);
/* Which schedule renders a frame: 0 = the measured-fastest one of the scene's class (default), 1 = one lane per pixel
 * (rm::render_kernel, every class), 5 = the wavefront pipeline of rm_wavefront.hip.h for the table-walk classes (primitives,
 * Menger sponge, Sierpinski; no samplers, procedural layers, refraction, Mandelbulb or 2-D Mandelbrot in the scene) — per
 * generation of rays (primary, then each reflection bounce of frag:2491-2524) a persistent march kernel whose lanes are rays
 * refilled from a queue as they end, a dense surface kernel, the same march kernel over the shadow rays, a dense light /
 * bounce kernel.  A request that does not apply to the scene (5 with a Mandelbulb, samplers, layers or refraction, or on a
 * frame its 32-bit ray ids cannot cover) runs 1.  Both produce identical bits; the switch exists for A/B measurement and
 * tests.  (Paths 2-4, three multi-kernel pipelines of the single-Mandelbulb class, were measured slower than path 1 on every
 * frame incl. frames without tile-order history — profiles/r04_b_bulb_paths.md — and removed in round 4; the numbers are refused.)
 * The switch acts on the PROCESS — every device, stream and thread reads it at its next launch: set it while no other thread is
 * launching. */
int rm_set_kernel_path(int path);
/* Scratch memory the library owns.  Everything the schedules need beyond the caller's frame lives in grow-only buffers per
 * (device, stream): 8 B per tile for the tile-order feedback, the post passes' ping-pong images, the lists of rm_render_adaptive
 * (4 B per pixel of a chunk of frames), and — by far the largest —
 * the wavefront pipeline's ray / hit / path records, ≈(160 + 4·numLights) bytes per pixel of the launch (5.8 GB for a
 * 7680×4320 frame, once per stream that renders such frames).  rm_set_workspace_limit caps the size of any ONE such buffer
 * (0 = no limit, the default; the environment variable RM_WF_MAX_WORKSPACE_BYTES sets the initial value).  When the wavefront
 * workspace exceeds the limit or the device cannot allocate it, a launch that chose the pipeline by itself (kernel path 0)
 * renders with rm::render_kernel instead — identical pixels, no workspace — and remembers the refusal for that stream; only
 * an explicit rm_set_kernel_path(5) reports RM_ERR_DEVICE.  An allocation failure never leaves HIP's error state set.
 * rm_release_workspaces drains the current device and frees all of its buffers (freedBytes may be NULL); a render launch or
 * post pass that another thread is enqueuing on the device at the time finishes its enqueue first.  The next launch that
 * needs a buffer allocates it again, and the next frame on each stream runs in raster tile order.  rm_set_workspace_limit acts
 * on the PROCESS: one limit for every device, stream and thread. */
int rm_set_workspace_limit(unsigned long long bytes);
int rm_release_workspaces(unsigned long long *freedBytes);
/* Tests: the schedule (numbering above; never 0) the most recent render launch on the current device ran, -1 on error; 6 = a
 * batch of rm_render_batch that went out as one launch of the one-lane-per-pixel kernel, 7 = a launch of rm_render_supersampled
 * with ss > 1, 8 = a call of rm_render_adaptive, 9 = a launch of rm_render_accumulated, 10 = a launch of rm_render_animated, 11 = a launch
 * of rm_render_gbuffer, 12 = a launch of rm_trace_rays, 13 = a launch of rm_shade_rays, 14 = a launch of rm_shade_rays_layers, 15 = a
 * launch of rm_trace_rays_layers, 16 = a launch of rm_sdf_grid, 17 = a launch of rm_shade_points, 18 = a launch of rm_sdf_blocks_select,
 * 19 = a launch of rm_sdf_grid_blocks, 20 = a launch of rm_sdf_blocks_select_pruned, 21 = a launch of rm_light_probes, 22 = a launch of rm_light_probes_depth,
 * 23 = a launch of rm_shade_rays_indirect, 24 = a launch of rm_light_probes_indirect (none of them is a
 * value rm_set_kernel_path takes).  The value belongs to the DEVICE, not to the calling thread or stream: it reports the device's most recent launch,
 * whichever thread made it. */
int rm_debug_last_path(void);
/* Tests: how many tiles the most recent render launch on the current device rendered one light per workgroup ("light split": the
 * heaviest tiles of a SETTLED picture of the plain table-walk class with two or more lights are rendered by numLights workgroups
 * each, one shadow march per pixel apiece, and finished — by whichever of them arrives last — from the stored results: the same
 * marches and the same sums in the same order, so the same pixels; it shortens the longest waves of latency-bound frames, C2 0.79 →
 * 0.51 ms.  Whether it pays is measured per picture.  RM_LIGHT_SPLIT=0 turns it off, =n makes the heaviest 1/n of the tiles the
 * candidates; default 256).  0: none; -1 on error.  Per DEVICE, as rm_debug_last_path: the device's most recent launch, whichever
 * thread made it. */
int rm_debug_last_split(void);
/* Tests / experiments: the divisor above for the process — n >= 1 also splits WITHOUT the measurement that normally decides per
 * picture whether the split pays (settled frames 0-1 plain, 2-3 split, the better of the two from then on); 0 = off, -1 = back to
 * RM_LIGHT_SPLIT / the default, measured.  It acts on the PROCESS (every device, stream and thread): set it while no other thread
 * is launching. */
int rm_debug_set_light_split(int div);
/* Launch order of a frame's tiles (workgroups).  Tile costs span three orders of magnitude and a single ray that never
 * converges is a sequential chain of ~1 ms, so a kernel whose heaviest tiles start late ends in a tail of a few lonely
 * waves; starting heavy tiles first removes it.  The order never changes a pixel.  mode 1 (default): every frame records each
 * tile's shader-cycle cost; the next frame of the same size on the same stream starts its tiles heaviest-first by those costs
 * when it is the SAME picture (scene tables, camera, settings, rows) — a picture that keeps repeating settles: from its fifth
 * frame on the order of the fourth is reused, with no ordering launches and no cost recording (RM_TILE_ORDER_SETTLE=0: re-sort
 * every frame) — and otherwise — the first frame, a moved camera, a
 * changed scene — by a geometric classification of the tiles (centre ray against the objects' bounding balls: silhouette rings
 * first, interiors next, background last), combined with the stale costs where a frame of that size was rendered before;
 * scenes with procedural layers or objects without a bound start new pictures in raster order.  mode 0: always raster order;
 * -1: back to the default / the RM_TILE_ORDER environment variable.  Applies to every launch of the one-lane-per-pixel kernel
 * with at least 2048 tiles (not to the 2-D Mandelbrot path or the wavefront pipeline, whose persistent waves balance
 * themselves).  The mode acts on the PROCESS: every device, stream and thread reads it at its next launch. */
int rm_set_tile_order(int mode);
/* Shape of the pixel tile a wave renders: 8×8 by default; for table-walk, sampler and layer scenes the launcher measures, per
 * stream and picture, whether 4 wide × 16 tall tiles are faster (frames 0-1 and 4-5 of a picture run 8×8, frames 2-3 and 6-7 4×16,
 * the second of each pair timed with HIP events) and keeps the shape with the smaller best time from the ninth frame on.  The shape never changes a pixel.  Tests /
 * experiments: mode 0 = tune (default), 3 = always 8×8, 2 = always 4×16, -1 = back to the RM_TILE_SHAPE environment variable.
 * The mode acts on the PROCESS: every device, stream and thread reads it at its next launch. */
int rm_debug_set_tile_shape(int mode);
/* Experiments: force a given launch order (d_order: a device permutation of 0..tileCount-1, or NULL) and / or collect the
 * tiles' costs (d_cost: tileCount device words, accumulated, or NULL) for subsequent launches on the current device. */
int rm_debug_set_tile_order(const int32_t *d_order, uint32_t *d_cost, int tileCount);
/* Tests: the 48 coefficients [triangle][near, far][P0, P1 − P0, P2 − P0][xyzw] from which the kernels interpolate nearClip /
 * farClip (raymarch.vert:23-24 evaluated at the corners of the full-screen quad, realtimerender.cpp:225-238; DESIGN.md
 * §2.3), computed on the host exactly as the launcher stages them.  No GPU needed. */
int rm_debug_ray_planes(const RmCamera *cam, float *out48);
/* Tests: the bounds the launcher stages for ending marches whose miss distance nobody reads: out14 = { ok,
 * centre xyz, R² of the ball, R² of the soft-shadow ball (0 = none), boxOk, box lo xyz, box hi xyz, lip }.  Outside the ball — and,
 * where boxOk, outside the box — every object's distance value exceeds the hit threshold (0.001) by a wide factor, so a ray
 * that has left ball ∩ box for good can only miss.  The box is staged only where it is much tighter than the ball (volume
 * ratio < 0.3).  lip: no object's distance value changes by more than lip per unit of world length (+inf with a fractal in
 * the table): the seed of the table walk's skip test.  A pure function of the object table and the globals; no GPU needed. */
int rm_debug_cull_bounds(const RmObject *objs, int numObjects, const RmGlobals *g, float *out14);
/* Tests: 1 if the launcher renders this table with the plain single-Mandelbulb kernel — one Mandelbulb whose invModel is 1
 * on the diagonal and a zero of either sign elsewhere in the three rows the distance function reads, scaleFactor exactly 1,
 * power 8, both Julia seed components zero — whose evaluations skip the object transform, the ·scaleFactor and the Julia
 * select (same bits); 0 otherwise (another table, or the general Mandelbulb kernel); -1 on a null pointer.  No GPU needed. */
int rm_debug_bulb_plain(const RmObject *objs, int numObjects, const RmGlobals *g);
/* Tests: the per-light constants the launcher stages for the single-Mandelbulb kernels' shadow pool, computed on the host exactly
 * as it stages them: out[8·numLights], per light { L xyz, pd xyz, a, 0 } with L = normalize(−dir) (v · (1 / sqrt(dot(v, v))),
 * dot = fma(z, z, fma(y, y, x·x))), pd = the 3×3 part of objs[0].invModel times L (fma(M[8 + r], L.z, fma(M[4 + r], L.y,
 * M[r]·L.x))) and a = dot(pd, pd): the bits the kernels computed per ray before.  Zeros for a light that is not directional;
 * pd and a are zero for an empty object table.  RM_ERR_INVALID_ARGUMENT: a null pointer with a count above 0, null out, a count
 * below 0 or above RM_MAX_OBJECTS / RM_MAX_LIGHTS.  No GPU needed. */
int rm_debug_light_prep(const RmObject *objs, int numObjects, const RmLight *lights, int numLights, float *out);
/* Tests: the kernels' cheap exact forms against the IEEE operations for every one of the 2^32 inputs, on the current device
 * (≈2 s).  mismatches5[0]: the reciprocal (v_rcp_f32 + one Newton step inside 2^-126 <= |y| < 2^126, the IEEE expansion
 * outside) vs 1.0f / y; [1]: the bare fast form over its range; [2]: the square root (v_sqrt_f32 + residual selection, the
 * scaled expansion only below 2^-96) vs sqrtf; [3]: the unscaled form over its domain; [4]: fract (v_fract_f32) vs
 * x − floor(x) kept below 1.  All must be 0. */
int rm_debug_check_math(unsigned long long *mismatches5);

/*
 * rm_frame_to_rgba8 — clamp→×255→round and vertical flip, the read-back of
 * Realtime::saveViewportImage (src/realtime.cpp:284-350).  d_rgba: H·W float4 (row 0 = bottom);
 * d_out: H·W·4 bytes, row 0 = top.  A NaN is stored as 0, as anything not greater than 0 is; +inf as 255 (rm_frames_to_rgba8
 * and rm_tiles_to_rgba8 convert the same way).
 */
int rm_frame_to_rgba8(const float *d_rgba, uint8_t *d_out, int W, int H, void *stream);
/*
 * rm_frames_to_rgba8 — rm_frame_to_rgba8 of numFrames frames in one launch.  Frame f is read from d_rgba + f·H·W·4 floats (rows
 * bottom-up, as rm_render_batch and rm_post_process_batch write it) and written to d_out + f·H·W·4 bytes, flipped within itself
 * (row 0 = the frame's top); every frame is bit-identical to rm_frame_to_rgba8 of that frame.  numFrames == 0: RM_OK, nothing
 * written.  RM_ERR_INVALID_ARGUMENT: numFrames < 0, null d_rgba / d_out, W or H <= 0, a pointer that is not device memory;
 * RM_ERR_CAPACITY: numFrames > RM_MAX_BATCH_FRAMES.
 */
int rm_frames_to_rgba8(const float *d_rgba, uint8_t *d_out, int W, int H, int numFrames, void *stream);

/* ---- post passes (src/realtimerender.cpp:78-165; resources/blur.frag, hdr.frag, fxaa.frag) ------------------ */
/* Settings surface — src/settings.h:37-41. */
typedef struct RmPostSettings {
  int32_t enableFXAA, enableGammaCorrection, enableHDR, enableBloom;
  float exposure;
} RmPostSettings;
/*
 * rm_post_process — what Realtime::rayMarch() does after the draw call: applyLightEffects() (bloom = 10 ping-pong
 * passes of a separable 9-tap Gaussian over BrightColor, of which the reference composites the 9th; then gamma
 * 1/2.2, or 1−exp(−(colour+bloom)·exposure)) and applyFXAA().  Storage formats are the reference's: the HDR /
 * bright / ping-pong targets are RGBA16F (values are rounded to binary16 between passes), the FXAA source is
 * RGBA8 sampled with GL_LINEAR / GL_REPEAT.  d_frag, d_bright (may be NULL without bloom) and d_out are H·W
 * float4, row 0 = bottom; d_out receives the colour the 8-bit default framebuffer would quantise
 * (rm_frame_to_rgba8 does that).  Uses a grow-only per-stream workspace of 20 B/pixel.  Non-finite and negative inputs have
 * defined results: a NaN that reaches the 8-bit FXAA source is stored as 0.
 */
int rm_post_process(const float *d_frag, const float *d_bright, float *d_out, int W, int H, const RmPostSettings *ps,
                    void *stream);
/*
 * rm_post_process_batch — rm_post_process of numFrames frames (an exported sequence: rm_render_batch's output feeds straight
 * in).  Frame f sits at + f·H·W·4 floats in d_frag, d_bright and d_out, rows bottom-up.  ps holds numPost entries: numPost == 1
 * applies ps[0] to every frame, numPost == numFrames gives frame f ps[f].  The four enable flags must be the same in every
 * entry; exposure may differ per frame (an exposure fade).  Every output frame is bit-identical to rm_post_process of that frame
 * with its settings.  d_out == d_frag (the whole batch in place) is allowed, any other overlap is undefined; d_bright may be
 * NULL without bloom.  Asynchronous on `stream`; ps is copied before return.
 * The frames go through the passes in chunks of k = min(64, numFrames, max(1, cap / (20·W·H))) frames, one launch per pass
 * and chunk, with the chunk's images in the stream's post workspace (20 B/pixel/frame); cap is the rm_set_workspace_limit
 * value when one is set, 256 MiB otherwise.  A single frame that exceeds a set limit fails with RM_ERR_DEVICE as in
 * rm_post_process.
 * numFrames == 0: RM_OK, nothing written.  RM_ERR_INVALID_ARGUMENT: numFrames < 0, numPost neither 1 nor numFrames, the enable
 * flags differ between entries of ps, null d_frag / d_out / ps, bloom without d_bright, W or H <= 0, a pointer that is not
 * device memory; RM_ERR_CAPACITY: numFrames > RM_MAX_BATCH_FRAMES.  All but the last are checked before any HIP call.
 */
int rm_post_process_batch(const float *d_frag, const float *d_bright, float *d_out, int W, int H, int numFrames,
                          const RmPostSettings *ps, int numPost, void *stream);

/* ---- math spec probes (tests only: evaluate the device implementation of one rm_math function
 *      element-wise so it can be compared bit-for-bit with the oracle) ---------------------------- */
enum { RM_FN_SIN = 0, RM_FN_COS, RM_FN_ACOS, RM_FN_ATAN2, RM_FN_LOG2, RM_FN_EXP2, RM_FN_POW, RM_FN_SQRT,
       RM_FN_DIV, RM_FN_PNOISE3, RM_FN_ASIN, RM_FN_Q16 /* round to binary16 and back */,
       RM_FN_SQRT_FAST /* device-only variant of sqrt, must equal RM_FN_SQRT bit for bit */,
       RM_FN_DIVR /* x · RN(1/y), the contract's hot-path quotient */, RM_FN_RCP /* device form of 1.0f / x */,
       RM_FN_SMOOTHSTEP /* smoothstep(x, y, z) */, RM_FN_MIN, RM_FN_MAX, RM_FN_FRACT,
       RM_FN_MEDIAN_ABS /* device only: v_med3_f32(|x|, |y|, |z|), the Menger level's spelling of min(max(x,y), min(max(y,z), max(z,x))) */,
       RM_FN_COUNT };
int rm_probe_math(int fn, const float *d_x, const float *d_y, const float *d_z, float *d_out, int n,
                  void *stream);
/* Evaluate sdScene (frag:1406-1430) at n world-space points: d_out[4n] = (minD, minObjIdx, trap.y, trap.z). */
int rm_probe_sdscene(const RmObject *objs, int numObjects, const RmGlobals *g, const RmSettings *s,
                     const float *d_pts, float *d_out, int n, void *stream);
/* Evaluate one of the production instantiations of the scene evaluator at n world-space points (tests only).
 * bulbClass: 0 the table walk, 1 the single-Mandelbulb class in its general form, 2 in its plain form; count: the work-counter
 * mode (0, 1, 2); trap: 0 none, 1 the shader's orbit trap, 2 the sponge's .z alone; skip / track: the table walk's pass-over
 * test and its runner-up bound; one >= 0: the march's single-object fast path on object `one` (a primitive) instead of the walk.
 * Only the combinations that production kernels instantiate are accepted:
 *   table walk:  trap 0 / 1 with skip = track = 0, and with skip = track = 1 when count != 1; trap 0 with skip = 1, track = 0
 *                when count != 1; trap 2 with count 0, track 0, skip 0 / 1;
 *   bulbClass 1: trap 0 / 1, count 0 / 1 / 2, skip = track = 0;   bulbClass 2: trap 0 / 1, count 0, skip = track = 0;
 *   one >= 0:    table walk, count 0 / 2, trap 0 / 1, skip = track = 1 (the march's instantiations that it stands in for).
 * A bulb class needs a table of one Mandelbulb (bulbClass 2 also one that the plain form accepts); `one` must name a primitive.
 * Anything else returns RM_ERR_INVALID_ARGUMENT before any HIP call.
 * d_ub: per point, the upper bound of the minimum handed to the evaluation (only read with skip); NULL = +inf.
 * d_out[8n] = (d, idx, trap.x, trap.y, trap.z, trap.w, second (+inf without track), shapes evaluated (0 with count 0)).
 * Point i runs on lane i % 64 of wave i / 64 (the evaluator's wave-uniform choices see exactly those 64 points; the last wave
 * may be partial). */
int rm_probe_sdscene_variant(const RmObject *objs, int numObjects, const RmGlobals *g, const RmSettings *s, int bulbClass,
                             int count, int trap, int skip, int track, int one, const float *d_pts, const float *d_ub,
                             float *d_out, int n, void *stream);
/* The four Perlin samples behind bumpNormal(n, p, 10, 2) at n world-space points, from the device function the production
 * kernels call for them (tests only).  d_pts[3n]: the positions; d_out[4n] = (nv, g0, g1, g2) with ps = 10 · p, nv = pnoise(ps)
 * and gk = pnoise(ps + 0.1 · e_k) − nv: the values before bumpNormal's normalize(n + 2 · g).  The function shares the noise
 * lattice of the base sample with an offset sample when every lane of the wave stays in its cell on that axis, and the result
 * is the same bits either way.  Point i runs on lane i % 64 of wave i / 64 (that choice sees exactly those 64 points; the last
 * wave may be partial).  n == 0: RM_OK, nothing written.  RM_ERR_INVALID_ARGUMENT: n < 0, a null pointer or one that is not
 * device memory. */
int rm_probe_bump(const float *d_pts, float *d_out, int n, void *stream);
/* The cull end of a hard-shadow ray as the single-Mandelbulb kernels' shadow pool computes it when it hands the ray out (tests
 * only): for n shadow origins d_pts[3n] and directional light `light` of the table, with march end `far`,
 * d_out[8n] = (end, own as 0 / 1) from the light's staged constants (rm_debug_light_prep) and the per-pixel part alone, then
 * (end, own) from the whole computation with the direction normalised on the device, then that direction xyz, then 0.  The two
 * pairs must be equal bit for bit, and the direction equal to the staged one.  bulbClass: 1 the general form, 2 the plain form
 * (a table rm_debug_bulb_plain accepts), which takes the origin for its object-space image unless an origin of the wave is not
 * finite.  Point i runs on lane i % 64 of wave i / 64 (that choice sees exactly those 64 origins; the last wave may be partial).
 * n == 0: RM_OK, nothing written.  RM_ERR_INVALID_ARGUMENT before any HIP call: a table that is not one Mandelbulb, a plain
 * request for a table that is not plain, `light` out of range or not directional, n < 0, a null pointer or one that is not device
 * memory; rm_render's checks of the tables apply. */
int rm_probe_pool_cull(const RmObject *objs, int numObjects, const RmLight *lights, int numLights, const RmGlobals *g,
                       const RmSettings *s, int bulbClass, int light, float far, const float *d_pts, float *d_out, int n, void *stream);

/* ---- host side kept from the reference: scenefile loader, camera, Settings -------------------- */
/* Settings surface — src/settings.h:19-55 (render-relevant fields only). */
typedef struct RmHostSettings {
  int32_t screenWidth, screenHeight; /* settings.h:21-22 */
  float nearPlane, farPlane;         /* settings.h:28-29 (GUI defaults 0.1 / 100, mainwindow.cpp:129-130) */
  int32_t twoDSpace;
  int32_t enableSoftShadow, enableReflection, enableRefraction, enableAmbientOcculusion;
  float power;                       /* settings.h:47 */
  float juliaSeed[2];                /* settings.h:48 */
} RmHostSettings;
void rm_host_settings_default(RmHostSettings *s);

/* Camera — src/camera/camera.cpp:8-34 (initializeCamera), :74-97 (view), :105-133 (proj). */
typedef struct RmCameraData {
  float pos[4], look[4], up[4]; /* SceneCameraData, scenedata.h:110-120 */
  float heightAngle;            /* radians */
} RmCameraData;
int rm_camera_build(const RmCameraData *cd, int W, int H, float nearPlane, float farPlane,
                    float view[16], float proj[16], RmCamera *out);
/* The n cameras of a thin lens, for rm_render_accumulated (no reference counterpart).  out[0] is rm_camera_build(cd, …) exactly: the
 * pinhole at the lens centre.  out[k], k >= 1, is rm_camera_build of a copy of cd whose pos is shifted on the lens disc by
 * lensRadius · r_k · (cos θ_k · right + sin θ_k · trueUp), r_k = sqrt(k / (n − 1)), θ_k = k · π(3 − √5) (the golden-angle spiral:
 * equal areas per sample, the last on the rim), and whose look points from the shifted position at the focus point
 * pos + focusDistance · normalize(look); right and trueUp are the camera's own axes (u and v of camera.cpp:8-34).  Everything up to
 * the shifted pos and look is computed in double and rounded once to float.  A point at focusDistance along the view direction
 * projects to the same pixel in every sample; everything nearer or farther spreads over a disc.  A sample whose shift rounds to nothing
 * (lensRadius = 0: every one) is out[0] bit for bit.  Both lengths are in world units.  RM_ERR_INVALID_ARGUMENT: n < 1, lensRadius negative or not finite, focusDistance not
 * positive or not finite, null cd / out, and what rm_camera_build refuses. */
int rm_camera_lens_samples(const RmCameraData *cd, int W, int H, float nearPlane, float farPlane, float lensRadius,
                           float focusDistance, int n, RmCamera *out);
/* An object moved by t in world space, for the object tables of rm_render_animated (no reference counterpart): *out is *in with
 * invModel' = invModel · T(−t), T the translation matrix — the fourth column becomes −t[0]·col0 − t[1]·col1 − t[2]·col2 + col3,
 * computed in double and rounded once to float; every other field is copied.  t = 0 returns *in bit for bit.  in and out may be the
 * same object.  RM_ERR_INVALID_ARGUMENT: a null pointer or a t that is not finite. */
int rm_object_translated(const RmObject *in, const float t[3], RmObject *out);

/* Opaque parsed scene — SceneParser::parse (src/utils/sceneparser.cpp:117-133) +
 * RayMarchScene::initScene (src/raymarch/raymarchscene.cpp:104-134). */
typedef struct RmScene RmScene;
int rm_scene_load(const char *path, RmScene **out);
int rm_scene_load_string(const char *json, RmScene **out);
void rm_scene_free(RmScene *scene);
int rm_scene_num_objects(const RmScene *scene);
int rm_scene_num_lights(const RmScene *scene);
/* Pointers stay valid until rm_scene_free. */
const RmObject *rm_scene_objects(const RmScene *scene);
const RmLight *rm_scene_lights(const RmScene *scene);
int rm_scene_globals(const RmScene *scene, const RmHostSettings *hs, RmGlobals *out);
int rm_scene_camera_data(const RmScene *scene, RmCameraData *out);
/* The scenefile's cameraData.aperture and cameraData.focalLength (scenedata.h:117-118, "Only applicable for depth of field"), 0 for
 * a field the file does not have.  The reference parses both and gives them no meaning — no shader reads them; this library reads
 * aperture as the radius of the lens and focalLength as the distance to the plane in focus, both in world units: the lensRadius and
 * focusDistance of rm_camera_lens_samples. */
int rm_scene_camera_lens(const RmScene *scene, float *aperture, float *focalLength);
/* Texture file referenced by object i, or NULL; load it with rm_image_load(path, 1, …) into RmResources.textures[texLoc]. */
const char *rm_scene_object_texture(const RmScene *scene, int i);

/* Image file → RGBA8 (stands in for QImage::load + convertToFormat(RGBA8888) + mirrored(), raymarchscene.cpp:198-209).
 * PNG (8/16-bit grey, grey+alpha, RGB, RGBA, palette; non-interlaced) and baseline JPEG (grayscale or YCbCr, 4:4:4 /
 * 4:2:2 / 4:2:0; decoded with libjpeg's default arithmetic — islow IDCT, fancy upsampling — so the pixels equal
 * QImage's) and the first frame of a GIF.  Other formats, progressive JPEG: RM_ERR_UNSUPPORTED.  flipVertical = 1 gives the bottom-up
 * rows the renderer expects.  *outPixels is malloc'ed host memory of w·h·4 bytes; free with rm_image_free. */
int rm_image_load(const char *path, int flipVertical, uint8_t **outPixels, int *w, int *h);
void rm_image_free(uint8_t *pixels);

/* Sky-box selection of the GUI (settings.idxSkyBox → RayMarchScene::getCubeMapWithType, raymarchscene.cpp:50-86;
 * enum CUBEMAP, scenedata.h:43-48): path of face `face` (0..5, the order of RmResources.skybox) of cube map `which`
 * (1 BEACH, 2 NIGHTSKY, 3 ISLAND) relative to the scenefiles directory, or NULL.  Reproduced as written, including the
 * NIGHTSKY list naming −x before +x and −y before +y.  Load each with rm_image_load(path, 1, …) as initCubeMap does. */
const char *rm_skybox_face_path(int which, int face);

/* PNG writer for RGBA8 rows (top row first) — stands in for QImage::save (realtime.cpp:346). */
int rm_write_png(const char *path, const uint8_t *rgba, int W, int H);
/* PLY writer for the mesh of rm_sdf_mesh, copied to host memory (no reference counterpart): binary little-endian, `element vertex`
 * with float x, y, z (the fourth float of a vertex is not written) and, with rgb (3 bytes per vertex, may be NULL), uchar red,
 * green, blue; `element face` with `property list uchar int vertex_indices`, four indices per face.  numVertices or numQuads may be
 * 0 (its array is then not read).  RM_ERR_INVALID_ARGUMENT: a null path, a negative count, a null array with a positive count, a
 * quad that names a vertex outside 0 … numVertices − 1 (nothing is written then); RM_ERR_IO: the file cannot be opened or written. */
int rm_write_ply(const char *path, const float *vertices4, int numVertices, const int32_t *quads4, int numQuads,
                 const uint8_t *rgb /* may be NULL, 3 per vertex */);
/* rm_write_ply with vertex normals: with normals4 (4 floats per vertex — RmSurfacePoint's first four, or any float4 array —, the
 * fourth not written; may be NULL) `property float nx`, `ny`, `nz` follow z, ahead of the colour.  With normals4 == NULL the file is
 * rm_write_ply's, byte for byte; the statuses are rm_write_ply's. */
int rm_write_ply_ex(const char *path, const float *vertices4, int numVertices, const int32_t *quads4, int numQuads,
                    const uint8_t *rgb /* may be NULL */, const float *normals4 /* may be NULL; 4 floats per vertex, the fourth not written */);

#ifdef __cplusplus
}
#endif
#endif /* RAYMARCHER_AMD_H */
