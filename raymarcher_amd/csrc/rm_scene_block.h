// rm_scene_block.h — what the host and the device share of a launch: the constant block of a frame (SceneBlock, with the
// EvalRecord of each object) and the row map.  Plain C++: the host-only scene prep (rm_frame.cpp) fills these, the launcher
// (rm_launcher.hip) uploads them, the device code (rm_device.hip.h) reads them.
#ifndef RM_SCENE_BLOCK_H  // a guard, not #pragma once: the header also compiles on its own (g++ -fsyntax-only)
#define RM_SCENE_BLOCK_H
#include "../../include/raymarcher_amd.h"
#include "rm_internal.h"

namespace rm {

// Everything a frame needs, in one constant block (filled by fill_frames in rm_frame.cpp, uploaded once per launch by the launcher).
struct EvalRecord {
  float m[12];  // invModel[0..2], [4..6], [8..10], [12..14]
  float scaleFactor;
  int32_t type;
  // object-space bound for the table walk's skip test: the unit shape lies inside the ball |p| <= boundR (sdMatch's sizes,
  // +inf for types without one), so its distance value is >= (|p_object| − boundR)·scaleFactor; invScale = 1 / scaleFactor
  float invScale, boundR;
};
static_assert(sizeof(EvalRecord) == 64, "one cache line");
// What the bulb kernels' shadow pool (rm_device.hip.h: renderPooled, shadowPool, hardLightSum) would recompute from a light and
// the single Mandelbulb's transform for every ray: L = normalize(−dir) of a directional light with the contract's dot, sqrt_ and
// rcp_; pd = invModel·L (the 3×3 part, bulbCullEnd's fma nesting) and a = dot(pd, pd).  Filled on the host by scene_light_prep
// (rm_frame.cpp) with the same bits the device computes: correctly rounded sqrtf and 1.0f / x, fmaf where the device writes fma.
// Zeros for a light of another type; pd and a are read only in the single-bulb classes.
struct LightPrep {
  float L[3], pd[3], a, pad;
};
static_assert(sizeof(LightPrep) == 32, "eight words per light: two 16-byte LDS reads");
struct SceneBlock {
  RmCamera cam;
  RmGlobals g;
  RmSettings s;
  int32_t numObjects;
  int32_t numLights;
  RmObject objs[RM_MAX_OBJECTS];
  RmLight lights[RM_MAX_LIGHTS];
  LightPrep lightPrep[RM_MAX_LIGHTS];  // per-light constants of the shadow pool, from lights[] and objs[0] (scene_light_prep)
  RmTexture tex[RM_MAX_TEXTURES];  // device pixel pointers
  int32_t numTextures;
  RmTexture noise;                 // `noise` (night sky, sea)
  RmTexture skybox[6];             // cube-map faces +X,-X,+Y,-Y,+Z,-Z
  const uint8_t *ltc1, *ltc2;      // RM_LTC_SIZE² RGBA8 tables of the area lights
  // World-space ball outside which no object can be hit (computed by the launcher, see scene_cull_ball); cullOk = 0
  // when the scene holds an object without a known bound.
  // What an evaluation reads of an object, packed into one 64-byte line (ONE s_load_dwordx16 instead of seven scattered
  // loads from RmObject): the three rows of invModel that sdScene uses, scaleFactor, type.  Filled by the launcher.
  alignas(64) EvalRecord evalRec[RM_MAX_OBJECTS];
  // nearClip / farClip at the corners of the full-screen quad, per triangle: [below / above the TL-BR diagonal][near, far]
  // [P0, P1 − P0, P2 − P0][xyzw]; filled by the launcher (ray_planes), interpolated per pixel by primaryRay.
  float rayPlane[2][2][3][4];
  float cullC[3];
  float cullR2;
  float cullR2Soft;  // larger ball for soft-shadow rays (0 = none): beyond it 8·d/t >= 1, so the penumbra min() is settled
  int32_t cullOk;
  int32_t cullOneOk;  // 1 = every object is a primitive (cube … rectangle): the march loops may take the single-object fast path
  // 1 = the single-Mandelbulb class in its plain form (bulb_plain in rm_frame.cpp): invModel 1 on the diagonal and ±0
  // elsewhere, scaleFactor exactly 1, power 8, no Julia seed.  The launcher then runs the kBulbPlain render kernel.
  int32_t bulbPlain;
  float cullLip;  // Lipschitz bound of every object's distance value per unit of world length (+inf with a fractal in the table)
  float cullLo[3], cullHi[3];  // axis-aligned box with the same property (see scene_cull_ball); cullBoxOk = 0: none
  int32_t cullBoxOk;
  // Shape of a wave's pixel tile: 2^tileShift pixels wide, 64 >> tileShift tall (3 = 8×8, the default; 2 = 4 wide × 16 tall,
  // which the launcher's tuner picks for pictures it measures faster that way: rm_launcher.hip, "tile shape").  Same pixels.
  int32_t tileShift;
  // World-space bounding ball of every object (centre xyz, radius; filled by scene_cull_ball with the balls it derives anyway),
  // objBallOk = 1 when every object has one: tile_geom_kernel classifies the tiles of a frame WITHOUT cost history by their
  // centre ray's closest approach to these balls (rm_kernels.hip, "tile order").  Never read by the render kernels.
  float objBall[RM_MAX_OBJECTS][4];
  int32_t objBallOk;
  // Launch order of the workgroups (see rm_kernels.hip, "tile order"): workgroup b renders tile tileOrder[b] (a permutation
  // of 0..tileCount-1, heaviest tiles first) or tile b if null; tileCost (or null) accumulates every tile's shader-cycle cost.
  const int32_t *tileOrder;
  uint32_t *tileCost;
  int32_t tileCount;
  // "Light split" (rm_launcher.hip, plan_light_split; render_kernel's SPLIT): the first splitTiles tiles of tileOrder — the heaviest of a settled picture — are rendered by
  // numLights workgroups each, one shadow march per pixel apiece, in the same launch as every other tile; the last of a tile's
  // workgroups to arrive finishes the tile from the stored results instead of marching.  splitStore holds splitTiles arrival
  // counters, padded to 64 words, then splitTiles·64·(2·numLights + 6) floats: per tile and pixel numLights × (object bits,
  // penumbra / distance) and the primary march's result (6 words).  The launcher zeroes the counters before every split launch.
  // 0 / null otherwise.
  int32_t splitTiles;
  float *splitStore;
  // Uniforms of sdMengerSponge's prologue (frag:1052-1053: ani = smoothstep(−0.2, 0.2, −cos(0.5·iTime)), off = 1.5·sin(0.01·iTime)),
  // evaluated ONCE per frame of a launch by scene_prep_batch_kernel with the contract's own sin / cos instead of once per evaluation
  // per lane (≈45 of the ≈230 vector instructions of a 5-level evaluation); only read when the table holds a Menger sponge.
  float mengerAni, mengerOff;
  // The block's index in its slot (upload_frames): a production render kernel writes its frame from out + frame·nRows·W.
  int32_t frame;
};

// Which frame row a launch's local row r is: a plain row range (numShards = 1) or the row tiles of one shard of a multi-GPU
// frame (tiles of tileRows rows dealt round-robin, include/raymarcher_amd.h rm_render_tiles).
struct RowMap {
  int rowBegin, tileRows, shard, numShards;
  int relief;  // the partition's root relief (rm_internal.h: 0 = tile t belongs to shard t mod numShards)
  __host__ __device__ int frameRow(int r) const {
    return rowBegin + tile_of(shard, r / tileRows, numShards, relief) * tileRows + (r % tileRows);
  }
};
static_assert(sizeof(SceneBlock) == 9984, "host and device agree on the block's layout");

// rm_render_animated: one bit per scene block of a call, beside the blocks (a kernel argument of render_anim_kernel, rm_animate.hip).
// Bit b set: block b's object table differs from block b − 1's, so a workgroup that walks from one to the other stages it anew.
struct RestageBits {
  uint32_t w[RM_MAX_BATCH_FRAMES / 32];
  void set(int b) { w[b >> 5] |= 1u << (b & 31); }
};

}  // namespace rm
#endif  // RM_SCENE_BLOCK_H
