// rm_launch.h — what the launcher (rm_launcher.hip) hands the launch functions of the kernels (rm_kernels.hip; declared in
// rm_internal.h): the arguments every render launch of a frame shares and the plans of its tile order, light split and
// wavefront pipeline; and what it lends the query entry points (rm_queries.hip): the one-block staging call and the shared checks.
#pragma once
#include <hip/hip_runtime.h>

#include <functional>

#include "rm_scene_block.h"
#include "rm_wavefront.h"

namespace rm {

// What every render launch of a frame shares.
struct RenderLaunch {
  SceneBlock *sb; RowMap map; int W, H, nRows; float4 *o, *b; unsigned long long *dc;  // the render kernels' arguments
  hipStream_t stream; dim3 grid, block;
};

// Tile order ("tile order" in rm_kernels.hip): 0 raster order, 1 feedback — tiles start heaviest-first by the costs the previous frame of this
// size on this stream recorded.  The plan of one frame, and its carve of the stream's tile-order workspace.
struct TileOrderPlan {
  bool ordered = false, byCost = false, byGeom = false, lastSort = false, settled = false;
  bool combine = false;  // byGeom: the estimates take in the stale costs of the previous picture of this size
  int ringLog2 = 16, dilate = 0;  // byGeom: tile_geom_kernel's cost of a silhouette tile and its reach into the stale costs (RM_GEOM_*)
  uint32_t *cost = nullptr, *hist = nullptr, *cost2 = nullptr;
  int32_t *order = nullptr;
  bool sorts() const { return (byCost || byGeom) && !settled; }  // the ordering launches run ahead of the render
};

// The light split of one launch (plan_light_split in rm_launcher.hip has the reasoning).
struct SplitPlan {
  int tiles = 0;        // the split tiles of this launch, 0: a plain launch
  float *store = nullptr;
  int timedSlot = -1;   // the tuner's timing slot for this launch
};

// The wavefront pipeline's records (rm_wavefront.hip.h), carved out of the stream's workspace by the launcher.
struct WfWs {
  uint32_t *counters;  // [WF_STRIDE·g + …]: source cursor, hit slots reserved, shadow-ray cursor, rays appended for g + 1
  float4 *rayO[2];     // rays of generation g >= 1 live in buffer g & 1: (origin, path id bits) …
  float4 *rayD[2];     // … (direction, unused)
  int4 *hit;           // per hit slot: (src = pixel index (g = 0) or ray index; < 0 = hole, bits of res.d, object, bits of trap.z)
  float4 *surfP;       // (p, ambient occlusion)
  float4 *surfN;       // (bumped normal, unused)
  float *shadow;       // [light·cap + hit slot]: penumbra factor of a ray that missed, kWfShadowHit of one that hit
  int2 *pathPix;       // paths are indexed by the generation-0 hit slot: (pixel index, object of the primary hit)
  float4 *pathA;       // (phong.xyz, refl.w)
  float4 *pathB;       // (refl.xyz, fil.x)
  float2 *pathC;       // (fil.y, fil.z)
  uint32_t cap;        // hit-slot capacity
};

// The wavefront pipeline's launch: whether this frame takes it, its persistent waves, chunk sizes and records.
struct Wavefront {
  bool on = false;
  WfWs ws{};
  int primaryWaves = 0, shadowWaves = 0, flush = 16;
  uint32_t slotChunk = 0, maxChunk = 0, rayChunk = 0, pixelChunk = 0;
};

// ---- what the launcher lends the query entry points (rm_queries.hip) -----------------------------------------------------------
// "One block, one launch": the description of a call that stages ONE scene block of one table and launches behind it.
struct BlockCall {
  const RmObject *objs; int numObjects; const RmGlobals *g; const RmSettings *s;
  hipStream_t stream;
  int path;                         // what rm_debug_last_path reports behind the launch
  const RmCamera *cam = nullptr;    // null: a camera of zeros
  const RmLight *lights = nullptr; int numLights = 0;
  const RmResources *res = nullptr; // null: none
  bool singleFrameRing = false;     // the slot's ring: the batch ring, or (the probes) the ring of single frames
  bool timed = true;                // false (the probes): no timing stamps, no path, only the slot's event follows the launch
  size_t workspaceBytes = 0;        // not 0: that much of the stream's kWsBlocks workspace, taken under the device's lock ahead of the staging
  void (*afterFill)(SceneBlock *host) = nullptr;  // the occlusion mode's own staged fields (rm_trace_rays); not a second fill
};
// The launch behind the staged block (device and pinned host copy) with the call's workspace, or null: an rm_status.
using BlockLaunch = std::function<int(const SceneBlock *dev, const SceneBlock *host, void *workspace)>;
// The device and its lock, the workspace, a slot of the ring filled by fill_frames and uploaded, the timing's start, the launch,
// then the timing's end, the path and the slot's event (rm_launcher.hip).
int stage_block_launch(const BlockCall &c, const BlockLaunch &launch);

// The checks the launcher's own entry points share with the queries: a scene without resources, the pointers of a call's
// resources and outputs, and the refusals of the entry points that are defined by the object table alone, each with the entry
// point's own text.
extern const RmResources kNoResources;
int check_device_pointers(const RmResources &res, const float *d_rgba, const float *d_bright);
int refuse_layers(const RmSettings *s, const char *text);
int refuse_two_d(const RmGlobals *g, const char *text);
int check_image_width(int imageWidth);

}  // namespace rm
