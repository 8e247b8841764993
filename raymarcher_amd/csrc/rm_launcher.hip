// rm_launcher.hip — the launcher of the per-pixel raymarch and the C ABI (gfx950 only): per-device and per-stream state (scene
// block rings, tuners, workspaces, tile-order history), the plan of a launch, the single-frame and multi-frame launch paths, the
// rm_render* entry points, the conversions, timing and debug entries, and stage_block_launch, the one staging call of the query
// entry points (rays, points, lattices, probes: rm_queries.hip).  Host code only: the kernels and the functions that launch them are
// in rm_kernels.hip and its sibling translation units (declared in rm_internal.h), the scene prep that needs no GPU in rm_frame.cpp.
#include <hip/hip_runtime.h>

#include <atomic>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

#include "rm_internal.h"
#include "rm_frame.h"
#include "rm_launch.h"

namespace rm {

bool device_accessible(const void *p) {
  hipPointerAttribute_t a{};
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();  // unknown (plain host) pointer: clear the sticky error
    return false;
  }
  return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged || a.type == hipMemoryTypeHost;  // Host = pinned
}
int require_device_pointers(std::initializer_list<std::pair<const char *, const void *>> ptrs) {
  for (const auto &p : ptrs)
    if (p.second && !device_accessible(p.second)) {
      set_error(std::string(p.first) + " is not device-accessible memory");
      return RM_ERR_INVALID_ARGUMENT;
    }
  return RM_OK;
}

// Block = 4 waves side by side, each wave an 8×8 pixel tile → the block covers 32×8 pixels.
#ifndef RM_TILE_W
#define RM_TILE_W 8   // pixels per wave tile, horizontally (RM_TILE_W × RM_TILE_H = 64)
#endif
static_assert(RM_TILE_W == 4 || RM_TILE_W == 8 || RM_TILE_W == 16, "tile width: 4, 8 or 16 pixels");

// ---- launcher state -------------------------------------------------------------------------------------
// Everything is per device: a host thread driving GPU k never takes a lock that a thread driving GPU j holds, and no lock
// is held across a blocking HIP call on the launch path.  Scratch memory is per (device, stream): two calls on different
// streams of one device may overlap on the GPU, so they must not share ping-pong buffers or hit lists.
namespace {
struct TileOrderState {
  int tileCount = 0, W = 0, nRows = 0, nw = 0, tileShift = 3;
  void *mem = nullptr;
  unsigned long long sceneKey = 0;  // hash of the scene + camera + row map of the frame that recorded the costs in `mem`
  int sorts = 0;                     // consecutive frames of that picture whose order came from measured costs
};
// "Tile shape": which of the two tile shapes a picture renders faster with is scene-dependent (upright objects: 4 wide × 16 tall
// tiles straddle fewer vertical silhouettes, so whole waves agree on the table walk's shortcuts more often — C2 at 1080p 0.866 →
// 0.792 ms — while reflections_complex.json loses 5 % that way; profiles/r04_m_tile_shape.txt).  So the launcher MEASURES, per
// stream and picture: frames 0-1 of a picture run 8×8 (frame 1, ordered by frame 0's costs, is timed with HIP events), frames 2-3
// run 4×16 (frame 3 timed), frames 4-7 repeat that (clocks ramp up over a process's first frames: one round would favour the later
// candidate), and from then on the shape with the smaller best time is used.  Same pixels whatever the shape.  Single-bulb class: 8×8
// always (measured: 4×16 +5 %).  RM_TILE_SHAPE / rm_debug_set_tile_shape: 0 tune, 3 always 8×8, 2 always 4×16.
// "Light split" (launch_render) helps frames that are bound by the life of their heaviest waves when those waves are shadow marches
// (C2 at 1080p: −35 %) and costs others a few per cent (redundant primary marches, cache write-backs: 4K frames +3…+9 %,
// depth_of_field.json +10 %; profiles/r04_s_light_split.md).  So it is MEASURED per stream and settled picture like the tile shape:
// settled frames 0-1 plain (frame 1 timed), 2-3 split (frame 3 timed), then the split stays only if it won by 3 %; plain while the
// timings are outstanding.
// Both are a Tuner: the schedule and the rule of rm_internal.h (tune_schedule, tune_decide) over `rounds` rounds (2 for the tile
// shape, 1 for the light split), timed with HIP events around the render kernel alone.  A decision is published in the device's
// map of that tuner, where the device's other streams adopt it.
using TuneKey = std::tuple<unsigned long long, int, int, int, int>;  // picture, W, nRows and 0, 0 (tile shape) or tile shift, divisor (light split)
using TuneDecisions = std::map<TuneKey, int>;  // decided candidate by key; cleared when it reaches 256 entries
constexpr int kTuneSlots = 4;                  // 2 candidates × up to 2 rounds
struct Tuner {
  TuneKey key;
  int frame = 0;    // frames of this key enqueued so far
  int chosen = -1;  // the decided candidate, -1 while measuring
  hipEvent_t ev[kTuneSlots][2] = {};  // [timing slot][start, stop]
  bool timed[kTuneSlots] = {};
  void drop() {
    for (auto &p : ev) for (auto &e : p) if (e) { (void)hipEventDestroy(e); e = nullptr; }
    for (bool &t : timed) t = false;
  }
  // This frame's candidate and timing slot.  A new key drops the old events and takes over a decision another stream of the
  // device has published; the tuner decides once every slot was recorded and its stop event reports done.
  TuneStep step(const TuneKey &k, int rounds, TuneDecisions &decided) {
    if (key != k) {
      drop();
      key = k; frame = 0; chosen = -1;
      const auto known = decided.find(k);
      if (known != decided.end()) chosen = known->second;
    }
    if (chosen < 0 && frame >= 4 * rounds) {
      bool ready = true;
      for (int i = 0; i < 2 * rounds; i++) ready = ready && timed[i] && hipEventQuery(ev[i][1]) == hipSuccess;
      if (ready) {
        float ms[kTuneSlots] = {};
        bool ok = true;
        for (int i = 0; i < 2 * rounds; i++) ok = ok && hipEventElapsedTime(&ms[i], ev[i][0], ev[i][1]) == hipSuccess;
        chosen = tune_decide(ms, rounds, ok);
        drop();
        if (decided.size() >= 256) decided.clear();
        decided[k] = chosen;
      }
    }
    (void)hipGetLastError();  // hipEventQuery's hipErrorNotReady is not an error
    const TuneStep t = chosen >= 0 ? TuneStep{chosen, -1} : tune_schedule(frame, rounds);
    frame++;
    return t;
  }
  // Events around a timed frame's render kernel.  A slot whose events cannot be created is never recorded (slot = -1): the tuner
  // then stays undecided, on candidate 0, until its key changes.
  int begin(int &slot, hipStream_t stream) {
    if (slot < 0) return RM_OK;
    if (hipEventCreate(&ev[slot][0]) == hipSuccess && hipEventCreate(&ev[slot][1]) == hipSuccess) HIP_OK(hipEventRecord(ev[slot][0], stream));
    else slot = -1;
    return RM_OK;
  }
  int end(int slot, hipStream_t stream) {
    if (slot < 0) return RM_OK;
    HIP_OK(hipEventRecord(ev[slot][1], stream));
    timed[slot] = true;
    return RM_OK;
  }
};
// What the launcher remembers per stream: calls on different streams of one device may overlap on the GPU.
struct StreamState {
  TileOrderState tileOrder;  // what the stream's feedback costs belong to
  Tuner shape, split;        // the tile-shape and light-split tuners
  size_t wfDenied = 0;       // smallest wavefront workspace (bytes) that could not be had on the stream; 0: none was refused
};
struct TimedLaunch { hipEvent_t ev[5]; int n; };  // n = 2 (one stage) or 3 (tile-order sort + render kernel)
// The scene blocks of one launch: `cap` SceneBlocks, contiguous, pinned on the host and on the device.
struct Slot {
  SceneBlock *host = nullptr, *dev = nullptr;
  int cap = 0;
  hipEvent_t done = nullptr;  // recorded behind the slot's last launch
  bool used = false;
};
// A ring of slots (acquire_slot): at most maxSlots, each of at least minCap blocks once allocated.
struct Ring {
  int maxSlots, minCap;
  std::vector<Slot> slots;
  size_t next = 0;
};
struct DeviceState {
  std::mutex mu;                 // guards everything below; held for the host-side enqueue of ONE launch on this device
  Ring frames{64, 1};            // single frames and probes: up to 64 slots of one block
  Ring batches{4, 16};           // rm_render_batch: up to 4 slots of 16 … RM_MAX_BATCH_FRAMES blocks
  unsigned long long *dCounters = nullptr;  // 10 words: evals, iterations, hits, clock stamps (2), span pointer, shades, fbm9, fbmd8, shapes
  std::vector<TimedLaunch> timed;           // rm_set_timing / rm_get_timing, per device
  int numCUs = 0;
  std::map<hipStream_t, StreamState> streams;
  TuneDecisions shapeChoice, splitChoice;  // the tuners' decisions, adopted by the device's other streams
  const int32_t *dbgTileOrder = nullptr;  // rm_debug_set_tile_order (experiments): overrides the modes below
  uint32_t *dbgTileCost = nullptr;
  int dbgTileCount = 0;
  int lastPath = 0;  // rm_debug_last_path: the schedule of the most recent render launch on this device
  int lastSplit = 0; // rm_debug_last_split: tiles that launch rendered one light per workgroup (0: none)
};
std::atomic<int> g_tileOrderMode{-1};  // rm_set_tile_order: -1 = take RM_TILE_ORDER or the default
constexpr int kDefaultTileOrder = 1;
DeviceState g_dev[64];
std::atomic<bool> g_timing{false};
std::atomic<int> g_tileShape{-1};  // rm_debug_set_tile_shape: -1 = the RM_TILE_SHAPE environment variable (default 0 = tune), 0 tune, 3 8×8, 2 4×16
std::atomic<bool> g_lightSplitForce{false};  // rm_debug_set_light_split with a divisor: split without measuring
std::atomic<int> g_lightSplit{-1};  // rm_debug_set_light_split: -1 = the RM_LIGHT_SPLIT environment variable (default 256), 0 off, n: the heaviest 1/n of the tiles
std::atomic<int> g_kernelPath{0};  // rm_set_kernel_path: 0 auto, 1 one lane per pixel, 5 wavefront pipeline

// the device the calling thread has current
int current_device_state(DeviceState **out) {
  int dev = 0;
  HIP_OK(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64) { set_error("device index out of range"); return RM_ERR_DEVICE; }
  *out = &g_dev[dev];
  return RM_OK;
}

void free_slot(Slot &s) {
  if (s.host) (void)hipHostFree(s.host);
  if (s.dev) (void)hipFree(s.dev);
  if (s.done) (void)hipEventDestroy(s.done);
  s = Slot{};
}
// Caller holds the device's lock.  Returns a slot of at least n blocks whose last launch (if any) has finished, so that its pinned
// blocks, whose upload may still be in flight, are never overwritten.  The next slot of the ring if its event has fired; otherwise
// a fresh slot in front of it (ring order) while the ring is below its maximum, so the enqueue path does not block on the GPU
// while it holds the device lock; only at the maximum does it wait for that slot (hipEventSynchronize), which bounds pinned
// memory.  Slots are grow-only: an idle slot of fewer than n blocks is reallocated to the next power of two >= max(n, minCap)
// (a batch slot at most six times over a process; those frees may wait for the device).  A failed allocation leaves an empty
// slot (cap 0), which the next launch that lands on it tries again.
int acquire_slot(Ring &ring, int n, Slot **out) {
  if (ring.slots.empty()) { ring.slots.resize(1); ring.next = 0; }
  Slot *s = &ring.slots[ring.next];
  if (s->used) {
    const hipError_t q = hipEventQuery(s->done);
    if (q == hipErrorNotReady) {
      if ((int)ring.slots.size() < ring.maxSlots) {
        ring.slots.insert(ring.slots.begin() + (long)ring.next, Slot{});
        s = &ring.slots[ring.next];
      } else {
        HIP_OK(hipEventSynchronize(s->done));
      }
    } else if (q != hipSuccess) {
      set_error(std::string("hipEventQuery: ") + hipGetErrorString(q));
      return RM_ERR_DEVICE;
    }
  }
  if (s->cap < n) {
    int cap = ring.minCap;
    while (cap < n) cap *= 2;
    free_slot(*s);
    const size_t bytes = (size_t)cap * sizeof(SceneBlock);
    if (hipHostMalloc(reinterpret_cast<void **>(&s->host), bytes, hipHostMallocDefault) != hipSuccess ||
        hipMalloc(reinterpret_cast<void **>(&s->dev), bytes) != hipSuccess ||
        hipEventCreateWithFlags(&s->done, hipEventDisableTiming) != hipSuccess) {
      (void)hipGetLastError();
      free_slot(*s);
      set_error("allocation of " + std::to_string(bytes) + " bytes of scene blocks failed");
      return RM_ERR_DEVICE;
    }
    s->cap = cap;
  }
  ring.next = (ring.next + 1) % ring.slots.size();
  s->used = true;
  *out = s;
  return RM_OK;
}

// Grow-only scratch memory of one (device, stream, user): see rm_internal.h.
struct WsKey { int dev; hipStream_t stream; int tag; bool operator<(const WsKey &o) const { return std::tie(dev, stream, tag) < std::tie(o.dev, o.stream, o.tag); } };
struct WsBuf { void *mem = nullptr; size_t bytes = 0; };
std::mutex g_wsMu;
std::map<WsKey, WsBuf> g_ws;
}  // namespace

// Largest single workspace buffer the library may allocate (0 = no limit): rm_set_workspace_limit / RM_WF_MAX_WORKSPACE_BYTES.
std::atomic<unsigned long long> g_wsLimit{~0ull};  // ~0 = not set yet: the environment variable decides
unsigned long long workspace_limit() {
  unsigned long long v = g_wsLimit.load();
  if (v == ~0ull) {
    const char *e = std::getenv("RM_WF_MAX_WORKSPACE_BYTES");
    v = e ? std::strtoull(e, nullptr, 10) : 0ull;
    g_wsLimit.store(v);
  }
  return v;
}

int lock_current_device(std::unique_lock<std::mutex> &lock) {
  DeviceState *ds;
  if (int st = current_device_state(&ds)) return st;
  lock = std::unique_lock<std::mutex>(ds->mu);
  return RM_OK;
}

int stream_workspace(int tag, hipStream_t stream, size_t need, void **out) {
  int dev = 0;
  HIP_OK(hipGetDevice(&dev));
  WsBuf *b;
  {
    std::lock_guard<std::mutex> lock(g_wsMu);
    b = &g_ws[WsKey{dev, stream, tag}];  // std::map nodes are stable: the pointer outlives the lock
  }  // and the caller holds the device's launcher lock, which release_workspaces' caller takes before it erases the node
  // only work enqueued on `stream` uses this buffer, and one host thread enqueues on a stream at a time
  if (b->bytes < need) {
    const unsigned long long limit = workspace_limit();
    if (limit && need > limit) {
      set_error("workspace of " + std::to_string(need) + " bytes exceeds the limit of " + std::to_string(limit) + " (rm_set_workspace_limit)");
      return RM_ERR_DEVICE;
    }
    HIP_OK(hipStreamSynchronize(stream));
    if (b->mem) HIP_OK(hipFree(b->mem));
    b->mem = nullptr; b->bytes = 0;
    const hipError_t e = hipMalloc(&b->mem, need);
    if (e != hipSuccess) {
      (void)hipGetLastError();  // an allocation failure is not sticky for the caller: later HIP calls on this thread start clean
      b->mem = nullptr;
      set_error("hipMalloc of a " + std::to_string(need) + "-byte workspace: " + hipGetErrorString(e));
      return RM_ERR_DEVICE;
    }
    b->bytes = need;
  }
  *out = b->mem;
  return RM_OK;
}
// Frees every grow-only buffer of the current device (after the device has drained); rm_release_workspaces.
int release_workspaces(size_t *freedOut) {
  int dev = 0;
  HIP_OK(hipGetDevice(&dev));
  HIP_OK(hipDeviceSynchronize());
  size_t freed = 0;
  std::lock_guard<std::mutex> lock(g_wsMu);
  for (auto it = g_ws.begin(); it != g_ws.end();) {
    if (it->first.dev != dev) { ++it; continue; }
    const WsBuf b = it->second;
    it = g_ws.erase(it);  // before the free: a failure leaves no entry that points at freed memory
    if (b.mem) { HIP_OK(hipFree(b.mem)); freed += b.bytes; }
  }
  if (freedOut) *freedOut = freed;
  return RM_OK;
}

// ---- the checks shared with the query entry points (rm_queries.hip; declared in rm_launch.h) -----------------------------------
int check_device_pointers(const RmResources &res, const float *d_rgba, const float *d_bright) {
  if (int st = require_device_pointers({{"d_rgba", d_rgba}, {"d_bright", d_bright}})) return st;
  for (int i = 0; i < res.numTextures; i++)
    if (int st = require_device_pointers({{"a texture's pixels", res.textures[i].pixels}})) return st;
  if (int st = require_device_pointers({{"RmResources.noise.pixels", res.noise.pixels}})) return st;
  for (int f = 0; f < 6; f++)
    if (int st = require_device_pointers({{"a sky-box face", res.skybox[f].pixels}})) return st;
  return require_device_pointers({{"RmResources.ltc1", res.ltc1}, {"RmResources.ltc2", res.ltc2}});
}
const RmResources kNoResources{};
// The refusals of the entry points that are defined by the object table alone, each with the entry point's own text: the layers
// that may cover the table, and the 2-D mode, which marches no ray.
int refuse_layers(const RmSettings *s, const char *text) {
  if (!(s->features & (RM_FEAT_TERRAIN | RM_FEAT_CLOUD | RM_FEAT_SEA))) return RM_OK;
  set_error(text);
  return RM_ERR_UNSUPPORTED;
}
// The width of the image the rays belong to (rm_shade_rays_layers, rm_trace_rays_layers): checked in every call, whatever the
// feature mask, so that the status does not depend on it.
int check_image_width(int imageWidth) {
  if (imageWidth >= 1) return RM_OK;
  set_error("imageWidth must be at least 1: the width in pixels of the image the rays belong to");
  return RM_ERR_INVALID_ARGUMENT;
}
int refuse_two_d(const RmGlobals *g, const char *text) {
  if (!g->isTwoD) return RM_OK;
  set_error(text);
  return RM_ERR_UNSUPPORTED;
}

namespace {

// The wavefront pipeline's records for `cap` hit slots and `nl` lights, laid out once: into ws from the workspace at mem, or
// measured where mem is null.
size_t wavefront_layout(size_t cap, int nl, void *mem, WfWs *ws) {
  Carve c(mem);
  ws->counters = c.take<uint32_t>(WF_STRIDE * (kWfMaxBounces + 2));
  ws->rayO[0] = c.take<float4>(cap); ws->rayO[1] = c.take<float4>(cap);
  ws->rayD[0] = c.take<float4>(cap); ws->rayD[1] = c.take<float4>(cap);
  ws->hit = c.take<int4>(cap);
  ws->surfP = c.take<float4>(cap);
  ws->surfN = c.take<float4>(cap);
  ws->shadow = c.take<float>(cap * (size_t)(nl > 0 ? nl : 1));
  ws->pathPix = c.take<int2>(cap);
  ws->pathA = c.take<float4>(cap);
  ws->pathB = c.take<float4>(cap);
  ws->pathC = c.take<float2>(cap);
  ws->cap = (uint32_t)cap;
  return c.bytes();
}
size_t wavefront_bytes(size_t cap, int nl) { WfWs unused; return wavefront_layout(cap, nl, nullptr, &unused); }
int wavefront_workspace(size_t cap, int nl, hipStream_t stream, WfWs *ws) {
  void *mem = nullptr;
  if (int st = stream_workspace(kWsWavefront, stream, wavefront_bytes(cap, nl), &mem)) return st;
  wavefront_layout(cap, nl, mem, ws);
  return RM_OK;
}

// The fields of a SceneBlock that the launch decides, the same in every block of the launch (the defaults: raster order, no
// cost feedback, 8×8 tiles, no light split).
struct LaunchFields {
  const int32_t *tileOrder = nullptr;
  uint32_t *tileCost = nullptr;
  int tileCount = 0, tileShift = 3, splitTiles = 0;
  float *splitStore = nullptr;
};
// The upload step: the launch fields into the slot's first n blocks, one copy of them to the device and, when the table holds a
// Menger sponge, each frame's sponge uniforms computed on the device — stream-ordered between the upload and the kernels that
// read the blocks.  mengerAnywhere (rm_render_animated, whose blocks have tables of their own): a block other than the first holds one.
int upload_frames(const Slot &slot, int n, const LaunchFields &lf, hipStream_t stream, bool mengerAnywhere = false) {
  for (int f = 0; f < n; f++) {
    SceneBlock *h = slot.host + f;
    h->tileOrder = lf.tileOrder; h->tileCost = lf.tileCost; h->tileCount = lf.tileCount;
    h->tileShift = lf.tileShift;
    h->splitTiles = lf.splitTiles; h->splitStore = lf.splitStore;
    h->mengerAni = 0.0f; h->mengerOff = 0.0f;
    h->frame = f;
  }
  HIP_OK(hipMemcpyAsync(slot.dev, slot.host, (size_t)n * sizeof(SceneBlock), hipMemcpyHostToDevice, stream));
  bool menger = mengerAnywhere;
  for (int i = 0; i < slot.host->numObjects; i++) menger = menger || slot.host->objs[i].type == RM_MENGERSPONGE;
  if (menger) {
    if (int st = launch_scene_prep(slot.dev, n, stream)) return st;
  }
  return RM_OK;
}

// Settled BEFORE anything else depends on `on`: if the workspace (≈(160 + 4·numLights) B per hit slot, grow-only per (device,
// stream): 5.8 GB for an 8K frame) cannot be had, the auto-selected launch falls back to render_kernel — identical bits, no
// workspace — and only an explicit path-5 request reports the failure.  A (device, stream) that was refused once is not asked
// again for as much or more, so a frame sequence does not pay a failing allocation (and the stream synchronisation in front of
// it) per frame.
int setup_wavefront(DeviceState &ds, StreamState &ss, const FrameClass &fc, const RmObject *objs, int numObjects,
                    int numLights, int W, int nRows, bool tileShard, int pathReq, hipStream_t stream, Wavefront *wf) {
  wf->on = fc.wfOk && (pathReq == 5 || (pathReq == 0 && wavefront_pays(objs, numObjects, fc.wfBounces, (size_t)nRows * W, tileShard)));
  if (!wf->on) return RM_OK;
  static const int perSimd = env_int("RM_WF_WAVES_PER_SIMD", 0), envFlush = env_int("RM_WF_FLUSH", 0),
                   envSlotChunk = env_int("RM_WF_SLOT_CHUNK", 0), envRayChunk = env_int("RM_WF_RAY_CHUNK", 0),
                   envPixelChunk = env_int("RM_WF_PIXEL_CHUNK", 0), envMaxChunk = env_int("RM_WF_MAX_CHUNK", 0);
  // chunk sizes are clamped so that slot and ray ids stay 32-bit
  constexpr int kWfChunkMax = 4096;
  auto clampChunk = [](int v) { return (uint32_t)(v > kWfChunkMax ? kWfChunkMax : v); };
  wf->slotChunk = envSlotChunk >= 64 ? clampChunk(envSlotChunk) : kWfSlotChunk;  // >= 64: one trip's hits fit one fresh chunk
  wf->maxChunk = envMaxChunk > 0 ? clampChunk(envMaxChunk) : 0u;  // 0: fixed chunks (guided chunks measured slower)
  wf->rayChunk = envRayChunk > 0 ? clampChunk(envRayChunk) : wfRayChunk(1);
  wf->pixelChunk = envPixelChunk > 0 ? clampChunk(envPixelChunk) : wfRayChunk(0);
  wf->flush = envFlush > 0 && envFlush <= 64 ? envFlush : 16;
  if (ds.numCUs == 0) {
    int dev = 0;
    hipDeviceProp_t prop;
    HIP_OK(hipGetDevice(&dev));
    HIP_OK(hipGetDeviceProperties(&prop, dev));
    ds.numCUs = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  }
  // persistent waves: as many as are resident at once (4 SIMDs per CU x the kernel's register budget)
  auto waves = [&](int kind) { return ds.numCUs * 4 * (perSimd > 0 && perSimd < wfMarchWaves(kind) ? perSimd : wfMarchWaves(kind)); };
  wf->primaryWaves = waves(0); wf->shadowWaves = waves(2);
  const int marchWaves = wf->shadowWaves > wf->primaryWaves ? wf->shadowWaves : wf->primaryWaves;
  // hit-slot capacity: every ray may hit, plus one partly used chunk of slots per persistent wave
  const size_t cap = (size_t)nRows * W + (size_t)wf->slotChunk * marchWaves;
  // 32-bit ids: hit slots x lights (shadow rays) and the striped cursors' padding (one chunk per stripe) stay below 2^32
  const size_t chunkMax = wf->rayChunk > wf->pixelChunk ? wf->rayChunk : wf->pixelChunk;
  const bool idsFit = (double)(cap + (size_t)kWfStripes * chunkMax) * (numLights > 0 ? numLights : 1) < 4.0e9;
  int wst = RM_ERR_DEVICE;
  const size_t wfBytes = wavefront_bytes(cap, numLights);
  if (!idsFit) set_error("frame too large for the wavefront pipeline's 32-bit ray ids");
  else if (ss.wfDenied != 0 && wfBytes >= ss.wfDenied) set_error("wavefront workspace was refused on this stream before");
  else if ((wst = wavefront_workspace(cap, numLights, stream, &wf->ws)) != RM_OK) ss.wfDenied = wfBytes;
  if (wst != RM_OK) {
    if (pathReq == 5 && idsFit) return wst;  // an explicit request reports the workspace failure; a frame the ids cannot cover "does not apply"
    wf->on = false;
  }
  return RM_OK;
}

// Tile shape ("tile shape" above) as a tile shift: 8×8 unless the tuner is measuring or has chosen 4×16 for this picture on this
// stream.  *timedSlot: the tuner's timing slot for this launch, -1 for none.
constexpr int kDefaultTileShift = (RM_TILE_W == 8) ? 3 : (RM_TILE_W == 4 ? 2 : (RM_TILE_W == 16 ? 4 : 3));
// rm_debug_set_tile_shape / RM_TILE_SHAPE: 0 tune, 2 pinned to 4×16, 3 pinned to 8×8
int tile_shape_request() {
  static const int envShape = env_int("RM_TILE_SHAPE", 0);
  return g_tileShape.load() >= 0 ? g_tileShape.load() : envShape;
}
int tile_shift(DeviceState &ds, StreamState &ss, const FrameClass &fc, bool wavefront, int count, int W, int nRows,
               unsigned long long key, int *timedSlot) {
  *timedSlot = -1;
  const int shapeReq = tile_shape_request();
  const bool bigFrame = (size_t)nRows * W >= (size_t)2048 * 64;
  if ((shapeReq == 2 || shapeReq == 3) && count == 0) return shapeReq;  // the counted / stamped diagnostic builds keep 8×8 (their callers size per-wave arrays by it)
  if (RM_TILE_W == 8 && !fc.bulb && !wavefront && !fc.twoD && count == 0 && bigFrame && !ds.dbgTileOrder && !ds.dbgTileCost) {
    const TuneStep t = ss.shape.step(TuneKey(key, W, nRows, 0, 0), 2, ds.shapeChoice);  // candidate 0 = 8×8, 1 = 4×16
    *timedSlot = t.slot;
    return t.candidate ? 2 : 3;
  }
  return kDefaultTileShift;
}

// The tile-order plan of this frame (TileOrderPlan, rm_launch.h) from the stream's history; "tile order" in rm_kernels.hip.
int plan_tile_order(const DeviceState &ds, StreamState &ss, const FrameClass &fc, bool wavefront, int count, int numObjects, int W,
                    int nRows, int nw, int tileShift, int tileCount, unsigned long long key, hipStream_t stream, TileOrderPlan *p) {
  static const int envOrder = env_int("RM_TILE_ORDER", kDefaultTileOrder);
  const int orderMode = g_tileOrderMode.load() >= 0 ? g_tileOrderMode.load() : envOrder;
  // every class of the one-lane-per-pixel kernel (round 3: the layer and sampler kernels too — area light + point light 1080p
  // 0.80 -> 0.59 ms, textured floor / sky box at 4K 2.5 -> 2.3 ms, terrain + cloud horizon view 4.31 -> 4.04 ms, sea unchanged).
  // Small frames are not worth the two extra launches.
  p->ordered = orderMode > 0 && !wavefront && !fc.twoD && count == 0 && tileCount >= 2048 && !ds.dbgTileOrder && !ds.dbgTileCost;
  if (!p->ordered) return RM_OK;
  void *mem = nullptr;
  if (int st = stream_workspace(kWsTileOrder, stream, (size_t)tileCount * 12 + 256, &mem)) return st;
  p->hist = static_cast<uint32_t *>(mem);
  p->cost = p->hist + 64;
  p->order = reinterpret_cast<int32_t *>(p->cost + tileCount);
  p->cost2 = p->cost + 2 * (size_t)tileCount;  // a new picture's estimates (tile_geom_kernel), so that it can read its neighbours' stale costs
  TileOrderState &ts = ss.tileOrder;
  const TileOrderState now{tileCount, W, nRows, nw, tileShift, mem, key};
  const bool haveCost = ts.tileCount == now.tileCount && ts.W == W && ts.nRows == nRows && ts.nw == nw && ts.tileShift == tileShift && ts.mem == mem;
  if (!haveCost) HIP_OK(hipMemsetAsync(p->cost, 0, (size_t)tileCount * 4, stream));
  const bool samePicture = haveCost && ts.sceneKey == key;
  // A picture that repeats SETTLES: its first frames re-sort by the costs the frame before measured (each under a better order than
  // the last); the kSettle-th such sort keeps its costs (they are the stale costs of whatever picture comes next) and from then on
  // the same order is reused — no ordering launches (memset + two kernels, ≈25 µs a frame: 1 % of the 4K bulb frame, 8 % of its
  // 1/8 shard) and no cost atomics in the render.  RM_TILE_ORDER_SETTLE=0: re-sort every frame (rounds 2-3).
  static const int kSettle = env_int("RM_TILE_ORDER_SETTLE", 3, 0, 1000);
  const int kSettleHold = kSettle + 1;
  const int costSorts = samePicture ? ts.sorts + 1 : 0;  // this frame is the costSorts-th consecutive cost-ordered frame of its picture (0: not cost-ordered)
  ts = now;
  ts.sorts = costSorts > kSettleHold ? kSettleHold : costSorts;
  // Which order this frame's tiles start in: the previous frame's measured costs when it was the same picture; otherwise — no
  // history, or the scene / camera moved — the geometric classification (tile_geom_kernel), where the scene has per-object balls
  // and no procedural layers (their cost is not where the objects are); otherwise raster order.
  p->byCost = samePicture;
  p->lastSort = p->byCost && kSettle > 0 && costSorts == kSettle;
  p->settled = p->byCost && kSettle > 0 && costSorts > kSettle;
  static const int geomMode = env_int("RM_TILE_ORDER_GEOMETRIC", 2);  // 0 off (raster), 1 geometry alone, 2 geometry + stale costs (measured best, default)
  p->byGeom = !samePicture && geomMode != 0 && !fc.envFeatures && numObjects > 0;
  p->combine = geomMode == 2 && haveCost;
  static const int ringLog2 = env_int("RM_GEOM_RING_LOG2", 16, 5, 17), dilate = env_int("RM_GEOM_DILATE", 0, 0, 16);
  p->ringLog2 = ringLog2; p->dilate = dilate;
  return RM_OK;
}

// "Light split": a settled picture of the plain table-walk class (no secondary rays, samplers or layers) with several lights is
// bound by the life of its heaviest waves, and those are whole tiles whose every pixel runs one long shadow march per light back to
// back (C2: 26-40 evaluations of primary march, then three soft-shadow marches of 256 — profiles/r04_r_c2_chain_sim.txt).  The
// first tileCount / kSplitDiv tiles of the settled order are therefore rendered by numLights workgroups each — every one repeats
// the primary march and the surface point and marches ONE light, its result going to memory (the first one's primary result too)
// — and the last of them to arrive finishes the tile from the stored results: surface point, AO and the light sum, no march.  The
// same marches, the same sums in the same order: the same pixels.  Whether it pays is measured per picture (the tuner above).
// RM_LIGHT_SPLIT=0: off; =n: the heaviest 1/n of the tiles.
SplitPlan plan_light_split(DeviceState &ds, StreamState &ss, const FrameClass &fc, const TileOrderPlan &to, int count, int nw,
                            int numLights, int W, int nRows, int tileShift, int tileCount, bool shapeTimed,
                            unsigned long long key, hipStream_t stream) {
  SplitPlan ls;
  static const int envSplitDiv = env_int("RM_LIGHT_SPLIT", 256, 0);
  const int kSplitDiv = g_lightSplit.load() >= 0 ? g_lightSplit.load() : envSplitDiv;  // rm_debug_set_light_split
  if (!to.settled || kSplitDiv <= 0 || fc.bulb || fc.envFeatures || fc.textured || fc.secondary || count != 0 || nw != 1 ||
      numLights < 2 || numLights > RM_MAX_LIGHTS || shapeTimed)
    return ls;
  int splitK = tileCount / kSplitDiv;
  if (splitK > 0 && !g_lightSplitForce.load()) {  // measured, unless a test forces it (rm_debug_set_light_split)
    const TuneStep t = ss.split.step(TuneKey(key, W, nRows, tileShift, kSplitDiv), 1, ds.splitChoice);  // candidate 0 = plain, 1 = split
    ls.timedSlot = t.slot;
    if (!t.candidate) splitK = 0;
  }
  if (splitK > 0) {
    void *mem = nullptr;
    // SceneBlock::splitStore: splitK arrival counters, padded to 64 words, then splitK·64·(2·numLights + 6) floats
    if (stream_workspace(kWsLightSplit, stream, ((((size_t)splitK + 63) & ~(size_t)63) + (size_t)splitK * 64 * (2 * numLights + 6)) * sizeof(float), &mem) == RM_OK) {
      ls.tiles = splitK;
      ls.store = static_cast<float *>(mem);
    }  // no memory for it: the plain launch
  }
  return ls;
}

// rm_set_kernel_path / RM_KERNEL_PATH: 0 = the measured-fastest schedule of the scene's class
int kernel_path_request() {
  static const int envPath = env_int("RM_KERNEL_PATH", 0);
  return g_kernelPath.load() ? g_kernelPath.load() : envPath;
}
// RM_WAVES_PER_BLOCK: 1 (default), 2 or 4 waves per workgroup (launch_render has the measurements)
int waves_per_block() {
  static const int wpb = env_int("RM_WAVES_PER_BLOCK", 0);
  return (wpb == 1 || wpb == 2 || wpb == 4) ? wpb : 1;
}

// rm_set_timing: the events of one launch — one ahead of it, one after the ordering launches if they run, one after the render.
// keep() hands them to the device's list; a launch that fails part-way destroys them on the way out.
struct LaunchTimer {
  TimedLaunch t{};
  hipStream_t stream;
  bool on = g_timing.load(), kept = false;
  explicit LaunchTimer(hipStream_t s) : stream(s) {}
  ~LaunchTimer() { if (!kept) for (int i = 0; i < t.n; i++) (void)hipEventDestroy(t.ev[i]); }
  int stamp() {
    if (!on) return RM_OK;
    HIP_OK(hipEventCreate(&t.ev[t.n]));
    t.n++;
    HIP_OK(hipEventRecord(t.ev[t.n - 1], stream));
    return RM_OK;
  }
  void keep(DeviceState &ds) {
    if (on) { ds.timed.push_back(t); kept = true; }
  }
};

int launch_render(const RmCamera *cam, const RmObject *objs, int numObjects, const RmLight *lights, int numLights,
                  const RmGlobals *g, const RmSettings *s, int W, int H, RowMap map, int nRows, float *d_rgba,
                  float *d_bright, hipStream_t stream, int count, RmCounters *countersOut,
                  const RmResources &res = kNoResources, double *clockMHz = nullptr, unsigned long long *d_waveSpans = nullptr) {
  // count: 0 production launch, 1 / 2 counted (reference work / executed work; synchronises), 3 production code with clock stamps
  int st = validate_scene(cam, objs, numObjects, lights, numLights, g, s, res);
  if (st != RM_OK) return st;
  if (W <= 0 || H <= 0 || nRows < 0) { set_error("bad frame size"); return RM_ERR_INVALID_ARGUMENT; }
  if (nRows == 0) return RM_OK;  // empty row range: nothing to write, a null buffer is fine
  if (!d_rgba) { set_error("null output buffer"); return RM_ERR_INVALID_ARGUMENT; }
  if ((st = check_device_pointers(res, d_rgba, d_bright)) != RM_OK) return st;
  DeviceState *pds;
  if ((st = current_device_state(&pds)) != RM_OK) return st;
  DeviceState &ds = *pds;
  std::lock_guard<std::mutex> lock(ds.mu);  // this device only; nothing below blocks on the GPU unless `count` asks for numbers back
  // the counter block (DeviceState::dCounters) that every render launch passes to its kernel, allocated once per device
  if (!ds.dCounters && hipMalloc(reinterpret_cast<void **>(&ds.dCounters), 10 * sizeof(unsigned long long)) != hipSuccess) {
    (void)hipGetLastError();
    ds.dCounters = nullptr;
    set_error("hipMalloc of the counter block failed");
    return RM_ERR_DEVICE;
  }
  StreamState &ss = ds.streams[stream];
  // Two schedules of the same per-ray arithmetic, identical bits: rm::render_kernel (one lane per pixel; every class, and the
  // counted variants) and, for table-walk classes with bounces, the wavefront pipeline.
  const int pathReq = kernel_path_request();
  const FrameClass fc = classify_frame(objs, numObjects, lights, numLights, g, s, count);
  Wavefront wf;
  if ((st = setup_wavefront(ds, ss, fc, objs, numObjects, numLights, W, nRows, map.numShards > 1, pathReq, stream, &wf)) != RM_OK) return st;
  // Waves (8×8 tiles, side by side) per workgroup.  A workgroup's registers and LDS come free only when its LAST wave
  // ends, and march lengths differ a lot between neighbouring tiles, so small workgroups keep more waves resident: one wave
  // per workgroup for every class (measured at the register budgets above: the 4K bulb frame 2.31 / 2.34 / 2.58 ms at
  // 1 / 2 / 4 waves, the 8K Menger frame 51.0 / 51.8 / 58.6 ms, bump + reflection at 4K 19.4 / 19.8 / 22.1 ms; at the
  // compiler's own budgets two waves were best for the bulb, profiles/r02_c_waves_per_block.md).  RM_WAVES_PER_BLOCK overrides.
  const int nw = waves_per_block();
  const unsigned long long key = picture_key(cam, objs, numObjects, lights, numLights, g, s, map);
  int shapeSlot;
  const int tileShift = tile_shift(ds, ss, fc, wf.on, count, W, nRows, key, &shapeSlot);
  const int tileW = 1 << tileShift, tileH = 64 >> tileShift;
  const dim3 rgrid((W + nw * tileW - 1) / (nw * tileW), (nRows + tileH - 1) / tileH), rblock(64 * nw);
  const int tileCount = (int)(rgrid.x * rgrid.y);
  TileOrderPlan to;
  if ((st = plan_tile_order(ds, ss, fc, wf.on, count, numObjects, W, nRows, nw, tileShift, tileCount, key, stream, &to)) != RM_OK) return st;
  const SplitPlan ls = plan_light_split(ds, ss, fc, to, count, nw, numLights, W, nRows, tileShift, tileCount, shapeSlot >= 0, key, stream);
  Slot *slot;
  if ((st = acquire_slot(ds.frames, 1, &slot)) != RM_OK) return st;
  fill_frames(slot->host, 1, cam, g, 1, objs, numObjects, lights, numLights, s, res);
  if (to.byGeom && !slot->host->objBallOk) to.byGeom = false;  // an object without a bounding ball (Sierpinski, 2-D Mandelbrot as an object): raster order
  LaunchFields lf;
  lf.tileOrder = to.ordered ? ((to.byCost || to.byGeom) ? to.order : nullptr) : ds.dbgTileOrder;
  lf.tileCost = to.ordered ? ((to.lastSort || to.settled) ? nullptr : to.cost) : ds.dbgTileCost;
  lf.tileCount = to.ordered ? tileCount : ds.dbgTileCount;
  lf.tileShift = tileShift;
  lf.splitTiles = ls.tiles; lf.splitStore = ls.store;
  if ((st = upload_frames(*slot, 1, lf, stream)) != RM_OK) return st;
  unsigned long long *dc = ds.dCounters;
  if (count) {
    HIP_OK(hipMemsetAsync(dc, 0, 10 * sizeof(unsigned long long), stream));
    if (d_waveSpans) HIP_OK(hipMemcpyAsync(dc + 5, &d_waveSpans, sizeof(d_waveSpans), hipMemcpyHostToDevice, stream));
  }
  LaunchTimer timer(stream);
  const RenderLaunch r{slot->dev, map, W, H, nRows, reinterpret_cast<float4 *>(d_rgba), reinterpret_cast<float4 *>(d_bright), dc, stream, rgrid, rblock};
  if (wf.on) {
    HIP_OK(hipMemsetAsync(wf.ws.counters, 0, WF_STRIDE * (kWfMaxBounces + 2) * sizeof(uint32_t), stream));
    if ((st = timer.stamp()) != RM_OK) return st;
    launch_wavefront(fc.wfSkip, r, wf, fc.wfBounces, numLights, ds.numCUs);
  } else {
    if ((st = timer.stamp()) != RM_OK) return st;
    if (to.sorts()) {
      if ((st = launch_tile_order(to, r, nw * tileW, tileH, tileCount)) != RM_OK) return st;
      if ((st = timer.stamp()) != RM_OK) return st;  // stage 0 = the ordering launches, stage 1 = the render
    }
    int splitSlot = ls.timedSlot;
    if ((st = ss.split.begin(splitSlot, stream)) != RM_OK || (st = ss.shape.begin(shapeSlot, stream)) != RM_OK) return st;
    if ((st = dispatch_render(fc, count, slot->host->bulbPlain != 0, ls, numLights, tileCount, r)) != RM_OK) return st;
    if ((st = ss.shape.end(shapeSlot, stream)) != RM_OK || (st = ss.split.end(splitSlot, stream)) != RM_OK) return st;
  }
  if ((st = timer.stamp()) != RM_OK) return st;
  HIP_OK(hipGetLastError());
  ds.lastPath = wf.on ? 5 : 1;
  ds.lastSplit = wf.on ? 0 : ls.tiles;
  timer.keep(ds);
  HIP_OK(hipEventRecord(slot->done, stream));
  if (count) {
    unsigned long long hc[10];
    HIP_OK(hipMemcpyAsync(hc, dc, sizeof(hc), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
    if (countersOut) {
      countersOut->sceneEvals = hc[0]; countersOut->bulbIters = hc[1]; countersOut->hitPixels = hc[2];
      countersOut->shadedPoints = hc[6]; countersOut->terrainEvals = hc[7]; countersOut->cloudEvals = hc[8];
      countersOut->shapeEvals = hc[9];
    }
    if (clockMHz) *clockMHz = hc[4] ? 100.0 * (double)hc[3] / (double)hc[4] : 0.0;
  }
  return RM_OK;
}

// ---- multi-frame calls: numFrames whole frames of one scene, each with its own camera and globals -----------------------------
// What rm_render_batch, rm_render_supersampled, rm_render_adaptive and rm_render_accumulated are all called with.  subFrames
// (rm_render_accumulated; 1 everywhere else): an output frame is made of that many cameras and globals, each staged as a scene
// block of its own — blocks() of them, block f·subFrames + j for sub-frame j of frame f — and globalsOf counts blocks.
struct FrameCall {
  const RmCamera *cams; const RmGlobals *globals; int numGlobals, numFrames;
  const RmObject *objs; int numObjects; const RmLight *lights; int numLights;
  const RmSettings *s; const RmResources &res;
  int W, H; float *d_rgba, *d_bright; hipStream_t stream;
  int subFrames = 1;
  int numObjectTables = 1, numLightTables = 1;  // rm_render_animated: 1 (table 0 for every block) or blocks()
  long long blocks() const { return (long long)numFrames * subFrames; }
  const RmGlobals *globalsOf(int b) const { return &globals[numGlobals == 1 ? 0 : b]; }
  const RmObject *objsOf(int b) const { return objs + (numObjectTables == 1 ? 0 : (size_t)b * (size_t)numObjects); }
  const RmLight *lightsOf(int b) const { return lights + (numLightTables == 1 ? 0 : (size_t)b * (size_t)numLights); }
};
// The launch of a one-lane-per-pixel kernel over `frames` frames of W × H pixels at ss samples per axis: waves_per_block() waves
// side by side in a workgroup, each on a tile of 2^tileShift × (64 >> tileShift) samples, the tiles of a frame in grid.x and
// grid.y and the frame in grid.z.
constexpr int kTiles8x8 = 3;  // the tile shift of the launches that take no shape pin
struct TileGrid { dim3 grid, block; };
TileGrid tile_grid(int W, int H, int frames, int ss = 1, int tileShift = kTiles8x8) {
  const long long nw = waves_per_block(), tileW = 1 << tileShift, tileH = 64 >> tileShift;
  return {dim3((unsigned)(((long long)ss * W + nw * tileW - 1) / (nw * tileW)), (unsigned)(((long long)ss * H + tileH - 1) / tileH),
               (unsigned)frames), dim3((unsigned)(64 * nw))};
}
// Its limits, for a frame whose ss·W and ss·H are at most INT_MAX / 8: the kernels' coordinates are 32-bit and come from blockIdx,
// a grid's y extent is at most 65535 tiles, and the tiles of one frame stay countable in an int (as render_kernel's).
bool tiles_fit(int W, int H, int ss) {
  const dim3 g = tile_grid(W, H, 1, ss).grid;
  return g.y <= 65535 && (long long)g.x * g.y <= INT_MAX;
}

// The head of every multi-frame call's argument checks, ahead of the first HIP call (as launch_render's); an input that fails
// several reports the first of this order.  numFrames = 0 passes: nothing to write, the caller returns RM_OK.  coordText (or
// null: launch_batch, whose kernel takes its tiles from the scene block's fields) and tilesText: the entry point's own texts where
// the call renders an ss·W × ss·H sample frame whose coordinates and tiles must fit the kernels' indices.
int check_frame_head(const FrameCall &c, int ss, const char *coordText, const char *tilesText) {
  if (c.numFrames < 0) { set_error("negative numFrames"); return RM_ERR_INVALID_ARGUMENT; }
  // one scene block per sub-frame: the cap counts blocks
  if (c.blocks() > RM_MAX_BATCH_FRAMES) {
    set_error(c.subFrames == 1 ? "numFrames exceeds RM_MAX_BATCH_FRAMES" : "numFrames·subFrames exceeds RM_MAX_BATCH_FRAMES");
    return RM_ERR_CAPACITY;
  }
  if (c.numFrames == 0) return RM_OK;
  if (c.numGlobals != 1 && c.numGlobals != c.blocks()) {
    set_error(c.subFrames == 1 ? "numGlobals must be 1 or numFrames" : "numGlobals must be 1 or numFrames·subFrames");
    return RM_ERR_INVALID_ARGUMENT;
  }
  if (!c.cams || !c.globals) { set_error("null cameras or globals"); return RM_ERR_INVALID_ARGUMENT; }
  if (c.W <= 0 || c.H <= 0) { set_error("bad frame size"); return RM_ERR_INVALID_ARGUMENT; }
  if (coordText) {
    if (c.W > INT_MAX / 8 / ss || c.H > INT_MAX / 8 / ss) { set_error(coordText); return RM_ERR_INVALID_ARGUMENT; }
    if (!tiles_fit(c.W, c.H, ss)) { set_error(tilesText); return RM_ERR_INVALID_ARGUMENT; }
  }
  return RM_OK;
}
// The argument checks of the entry points that render colour: the head, then sizeCheck, the entry point's own check of the frame
// size, then the scene and the outputs.  sampled: rm_render_supersampled and the calls that, like it, take their coordinates
// from blockIdx (rm_render_adaptive for ss = 1 too).
int check_frames(const FrameCall &c, int ss, bool sampled, int (*sizeCheck)(const FrameCall &) = nullptr) {
  int st = check_frame_head(c, ss, sampled ? "ss·W or ss·H exceeds INT_MAX / 8" : nullptr, "too many samples for one supersampled launch");
  if (st != RM_OK || c.numFrames == 0) return st;
  if (sizeCheck && (st = sizeCheck(c)) != RM_OK) return st;
  if ((st = validate_scene(&c.cams[0], c.objs, c.numObjects, c.lights, c.numLights, &c.globals[0], c.s, c.res)) != RM_OK) return st;
  if (!c.d_rgba) { set_error("null output buffer"); return RM_ERR_INVALID_ARGUMENT; }
  return check_device_pointers(c.res, c.d_rgba, c.d_bright);
}

// What the staging step hands a launcher, and what holds the device's lock for it: from lock_device (or stage_blocks) until the
// object goes, behind finish_frames.
struct StagedFrames {
  DeviceState *ds = nullptr;
  std::unique_lock<std::mutex> lock;  // ds->mu
  Slot *slot = nullptr;   // one scene block per frame (not per sample) and sub-frame, filled and uploaded
  FrameClass fc{};        // shared by every frame
  bool plainBulb = true;  // the plain bulb form only where every frame (and sub-frame) has it
  int bulbClass = 0;      // bulb_class of the two
  LaunchTimer timer;      // stamped once, ahead of the caller's launches
  explicit StagedFrames(hipStream_t stream) : timer(stream) {}
  // The current device's state and its lock, for a caller that needs them ahead of the staging (launch_adaptive's workspaces).
  int lock_device() {
    if (int st = current_device_state(&ds)) return st;
    lock = std::unique_lock<std::mutex>(ds->mu);
    return RM_OK;
  }
};
// The staging step of every launch but launch_render's own, between the argument checks and the first kernel: the device and its
// lock, a slot of n blocks of `ring` (nothing here waits for the GPU but acquire_slot at the ring's bounds), the caller's fill of
// the slot's pinned blocks, the upload with the launch fields (and the sponge prologue, upload_frames), the timing's start.
template <class Fill>
int stage_blocks(StagedFrames *sf, Ring DeviceState::*ring, int n, const LaunchFields &lf, bool mengerAnywhere, Fill fill) {
  int st = sf->ds ? RM_OK : sf->lock_device();
  if (st != RM_OK || (st = acquire_slot(sf->ds->*ring, n, &sf->slot)) != RM_OK) return st;
  fill(sf->slot->host);
  if ((st = upload_frames(*sf->slot, n, lf, sf->timer.stream, mengerAnywhere)) != RM_OK) return st;
  return sf->timer.stamp();
}
// A FrameCall's staging: stage_blocks on the batch ring with fill_frames, and the class of the call.  tileShift: the tile shape
// of the launch (LaunchFields).  alone (or null): the frames that are not part of the launch (launch_batch), which have no say
// in plainBulb.
int stage_frames(const FrameCall &c, int tileShift, const char *alone, StagedFrames *sf) {
  const int blocks = (int)c.blocks();  // = numFrames but for rm_render_accumulated (which passes no `alone`)
  for (int f = 0; f < blocks; f++)
    if (!alone || !alone[f]) sf->plainBulb = sf->plainBulb && bulb_plain(c.objs, c.numObjects, c.globalsOf(f));
  sf->fc = classify_frame(c.objs, c.numObjects, c.lights, c.numLights, c.globalsOf(0), c.s, 0);
  sf->bulbClass = bulb_class(sf->fc, sf->plainBulb);
  LaunchFields lf;
  lf.tileShift = tileShift;
  return stage_blocks(sf, &DeviceState::batches, blocks, lf, false, [&](SceneBlock *h) {
    fill_frames(h, blocks, c.cams, c.globals, c.numGlobals, c.objs, c.numObjects, c.lights, c.numLights, c.s, c.res);
  });
}
// One launch of the one-lane-per-pixel kernel of the class over frames f0 … f0 + k − 1 of the staged slot (grid.z = k), straight
// into the call's outputs: raster order, tiles 2^tileShift pixels wide (the shift the slot was staged with).
int launch_frames(const FrameCall &c, const StagedFrames &sf, int f0, int k, int tileShift) {
  const RowMap map{0, c.H, 0, 1, 0};
  const TileGrid t = tile_grid(c.W, c.H, k, 1, tileShift);
  const RenderLaunch r{sf.slot->dev + f0, map, c.W, c.H, c.H, reinterpret_cast<float4 *>(c.d_rgba), reinterpret_cast<float4 *>(c.d_bright),
                       nullptr, c.stream, t.grid, t.block};
  return dispatch_render(sf.fc, 0, sf.plainBulb, SplitPlan{}, c.numLights, 0, r);
}
// The finishing step, behind the caller's last launch: the timing's end, rm_debug_last_path / rm_debug_last_split and the slot's event.
int finish_frames(StagedFrames &sf, int path) {
  if (int st = sf.timer.stamp()) return st;
  HIP_OK(hipGetLastError());
  sf.ds->lastPath = path;
  sf.ds->lastSplit = 0;
  sf.timer.keep(*sf.ds);
  HIP_OK(hipEventRecord(sf.slot->done, sf.timer.stream));
  return RM_OK;
}

// ---- batches: rm_render_batch ------------------------------------------------------------------------------------------------
// Every batched frame renders with the one-lane-per-pixel kernel in raster tile order (no tile-order history, no light split), 8×8
// tiles unless a shape is pinned: a batch reads and changes none of the per-stream state (tuners, tile order), so a host that
// interleaves batches with repeated single frames sees those tune as before.  The frames overlap on the chip as frames in flight
// on several streams do — the tail of frame f under the full waves of frame f + 1 — without streams or per-call host overhead.
// A frame that would take the wavefront pipeline on its own (path 5, chosen or requested) is rendered through launch_render
// instead, after the batched launch, in frame order on the same stream.
int launch_batch(const FrameCall &c) {
  int st = check_frames(c, 1, false);
  if (st != RM_OK || c.numFrames == 0) return st;
  // which frames the single-frame launcher would give the wavefront pipeline (launch_render, setup_wavefront): only the 2-D mode,
  // a per-frame global, can tell frames apart
  const int pathReq = kernel_path_request();
  std::vector<char> alone(c.numFrames, 0);
  bool anyBatched = false;
  for (int f = 0; f < c.numFrames; f++) {
    const FrameClass fc = classify_frame(c.objs, c.numObjects, c.lights, c.numLights, c.globalsOf(f), c.s, 0);
    alone[f] = fc.wfOk && (pathReq == 5 || (pathReq == 0 && wavefront_pays(c.objs, c.numObjects, fc.wfBounces, (size_t)c.H * c.W, false)));
    anyBatched = anyBatched || !alone[f];
  }
  if (anyBatched) {
    const int pinned = tile_shape_request(), tileShift = (pinned == 2 || pinned == 3) ? pinned : kDefaultTileShift;
    StagedFrames sf(c.stream);  // and the device's lock, to the end of this block: launch_render below takes it itself
    if ((st = stage_frames(c, tileShift, alone.data(), &sf)) != RM_OK) return st;
    // one launch per run of consecutive batched frames (one run unless wavefront frames sit between them)
    for (int f0 = 0; f0 < c.numFrames;) {
      if (alone[f0]) { f0++; continue; }
      int f1 = f0;
      while (f1 < c.numFrames && !alone[f1]) f1++;
      if ((st = launch_frames(c, sf, f0, f1 - f0, tileShift)) != RM_OK) return st;
      f0 = f1;
    }
    if ((st = finish_frames(sf, 6)) != RM_OK) return st;
  }
  const size_t frame = (size_t)c.H * c.W * 4;  // floats per frame
  const RowMap whole{0, c.H, 0, 1, 0};
  for (int f = 0; f < c.numFrames; f++)
    if (alone[f] && (st = launch_render(&c.cams[f], c.objs, c.numObjects, c.lights, c.numLights, c.globalsOf(f), c.s, c.W, c.H, whole, c.H,
                                        c.d_rgba + f * frame, c.d_bright ? c.d_bright + f * frame : nullptr, c.stream, 0, nullptr, c.res)) != RM_OK)
      return st;
  return RM_OK;
}

// ---- supersampled frames: ss × ss samples per pixel, resolved in the wave (render_ss_kernel) -----------------------------------
// rm_render_supersampled.  stage_frames, then ONE launch over (tilesX, tilesY, numFrames) 8×8 sample tiles in raster order for
// every frame: no wavefront pipeline, no light split, no tile-shape pin, no tuner or tile-order state read or written, no library
// workspace.  The kernels are a translation unit of their own (rm_supersample.hip).
int launch_supersampled(const FrameCall &c, int ss) {
  if (ss != 1 && ss != 2 && ss != 4) { set_error("ss (samples per pixel along each axis) must be 1, 2 or 4"); return RM_ERR_INVALID_ARGUMENT; }
  if (ss == 1) return launch_batch(c);
  int st = check_frames(c, ss, true);
  if (st != RM_OK || c.numFrames == 0) return st;
  StagedFrames sf(c.stream);
  if ((st = stage_frames(c, kTiles8x8, nullptr, &sf)) != RM_OK) return st;
  const TileGrid t = tile_grid(c.W, c.H, c.numFrames, ss);
  if ((st = launch_render_ss(sf.slot->dev, sf.bulbClass, sf.fc.envFeatures, sf.fc.textured, sf.fc.secondary, t.grid, t.block, c.W, c.H, ss,
                             c.d_rgba, c.d_bright, c.stream)) != RM_OK) return st;
  return finish_frames(sf, 7);
}

// ---- adaptive supersampling: the 1-sample frame everywhere, ss × ss samples where it shows contrast ----------------------------
// rm_render_adaptive (the header has the definition).  stage_frames (one slot of the batch ring for the whole call), then per
// chunk of frames, all on the caller's stream: (1) launch_frames, the one-lane-per-pixel launch of launch_batch (8×8 tiles always)
// straight into the outputs — so an unflagged pixel is rm_render_batch's by construction —, (2) the classify kernel: mask,
// per-frame lists of flagged pixels and their counts into the stream's workspace, (3) for ss > 1 the refine kernel over the lists,
// which overwrites the flagged pixels.  The host never learns the counts: the refine grid is fixed — at most kRefineWaves waves per
// chunk, about three times what the chip holds, each striding over its frame's list — and workgroups past the end of a list leave
// at once.  No wavefront pipeline, no light split, no tile-shape pin, no tuner or tile-order state.
constexpr unsigned long long kAdaptiveDefaultCap = 256ull << 20;  // of list per chunk when no workspace limit is set (as the post passes')
constexpr int kRefineWaves = 16384;
int launch_adaptive(const FrameCall &c, int ss, float threshold, uint8_t *d_mask, uint32_t *d_refined) {
  if (ss != 1 && ss != 2 && ss != 4) { set_error("ss (samples per pixel along each axis) must be 1, 2 or 4"); return RM_ERR_INVALID_ARGUMENT; }
  if (threshold != threshold) { set_error("threshold is NaN"); return RM_ERR_INVALID_ARGUMENT; }
  int st = check_frames(c, ss, true, [](const FrameCall &call) {
    if ((long long)call.W * call.H > INT_MAX) { set_error("more pixels per frame than a list entry can index"); return (int)RM_ERR_INVALID_ARGUMENT; }
    return (int)RM_OK;
  });
  if (st != RM_OK || c.numFrames == 0) return st;
  if ((st = require_device_pointers({{"d_mask", d_mask}, {"d_refined", d_refined}})) != RM_OK) return st;
  StagedFrames sf(c.stream);
  if ((st = sf.lock_device()) != RM_OK) return st;  // ahead of the workspaces, which are in use until the last launch (rm_release_workspaces)
  // frames per chunk: 4 B of list per pixel under the workspace limit (a single frame above a set limit fails in stream_workspace)
  const size_t px = (size_t)c.W * (size_t)c.H;
  const unsigned long long limit = workspace_limit(), fit = (limit ? limit : kAdaptiveDefaultCap) / (4ull * px);
  const int chunk = fit < (unsigned long long)c.numFrames ? (fit < 1 ? 1 : (int)fit) : c.numFrames;
  void *listMem, *countMem;
  if ((st = stream_workspace(kWsAdaptive, c.stream, (size_t)chunk * px * sizeof(uint32_t), &listMem)) != RM_OK) return st;
  if ((st = stream_workspace(kWsAdaptiveCounts, c.stream, RM_MAX_BATCH_FRAMES * sizeof(uint32_t), &countMem)) != RM_OK) return st;
  uint32_t *list = static_cast<uint32_t *>(listMem), *counts = static_cast<uint32_t *>(countMem);
  if ((st = stage_frames(c, kTiles8x8, nullptr, &sf)) != RM_OK) return st;
  const int nw = waves_per_block();
  for (int f0 = 0; f0 < c.numFrames; f0 += chunk) {
    const int k = c.numFrames - f0 < chunk ? c.numFrames - f0 : chunk;
    if ((st = launch_frames(c, sf, f0, k, kTiles8x8)) != RM_OK) return st;
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemsetAsync(counts, 0, (size_t)k * sizeof(uint32_t), c.stream));
    const TileGrid t = tile_grid(c.W, c.H, k);
    if ((st = launch_adaptive_classify(c.d_rgba, c.W, c.H, f0, t.grid, t.block, threshold, d_mask, list, counts, c.stream)) != RM_OK) return st;
    if (d_refined) HIP_OK(hipMemcpyAsync(d_refined + f0, counts, (size_t)k * sizeof(uint32_t), hipMemcpyDeviceToDevice, c.stream));
    if (ss > 1) {
      // a frame's grid slice: enough waves for every pixel of it, at most the chunk's share of kRefineWaves
      const size_t perWave = 64 / (size_t)(ss * ss), want = (px + perWave * nw - 1) / (perWave * nw);
      const size_t most = (size_t)(kRefineWaves / nw / k > 0 ? kRefineWaves / nw / k : 1);
      const dim3 rgrid((unsigned)(want < most ? want : most), 1, (unsigned)k);
      if ((st = launch_adaptive_refine(sf.slot->dev + f0, sf.bulbClass, sf.fc.envFeatures, sf.fc.textured, sf.fc.secondary, rgrid, dim3(64 * nw),
                                       c.W, c.H, ss, list, counts, c.d_rgba, c.d_bright, c.stream)) != RM_OK) return st;
    }
  }
  return finish_frames(sf, 8);
}

// ---- accumulated frames: the mean of subFrames renders per output frame, summed in the lane (render_acc_kernel) -----------------
// rm_render_accumulated (the header has the definition).  stage_frames with one scene block per SUB-frame — numFrames·subFrames
// of them in one slot of the batch ring, which is all that grows with subFrames: "one block per sub-frame" also leaves room for
// per-sub-frame object tables later — then ONE launch over (tilesX, tilesY, numFrames) 8×8 tiles in raster order whose lanes walk
// their frame's blocks: no wavefront pipeline, no light split, no tile-shape pin, no tuner or tile-order state read or written, no
// library workspace.  The kernels are a translation unit of their own (rm_accumulate.hip).  subFrames = 1 takes the same launch:
// the sum of one frame is that frame and the scale is 1, so the bits are rm_render_batch's.
int launch_accumulated(const FrameCall &c) {
  if (c.subFrames < 1 || c.subFrames > RM_MAX_SUBFRAMES) { set_error("subFrames must be 1 … RM_MAX_SUBFRAMES"); return RM_ERR_INVALID_ARGUMENT; }
  int st = check_frames(c, 1, true);  // the frame's coordinates and tiles come from blockIdx, as a sample frame's do
  if (st != RM_OK || c.numFrames == 0) return st;
  StagedFrames sf(c.stream);
  if ((st = stage_frames(c, kTiles8x8, nullptr, &sf)) != RM_OK) return st;
  const TileGrid t = tile_grid(c.W, c.H, c.numFrames);
  if ((st = launch_render_acc(sf.slot->dev, sf.bulbClass, sf.fc.envFeatures, sf.fc.textured, sf.fc.secondary, t.grid, t.block, c.W, c.H,
                              c.subFrames, c.d_rgba, c.d_bright, c.stream)) != RM_OK) return st;
  return finish_frames(sf, 9);
}

// ---- animated frames: object and light tables per block (rm_render_animated) ---------------------------------------------------
// rm_render_animated (the header has the definition): rm_render_accumulated's call where numObjectTables / numLightTables say
// whether every block brings an object / light table of its own.  The table counts and validate_scene of EVERY block (the error
// text names the block) run as check_frames' size check, ahead of its pointer checks and of any HIP call.  Staging is
// stage_blocks with fill_frames_animated, one block per sub-frame, with the sponge prologue when any block holds a sponge.  The class of the call is the most general one any block needs: textured / secondary if any block is, the bulb classes
// only if every block is a lone Mandelbulb, the plain form only if every block has it.  subFrames = 1: the production
// render_kernel of that class over the blocks (launch_frames, 8×8 tiles); subFrames > 1: render_anim_kernel (rm_animate.hip), which
// stages the object table again where the restage bits say it changed.  One launch either way, path 10: no wavefront pipeline,
// light split, tile-shape pin, tile order or library workspace, no tuner or tile-order state read or written.
int check_animated_tables(const FrameCall &c) {
  const long long blocks = c.blocks();
  if (c.numObjectTables != 1 && c.numObjectTables != blocks) {
    set_error("numObjectTables must be 1 or numFrames·subFrames");
    return RM_ERR_INVALID_ARGUMENT;
  }
  if (c.numLightTables != 1 && c.numLightTables != blocks) {
    set_error("numLightTables must be 1 or numFrames·subFrames");
    return RM_ERR_INVALID_ARGUMENT;
  }
  // block 0 first: it also checks the counts that index the later tables (and the pointers they are taken from)
  for (int b = 0; b < (int)blocks; b++) {
    if (b > 0 && c.numObjectTables == 1 && c.numLightTables == 1) break;  // validate_scene reads nothing else per block
    const int st = validate_scene(&c.cams[b], c.objsOf(b), c.numObjects, c.lightsOf(b), c.numLights, c.globalsOf(b), c.s, c.res);
    if (st != RM_OK) {
      if (blocks > 1) set_error("block " + std::to_string(b) + ": " + rm_last_error());
      return st;
    }
  }
  return RM_OK;
}
int launch_animated(const FrameCall &c) {
  if (c.subFrames < 1 || c.subFrames > RM_MAX_SUBFRAMES) { set_error("subFrames must be 1 … RM_MAX_SUBFRAMES"); return RM_ERR_INVALID_ARGUMENT; }
  int st = check_frames(c, 1, true, check_animated_tables);
  if (st != RM_OK || c.numFrames == 0) return st;
  const int blocks = (int)c.blocks();
  // the class of the call and what the upload needs to know, from every block's own tables
  FrameClass fc = classify_frame(c.objsOf(0), c.numObjects, c.lightsOf(0), c.numLights, c.globalsOf(0), c.s, 0);
  bool plainBulb = true, menger = false;
  for (int b = 0; b < blocks; b++) {
    plainBulb = plainBulb && bulb_plain(c.objsOf(b), c.numObjects, c.globalsOf(b));
    if (b == 0 || (c.numObjectTables == 1 && c.numLightTables == 1)) continue;
    const FrameClass fb = classify_frame(c.objsOf(b), c.numObjects, c.lightsOf(b), c.numLights, c.globalsOf(b), c.s, 0);
    fc.bulb = fc.bulb && fb.bulb;
    fc.textured = fc.textured || fb.textured;
    fc.secondary = fc.secondary || fb.secondary;
    for (int i = 0; i < c.numObjects; i++) menger = menger || c.objsOf(b)[i].type == RM_MENGERSPONGE;
  }
  StagedFrames sf(c.stream);
  sf.fc = fc;
  sf.plainBulb = plainBulb;
  sf.bulbClass = bulb_class(fc, plainBulb);
  RestageBits restage;
  if ((st = stage_blocks(&sf, &DeviceState::batches, blocks, LaunchFields{}, menger, [&](SceneBlock *h) {
        fill_frames_animated(h, blocks, c.cams, c.globals, c.numGlobals, c.objs, c.numObjects, c.numObjectTables, c.lights, c.numLights,
                             c.numLightTables, c.s, c.res, &restage);
      })) != RM_OK) return st;
  if (c.subFrames == 1) {
    if ((st = launch_frames(c, sf, 0, c.numFrames, kTiles8x8)) != RM_OK) return st;
  } else {
    const TileGrid t = tile_grid(c.W, c.H, c.numFrames);
    if ((st = launch_render_anim(sf.slot->dev, restage, sf.bulbClass, fc.envFeatures, fc.textured, fc.secondary, t.grid, t.block, c.W, c.H,
                                 c.subFrames, c.d_rgba, c.d_bright, c.stream)) != RM_OK) return st;
  }
  return finish_frames(sf, 10);
}

// ---- G-buffers: what the primary ray hit (rm_render_gbuffer) -------------------------------------------------------------------
// rm_render_gbuffer (the header has the definition): rm_render_batch's call shape without lights and resources — a FrameCall
// that has none — and three outputs instead of colour.  Its checks run in check_frames' order, every one ahead of the first HIP
// call: check_frame_head (the coordinates and tiles come from blockIdx, as a sample frame's), then the scene — settings and
// table pointers, the layers and the 2-D mode the G-buffer does not describe, the table's limits and types — then the outputs.
// A texLoc, a sky box or an area light's rectangle without its sampler is no error: nothing here reads one.
// Staging is stage_blocks with fill_frames (one scene block per frame: cull data, ray planes, bulbPlain).  Then ONE launch of
// gbuffer_kernel (rm_gbuffer.hip) over (tilesX, tilesY, numFrames) 8×8 tiles in raster order, path 11: no wavefront pipeline,
// light split, tile-shape pin, tile order, tuner state or library workspace.
int check_gbuffer(const FrameCall &c, const float *d_normalDepth, const int32_t *d_objectId, const float *d_position) {
  int st = check_frame_head(c, 1, "W or H exceeds INT_MAX / 8", "too many tiles for one launch");
  if (st != RM_OK || c.numFrames == 0) return st;
  if (!c.s || (c.numObjects > 0 && !c.objs) || c.numObjects < 0) {
    set_error("null scene pointer or negative count");
    return RM_ERR_INVALID_ARGUMENT;
  }
  if ((st = refuse_layers(c.s, "rm_render_gbuffer describes the object table: TERRAIN / CLOUD / SEA may cover it")) != RM_OK) return st;
  for (int f = 0; f < c.numFrames; f++)
    if ((st = refuse_two_d(c.globalsOf(f), "the 2-D mode (isTwoD) marches no ray, it has no G-buffer")) != RM_OK) {
      set_error("frame " + std::to_string(f) + ": " + rm_last_error());
      return st;
    }
  if ((st = check_object_table(c.objs, c.numObjects, c.s)) != RM_OK) return st;
  if (!d_normalDepth || !d_objectId) { set_error("null output buffer"); return RM_ERR_INVALID_ARGUMENT; }
  return require_device_pointers({{"d_normalDepth", d_normalDepth}, {"d_objectId", d_objectId}, {"d_position", d_position}});
}
int launch_gbuffer(const FrameCall &c, float *d_normalDepth, int32_t *d_objectId, float *d_position) {
  int st = check_gbuffer(c, d_normalDepth, d_objectId, d_position);
  if (st != RM_OK || c.numFrames == 0) return st;
  const int n = c.numFrames;
  // the march class of the call: a lone Mandelbulb, its plain form only if every frame has it
  bool plainBulb = true;
  for (int f = 0; f < n; f++) plainBulb = plainBulb && bulb_plain(c.objs, c.numObjects, c.globalsOf(f));
  StagedFrames sf(c.stream);
  if ((st = stage_blocks(&sf, &DeviceState::batches, n, LaunchFields{}, false, [&](SceneBlock *h) {
        fill_frames(h, n, c.cams, c.globals, c.numGlobals, c.objs, c.numObjects, nullptr, 0, c.s, kNoResources);
      })) != RM_OK) return st;
  const TileGrid t = tile_grid(c.W, c.H, n);
  if ((st = launch_gbuffer_kernel(sf.slot->dev, table_bulb_class(c.objs, c.numObjects, plainBulb), t.grid, t.block, c.W, c.H, d_normalDepth,
                                  d_objectId, d_position, c.stream)) != RM_OK) return st;
  return finish_frames(sf, 11);
}
}  // namespace

// ---- one block, one launch: what the query entry points (rm_queries.hip) are staged with -----------------------------------------
// rm_launch.h has the call.  The device's lock first where the call takes a workspace, which is in use until the last launch
// (rm_release_workspaces); stage_blocks of one block filled by fill_frames; the launch; finish_frames.  An untimed call (the
// probes) takes no stamps and ends with the slot's event alone, whatever the launch returned.
int stage_block_launch(const BlockCall &c, const BlockLaunch &launch) {
  const RmCamera noCam{};
  StagedFrames sf(c.stream);
  sf.timer.on = sf.timer.on && c.timed;
  int st = RM_OK;
  void *mem = nullptr;
  if (c.workspaceBytes != 0 && ((st = sf.lock_device()) != RM_OK || (st = stream_workspace(kWsBlocks, c.stream, c.workspaceBytes, &mem)) != RM_OK))
    return st;
  if ((st = stage_blocks(&sf, c.singleFrameRing ? &DeviceState::frames : &DeviceState::batches, 1, LaunchFields{}, false, [&](SceneBlock *h) {
        fill_frames(h, 1, c.cam ? c.cam : &noCam, c.g, 1, c.objs, c.numObjects, c.lights, c.numLights, c.s, c.res ? *c.res : kNoResources);
        if (c.afterFill) c.afterFill(h);
      })) != RM_OK) return st;
  st = launch(sf.slot->dev, sf.slot->host, mem);
  if (!c.timed) {
    HIP_OK(hipEventRecord(sf.slot->done, c.stream));
    return st;
  }
  return st != RM_OK ? st : finish_frames(sf, c.path);
}
}  // namespace rm

using namespace rm;

extern "C" {

int rm_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return -1;
  return n;
}
int rm_set_device(int device) {
  HIP_OK(hipSetDevice(device));
  return RM_OK;
}

int rm_render(const RmCamera *cam, const RmObject *objs, int numObjects, const RmLight *lights, int numLights,
              const RmGlobals *g, const RmSettings *s, int W, int H, int rowBegin, int rowEnd, float *d_rgba,
              float *d_bright, void *stream) {
  return rm_render_res(cam, objs, numObjects, lights, numLights, g, s, nullptr, W, H, rowBegin, rowEnd, d_rgba, d_bright, stream);
}

int rm_render_ex(const RmCamera *cam, const RmObject *objs, int numObjects, const RmLight *lights, int numLights,
                 const RmGlobals *g, const RmSettings *s, const RmTexture *textures, int numTextures, int W, int H,
                 int rowBegin, int rowEnd, float *d_rgba, float *d_bright, void *stream) {
  RmResources res{};
  res.textures = textures; res.numTextures = numTextures;
  return rm_render_res(cam, objs, numObjects, lights, numLights, g, s, &res, W, H, rowBegin, rowEnd, d_rgba, d_bright, stream);
}

int rm_render_res(const RmCamera *cam, const RmObject *objs, int numObjects, const RmLight *lights, int numLights,
                  const RmGlobals *g, const RmSettings *s, const RmResources *res, int W, int H, int rowBegin, int rowEnd,
                  float *d_rgba, float *d_bright, void *stream) {
  RowMap map;
  int n;
  if (int st = row_range(H, rowBegin, rowEnd, &map, &n)) return st;
  return launch_render(cam, objs, numObjects, lights, numLights, g, s, W, H, map, n, d_rgba, d_bright,
                       static_cast<hipStream_t>(stream), 0, nullptr, res ? *res : kNoResources);
}

int rm_render_batch(const RmCamera *cams, const RmGlobals *globals, int numGlobals, int numFrames, const RmObject *objs, int numObjects,
                    const RmLight *lights, int numLights, const RmSettings *s, const RmResources *res, int W, int H, float *d_rgba,
                    float *d_bright, void *stream) {
  return launch_batch(FrameCall{cams, globals, numGlobals, numFrames, objs, numObjects, lights, numLights, s, res ? *res : kNoResources, W, H,
                                d_rgba, d_bright, static_cast<hipStream_t>(stream)});
}

int rm_render_supersampled(const RmCamera *cams, const RmGlobals *globals, int numGlobals, int numFrames, const RmObject *objs,
                           int numObjects, const RmLight *lights, int numLights, const RmSettings *s, const RmResources *res, int W,
                           int H, int ss, float *d_rgba, float *d_bright, void *stream) {
  return launch_supersampled(FrameCall{cams, globals, numGlobals, numFrames, objs, numObjects, lights, numLights, s,
                                       res ? *res : kNoResources, W, H, d_rgba, d_bright, static_cast<hipStream_t>(stream)}, ss);
}

int rm_render_adaptive(const RmCamera *cams, const RmGlobals *globals, int numGlobals, int numFrames, const RmObject *objs,
                       int numObjects, const RmLight *lights, int numLights, const RmSettings *s, const RmResources *res, int W, int H,
                       int ss, float threshold, float *d_rgba, float *d_bright, uint8_t *d_mask, uint32_t *d_refined, void *stream) {
  return launch_adaptive(FrameCall{cams, globals, numGlobals, numFrames, objs, numObjects, lights, numLights, s, res ? *res : kNoResources,
                                   W, H, d_rgba, d_bright, static_cast<hipStream_t>(stream)}, ss, threshold, d_mask, d_refined);
}

int rm_render_accumulated(const RmCamera *cams, const RmGlobals *globals, int numGlobals, int numFrames, int subFrames,
                          const RmObject *objs, int numObjects, const RmLight *lights, int numLights, const RmSettings *s,
                          const RmResources *res, int W, int H, float *d_rgba, float *d_bright, void *stream) {
  return launch_accumulated(FrameCall{cams, globals, numGlobals, numFrames, objs, numObjects, lights, numLights, s, res ? *res : kNoResources,
                                      W, H, d_rgba, d_bright, static_cast<hipStream_t>(stream), subFrames});
}

int rm_render_animated(const RmCamera *cams, const RmGlobals *globals, int numGlobals, const RmObject *objs, int numObjects,
                       int numObjectTables, const RmLight *lights, int numLights, int numLightTables, int numFrames, int subFrames,
                       const RmSettings *s, const RmResources *res, int W, int H, float *d_rgba, float *d_bright, void *stream) {
  FrameCall c{cams, globals, numGlobals, numFrames, objs, numObjects, lights, numLights, s, res ? *res : kNoResources,
              W, H, d_rgba, d_bright, static_cast<hipStream_t>(stream), subFrames};
  c.numObjectTables = numObjectTables; c.numLightTables = numLightTables;
  return launch_animated(c);
}

int rm_render_gbuffer(const RmCamera *cams, const RmGlobals *globals, int numGlobals, int numFrames, const RmObject *objs, int numObjects,
                      const RmSettings *s, int W, int H, float *d_normalDepth, int32_t *d_objectId, float *d_position, void *stream) {
  return launch_gbuffer(FrameCall{cams, globals, numGlobals, numFrames, objs, numObjects, nullptr, 0, s, kNoResources, W, H, nullptr, nullptr,
                                  static_cast<hipStream_t>(stream)}, d_normalDepth, d_objectId, d_position);
}

int rm_render_counted_ex(const RmCamera *cam, const RmObject *objs, int numObjects, const RmLight *lights, int numLights,
                         const RmGlobals *g, const RmSettings *s, int W, int H, int rowBegin, int rowEnd, float *d_rgba,
                         float *d_bright, int mode, RmCounters *out) {
  return rm_render_counted_res(cam, objs, numObjects, lights, numLights, g, s, nullptr, W, H, rowBegin, rowEnd, d_rgba, d_bright,
                               mode, out);
}
int rm_render_counted_res(const RmCamera *cam, const RmObject *objs, int numObjects, const RmLight *lights, int numLights,
                          const RmGlobals *g, const RmSettings *s, const RmResources *res, int W, int H, int rowBegin, int rowEnd,
                          float *d_rgba, float *d_bright, int mode, RmCounters *out) {
  RowMap map;
  int n;
  if (int st = row_range(H, rowBegin, rowEnd, &map, &n)) return st;
  if (mode != RM_COUNT_REFERENCE && mode != RM_COUNT_EXECUTED) { set_error("bad counting mode"); return RM_ERR_INVALID_ARGUMENT; }
  return launch_render(cam, objs, numObjects, lights, numLights, g, s, W, H, map, n, d_rgba, d_bright, nullptr, mode, out,
                       res ? *res : kNoResources);
}
int rm_render_counted(const RmCamera *cam, const RmObject *objs, int numObjects, const RmLight *lights, int numLights,
                      const RmGlobals *g, const RmSettings *s, int W, int H, int rowBegin, int rowEnd, float *d_rgba,
                      float *d_bright, RmCounters *out) {
  return rm_render_counted_ex(cam, objs, numObjects, lights, numLights, g, s, W, H, rowBegin, rowEnd, d_rgba, d_bright,
                              RM_COUNT_REFERENCE, out);
}
int rm_render_clocked(const RmCamera *cam, const RmObject *objs, int numObjects, const RmLight *lights, int numLights,
                      const RmGlobals *g, const RmSettings *s, int W, int H, float *d_rgba, double *shaderMHz,
                      unsigned long long *d_waveSpans) {
  if (!shaderMHz) { set_error("null shaderMHz"); return RM_ERR_INVALID_ARGUMENT; }
  if (d_waveSpans && !device_accessible(d_waveSpans)) { set_error("d_waveSpans is not device-accessible memory"); return RM_ERR_INVALID_ARGUMENT; }
  // the stamped build exists for the single-Mandelbulb class and for the plain table walk (no samplers, no procedural layers)
  bool plain = objs != nullptr && s != nullptr && numObjects >= 1 &&
               (s->features & (RM_FEAT_TERRAIN | RM_FEAT_CLOUD | RM_FEAT_SEA | RM_FEAT_SKY_BACKGROUND | RM_FEAT_NIGHTSKY_BACKGROUND)) == 0 && !s->enableSkyBox;
  for (int i = 0; plain && i < numObjects; i++) plain = objs[i].texLoc < 0 && !objs[i].isEmissive;
  for (int i = 0; plain && i < numLights; i++) plain = lights[i].type != RM_LIGHT_AREA;
  if (!plain) {
    set_error("rm_render_clocked covers the single-Mandelbulb class and the plain table walk (no samplers, no procedural layers)");
    return RM_ERR_UNSUPPORTED;
  }
  RowMap map{0, H > 0 ? H : 1, 0, 1, 0};
  return launch_render(cam, objs, numObjects, lights, numLights, g, s, W, H, map, H, d_rgba, nullptr, nullptr, 3, nullptr,
                       kNoResources, shaderMHz, d_waveSpans);
}

int rm_render_tiles(const RmCamera *cam, const RmObject *objs, int numObjects, const RmLight *lights, int numLights,
                    const RmGlobals *g, const RmSettings *s, int W, int H, int tileRows, int shard, int numShards,
                    float *d_rgba, float *d_bright, void *stream) {
  return rm_render_tiles_res(cam, objs, numObjects, lights, numLights, g, s, nullptr, W, H, tileRows, shard, numShards, d_rgba,
                             d_bright, stream);
}

int rm_render_tiles_res(const RmCamera *cam, const RmObject *objs, int numObjects, const RmLight *lights, int numLights,
                        const RmGlobals *g, const RmSettings *s, const RmResources *res, int W, int H, int tileRows,
                        int shard, int numShards, float *d_rgba, float *d_bright, void *stream) {
  if (tileRows <= 0 || numShards <= 0 || shard < 0 || shard >= numShards) {
    set_error("bad tile partition");
    return RM_ERR_INVALID_ARGUMENT;
  }
  RowMap map{0, tileRows, shard, numShards, root_relief()};
  return launch_render(cam, objs, numObjects, lights, numLights, g, s, W, H, map, shard_rows(H, tileRows, shard, numShards, root_relief()),
                       d_rgba, d_bright, static_cast<hipStream_t>(stream), 0, nullptr, res ? *res : kNoResources);
}

int rm_deinterleave(const float *d_gathered, float *d_frame, int W, int H, int tileRows, int numShards,
                    int shardStrideRows, void *stream) {
  if (!d_gathered || !d_frame || W <= 0 || H <= 0 || tileRows <= 0 || numShards <= 0 || numShards > 64 ||
      (shardStrideRows != 0 && shardStrideRows < max_shard_rows(H, tileRows, numShards, root_relief()))) {
    set_error("bad deinterleave arguments");
    return RM_ERR_INVALID_ARGUMENT;
  }
  if (int st = require_device_pointers({{"d_gathered", d_gathered}, {"d_frame", d_frame}})) return st;
  return launch_deinterleave(d_gathered, d_frame, W, H, tileRows, numShards, shardStrideRows, root_relief(), static_cast<hipStream_t>(stream));
}

int rm_tiles_to_rgba8(const float *d_tiles, uint8_t *d_tiles8, int W, int rows, void *stream) {
  if (W <= 0 || rows < 0) { set_error("bad tile arguments"); return RM_ERR_INVALID_ARGUMENT; }
  if (rows == 0) return RM_OK;
  if (!d_tiles || !d_tiles8) { set_error("null tile buffer"); return RM_ERR_INVALID_ARGUMENT; }
  if (int st = require_device_pointers({{"d_tiles", d_tiles}, {"d_tiles8", d_tiles8}})) return st;
  return launch_tiles_to_rgba8(d_tiles, d_tiles8, (size_t)rows * W, static_cast<hipStream_t>(stream));
}
int rm_deinterleave_rgba8(const uint8_t *d_gathered8, uint8_t *d_frame8, int W, int H, int tileRows, int numShards,
                          int shardStrideRows, int flip, void *stream) {
  if (!d_gathered8 || !d_frame8 || W <= 0 || H <= 0 || tileRows <= 0 || numShards <= 0 || numShards > 64 ||
      (shardStrideRows != 0 && shardStrideRows < max_shard_rows(H, tileRows, numShards, root_relief()))) {
    set_error("bad deinterleave arguments");
    return RM_ERR_INVALID_ARGUMENT;
  }
  if (int st = require_device_pointers({{"d_gathered8", d_gathered8}, {"d_frame8", d_frame8}})) return st;
  return launch_deinterleave_rgba8(d_gathered8, d_frame8, W, H, tileRows, numShards, shardStrideRows, flip, root_relief(),
                                   static_cast<hipStream_t>(stream));
}

int rm_frame_to_rgba8(const float *d_rgba, uint8_t *d_out, int W, int H, void *stream) {
  return rm_frames_to_rgba8(d_rgba, d_out, W, H, 1, stream);
}

int rm_frames_to_rgba8(const float *d_rgba, uint8_t *d_out, int W, int H, int numFrames, void *stream) {
  // every argument check ahead of the first HIP call (as rm_render_batch's)
  if (numFrames < 0) { set_error("negative numFrames"); return RM_ERR_INVALID_ARGUMENT; }
  if (numFrames > RM_MAX_BATCH_FRAMES) { set_error("numFrames exceeds RM_MAX_BATCH_FRAMES"); return RM_ERR_CAPACITY; }
  if (numFrames == 0) return RM_OK;
  if (!d_rgba || !d_out || W <= 0 || H <= 0) { set_error("bad frame arguments"); return RM_ERR_INVALID_ARGUMENT; }
  if (int st = require_device_pointers({{"d_rgba", d_rgba}, {"d_out", d_out}})) return st;
  return launch_to_rgba8(d_rgba, d_out, W, H, numFrames, static_cast<hipStream_t>(stream));
}

int rm_set_timing(int on) {
  g_timing.store(on != 0);
  DeviceState *ds;
  if (int st = current_device_state(&ds)) return st;
  std::lock_guard<std::mutex> lock(ds->mu);
  for (auto &t : ds->timed)
    for (int i = 0; i < t.n; i++) (void)hipEventDestroy(t.ev[i]);
  ds->timed.clear();
  return RM_OK;
}
int rm_get_timing(double *avgKernelMs, int *launches) {
  double stages[4];
  return rm_get_stage_timing(avgKernelMs, stages, launches);
}
int rm_get_stage_timing(double *avgTotalMs, double avgStageMs[4], int *launches) {
  DeviceState *ds;
  if (int st = current_device_state(&ds)) return st;
  std::vector<TimedLaunch> timed;
  {
    std::lock_guard<std::mutex> lock(ds->mu);
    timed.swap(ds->timed);  // waiting for the events happens outside the device lock
  }
  double total = 0.0, stage[4] = {0, 0, 0, 0};
  int rc = RM_OK;
  for (auto &t : timed) {
    if (t.n < 2 || rc != RM_OK) continue;
    float ms = 0.0f;
    if (hipEventSynchronize(t.ev[t.n - 1]) != hipSuccess || hipEventElapsedTime(&ms, t.ev[0], t.ev[t.n - 1]) != hipSuccess) {
      set_error("timing events could not be read");
      rc = RM_ERR_DEVICE;
      continue;
    }
    total += ms;
    // by role, whatever the launch was made of: the last interval is the render (one kernel or the wavefront pipeline's), the one
    // before it — present only in a launch that sorted its tiles — the ordering launches
    if (hipEventElapsedTime(&ms, t.ev[t.n - 2], t.ev[t.n - 1]) == hipSuccess) stage[1] += ms;
    if (t.n >= 3 && hipEventElapsedTime(&ms, t.ev[0], t.ev[t.n - 2]) == hipSuccess) stage[0] += ms;
  }
  const double n = timed.empty() ? 1.0 : (double)timed.size();
  if (launches) *launches = (int)timed.size();
  if (avgTotalMs) *avgTotalMs = total / n;
  if (avgStageMs) for (int i = 0; i < 4; i++) avgStageMs[i] = stage[i] / n;
  for (auto &t : timed)
    for (int i = 0; i < t.n; i++) (void)hipEventDestroy(t.ev[i]);
  return rc;
}
int rm_debug_check_math(unsigned long long *mismatches5) {
  if (!mismatches5) { set_error("null pointer"); return RM_ERR_INVALID_ARGUMENT; }
  unsigned long long *d = nullptr;
  HIP_OK(hipMalloc(reinterpret_cast<void **>(&d), 5 * sizeof(unsigned long long)));
  hipError_t e = hipMemset(d, 0, 5 * sizeof(unsigned long long));
  if (e == hipSuccess) {
    launch_check_math(d);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(mismatches5, d, 5 * sizeof(unsigned long long), hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (e != hipSuccess) { set_error(std::string("rm_debug_check_math: ") + hipGetErrorString(e)); return RM_ERR_DEVICE; }
  return RM_OK;
}
int rm_debug_set_tile_order(const int32_t *d_order, uint32_t *d_cost, int tileCount) {
  DeviceState *ds;
  if (int st = current_device_state(&ds)) return st;
  std::lock_guard<std::mutex> lock(ds->mu);
  ds->dbgTileOrder = d_order; ds->dbgTileCost = d_cost; ds->dbgTileCount = tileCount;
  return RM_OK;
}
int rm_set_tile_order(int mode) {
  if (mode < -1 || mode > 1) { set_error("tile order mode must be -1, 0 or 1"); return RM_ERR_INVALID_ARGUMENT; }
  g_tileOrderMode.store(mode);
  return RM_OK;
}
int rm_debug_last_path(void) {
  DeviceState *ds;
  if (current_device_state(&ds)) return -1;
  std::lock_guard<std::mutex> lock(ds->mu);
  return ds->lastPath;
}
int rm_debug_set_light_split(int div) {
  if (div < -1) { set_error("light split: -1 (default), 0 (off) or the divisor n >= 1"); return RM_ERR_INVALID_ARGUMENT; }
  g_lightSplit.store(div);
  g_lightSplitForce.store(div > 0);  // an explicit divisor splits without measuring (tests); -1 / the environment variable: measured
  return RM_OK;
}
int rm_debug_last_split(void) {
  DeviceState *ds;
  if (current_device_state(&ds) != RM_OK) return -1;
  std::lock_guard<std::mutex> lock(ds->mu);
  return ds->lastSplit;
}
int rm_set_kernel_path(int path) {
  if (path != 0 && path != 1 && path != 5) { set_error("kernel path must be 0, 1 or 5 (2-4, the bulb pipelines, were removed in round 4)"); return RM_ERR_INVALID_ARGUMENT; }
  g_kernelPath.store(path);
  return RM_OK;
}
int rm_debug_set_tile_shape(int mode) {
  if (mode != -1 && mode != 0 && mode != 2 && mode != 3) { set_error("tile shape mode must be -1, 0, 2 or 3"); return RM_ERR_INVALID_ARGUMENT; }
  g_tileShape.store(mode);
  return RM_OK;
}
int rm_set_workspace_limit(unsigned long long bytes) {
  g_wsLimit.store(bytes == ~0ull ? ~0ull - 1 : bytes);
  for (DeviceState &ds : g_dev) {  // what was refused under the old limit may be asked for again
    std::lock_guard<std::mutex> lock(ds.mu);
    for (auto &kv : ds.streams) kv.second.wfDenied = 0;
  }
  return RM_OK;
}
int rm_release_workspaces(unsigned long long *freedBytes) {
  DeviceState *ds;
  if (int st = current_device_state(&ds)) return st;
  std::lock_guard<std::mutex> lock(ds->mu);  // no launch is being enqueued on this device meanwhile
  size_t freed = 0;
  if (int st = release_workspaces(&freed)) return st;
  for (auto &kv : ds->streams) { kv.second.shape.drop(); kv.second.split.drop(); }
  for (Slot &b : ds->batches.slots) { freed += (size_t)b.cap * sizeof(SceneBlock); free_slot(b); }  // the device has drained
  ds->batches.slots.clear();
  ds->streams.clear();  // with the tile-order state: the feedback costs lived in the buffers just freed
  ds->shapeChoice.clear();
  ds->splitChoice.clear();
  if (freedBytes) *freedBytes = freed;
  return RM_OK;
}

}  // extern "C"
