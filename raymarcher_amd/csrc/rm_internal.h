// rm_internal.h — helpers shared by the launcher (rm_launcher.hip), the kernels' translation units and the host side (rm_host.cpp).
#pragma once
#include <initializer_list>
#include <mutex>
#include <string>
#include <utility>
#include <vector>
#include <cstdint>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#else
#define __host__
#define __device__
#endif

namespace rm {

// Records the text returned by rm_last_error() for the calling thread.
void set_error(const std::string &msg);

// True if `p` is memory a kernel may dereference (device, managed or pinned host) according to the HIP runtime.
// Every "device pointer" argument of the ABI is checked with it before a launch: a kernel that touches plain host
// memory faults the GPU.
bool device_accessible(const void *p);
// RM_ERR_INVALID_ARGUMENT (+ rm_last_error text) unless every non-null pointer of the list is device-accessible.
int require_device_pointers(std::initializer_list<std::pair<const char *, const void *>> ptrs);

#ifdef __HIPCC__
// Evaluates a HIP call; on failure records "<call>: <HIP's text>" and returns RM_ERR_DEVICE from the enclosing function.
#define HIP_OK(expr)                                                                              \
  do {                                                                                            \
    hipError_t e_ = (expr);                                                                       \
    if (e_ != hipSuccess) {                                                                       \
      set_error(std::string(#expr) + ": " + hipGetErrorString(e_));                               \
      return RM_ERR_DEVICE;                                                                       \
    }                                                                                             \
  } while (0)
// Takes the launcher's lock of the current device (rm_launcher.hip).  Whoever enqueues work on a buffer of stream_workspace
// holds it from that call to its last launch: rm_release_workspaces takes it too, so it never frees a buffer in use.
int lock_current_device(std::unique_lock<std::mutex> &lock);
// Grow-only device scratch memory owned by the library, one buffer per (current device, stream, user tag): calls on
// different streams of one device may run concurrently on the GPU and therefore never share scratch.  Growing
// synchronises `stream` (nothing else uses the old buffer) and reallocates.  Returns an rm_status.
enum { kWsPost = 2, kWsTileOrder = 3, kWsWavefront = 4, kWsLightSplit = 5, kWsAdaptive = 6, kWsAdaptiveCounts = 7, kWsMesh = 8, kWsBlocks = 9, kWsRayOrder = 10 };
int stream_workspace(int tag, hipStream_t stream, size_t need, void **out);
// The layout of a workspace, written once: take<T>(count) hands out the next `count` elements, every buffer on a multiple of 256
// bytes; bytes() is what has been taken.  Without a base it only measures (take returns null), so the size a caller asks
// stream_workspace for and the pointers its kernels get come from the same lines.
class Carve {
 public:
  explicit Carve(void *base = nullptr) : base_(static_cast<char *>(base)) {}
  template <class T>
  T *take(size_t count) {
    const size_t at = used_;
    used_ += (count * sizeof(T) + 255) & ~size_t(255);
    return base_ ? reinterpret_cast<T *>(base_ + at) : nullptr;
  }
  size_t bytes() const { return used_; }

 private:
  char *base_;
  size_t used_ = 0;
};
// The test-only probe of the scene evaluator (rm_probe.hip, rm_probe_sdscene_variant): whether a production kernel instantiates
// this combination (no HIP call), and the launch of its probe kernel on a staged SceneBlock (device pointer `sb`).
bool sdscene_variant_exists(int bulbClass, int count, int trap, int skip, int track, bool one);
int launch_sdscene_variant(const void *sb, int bulbClass, int count, int trap, int skip, int track, int one, const float *d_pts,
                           const float *d_ub, float *d_out, int n, hipStream_t stream);
// The other test-only probes of rm_probe.hip: rm_probe_math's kernel, the plain sdScene probe on a staged SceneBlock and the
// 2^32-input checker of the cheap exact forms (rm_debug_check_math; `d_out5` zeroed by the caller, default stream).
int launch_probe_math(int fn, const float *d_x, const float *d_y, const float *d_z, float *d_out, int n, hipStream_t stream);
int launch_probe_sdscene(const void *sb, const float *d_pts, float *d_out, int n, hipStream_t stream);
int launch_probe_bump(const float *d_pts, float *d_out, int n, hipStream_t stream);  // rm_probe_bump's kernel: bumpGradient
// rm_probe_pool_cull's kernel: the shadow pool's prepared cull beside bulbCullEnd (rm_probe.hip)
int launch_probe_pool_cull(const void *sb, int bulbClass, int light, float far, const float *d_pts, float *d_out, int n, hipStream_t stream);
void launch_check_math(unsigned long long *d_out5);
// The kernels of rm_kernels.hip, as the launcher calls them (the structs are rm_launch.h's, FrameClass rm_frame.h's).  Scene prep:
// the sponge uniforms of the n staged blocks.  Tile order: the ordering launches of a plan, ahead of the render.  Wavefront: the
// pipeline's generations (skip: its kernels take the table walk's pass-over test).  dispatch_render: the one-lane-per-pixel kernel
// of the frame's class — counted, light-split or production — over r's grid.  Then the conversion kernels of the entry points
// named after them, arguments already checked.
struct SceneBlock; struct RenderLaunch; struct TileOrderPlan; struct SplitPlan; struct Wavefront; struct FrameClass;
int launch_scene_prep(SceneBlock *sb, int n, hipStream_t stream);
int launch_tile_order(const TileOrderPlan &p, const RenderLaunch &r, int tileWpx, int tileH, int tileCount);
void launch_wavefront(bool skip, const RenderLaunch &r, const Wavefront &wf, int bounces, int numLights, int numCUs);
int dispatch_render(const FrameClass &fc, int count, bool plainBulb, const SplitPlan &ls, int numLights, int tileCount,
                    const RenderLaunch &r);
int launch_to_rgba8(const float *d_rgba, uint8_t *d_out, int W, int H, int numFrames, hipStream_t stream);
int launch_tiles_to_rgba8(const float *d_tiles, uint8_t *d_tiles8, size_t n, hipStream_t stream);
int launch_deinterleave(const float *d_gathered, float *d_frame, int W, int H, int tileRows, int numShards, int shardStrideRows,
                        int relief, hipStream_t stream);
int launch_deinterleave_rgba8(const uint8_t *d_gathered8, uint8_t *d_frame8, int W, int H, int tileRows, int numShards,
                              int shardStrideRows, int flip, int relief, hipStream_t stream);
// The supersampling kernels (rm_supersample.hip, rm_render_supersampled): the launch of render_ss_kernel<bulbClass, env, tex, sec>
// over the staged SceneBlocks `sb` (device pointer; one per frame of grid.z), W × H output pixels of ss × ss samples each.  A
// translation unit of its own, so that the code objects of rm_kernels.hip do not depend on it.
int launch_render_ss(const void *sb, int bulbClass, bool env, bool tex, bool sec, dim3 grid, dim3 block, int W, int H, int ss,
                     float *d_rgba, float *d_bright, hipStream_t stream);
// The accumulating kernels (rm_accumulate.hip, rm_render_accumulated; a translation unit of its own for the same reason): the
// launch of render_acc_kernel<bulbClass, env, tex, sec> over the staged SceneBlocks `sb` — n per frame of grid.z, frame f's at
// sb[f·n] … sb[f·n + n − 1] — into W × H output pixels per frame: their sum in index order, times 1.0f / n.
int launch_render_acc(const void *sb, int bulbClass, bool env, bool tex, bool sec, dim3 grid, dim3 block, int W, int H, int n,
                      float *d_rgba, float *d_bright, hipStream_t stream);
// The animated kernels (rm_animate.hip, rm_render_animated with subFrames > 1; a translation unit of its own for the same reason):
// launch_render_acc's launch where every block has its own object and light table; `restage` says before which blocks a workgroup
// stages the object table anew (RestageBits, rm_scene_block.h).
struct RestageBits;
int launch_render_anim(const void *sb, const RestageBits &restage, int bulbClass, bool env, bool tex, bool sec, dim3 grid, dim3 block,
                       int W, int H, int n, float *d_rgba, float *d_bright, hipStream_t stream);
// The G-buffer kernels (rm_gbuffer.hip, rm_render_gbuffer; a translation unit of its own for the same reason): the launch of
// gbuffer_kernel<bulbClass> over the staged SceneBlocks `sb` (one per frame of grid.z) — normal and depth, object index and, when
// d_position is not null, the surface point of every pixel's primary hit, W·H elements per frame.
int launch_gbuffer_kernel(const void *sb, int bulbClass, dim3 grid, dim3 block, int W, int H, float *d_normalDepth, int32_t *d_objectId,
                          float *d_position, hipStream_t stream);
// The trace kernels (rm_trace.hip, rm_trace_rays; a translation unit of its own for the same reason): the launch of
// trace_kernel<bulbClass, closest / occlusion> over the ONE staged SceneBlock `sb`, one lane per ray — numRays RmRay from d_rays,
// numRays RmRayHit into d_hits.  noNormal (closest only): the surface point and the normal are left out, zeros stored.
int launch_trace_kernel(const void *sb, int bulbClass, bool occlusion, bool noNormal, const void *d_rays, int numRays, void *d_hits,
                        hipStream_t stream);
// The shade kernels (rm_shade.hip, rm_shade_rays; a translation unit of its own for the same reason): the launch of
// shade_rays_kernel<bulbClass, env, tex, sec> over the ONE staged SceneBlock `sb`, one lane per ray — numRays RmRay from d_rays,
// numRays float4 of colour into d_rgba and, when d_bright is not null, of bright values into d_bright.
int launch_shade_kernel(const void *sb, int bulbClass, bool env, bool tex, bool sec, const void *d_rays, int numRays, float *d_rgba,
                        float *d_bright, hipStream_t stream);
// The light-probe kernels (rm_light_probes.hip, rm_light_probes; a translation unit of its own for the same reason): the launch of
// light_probes_kernel<bulbClass, env, tex, sec, numDirs above 64> over the ONE staged SceneBlock `sb`, (probe, row) pairs flattened
// over lanes — numProbes float4 from d_positions, numSets·numDirs RmProbeDir from d_dirs, numProbes RmLightProbe into d_out.
int launch_probes_kernel(const void *sb, int bulbClass, bool env, bool tex, bool sec, const float *d_positions, int numProbes,
                         const void *d_dirs, int numDirs, int numSets, void *d_out, hipStream_t stream);
// The probe-depth kernels (rm_light_depth.hip, rm_light_probes_depth; a translation unit of its own for the same reason): the launch
// of light_depth_kernel<bulbClass, numDirs from 64 on> over the ONE staged SceneBlock `sb`, light_probes_kernel's flattening for the
// march and a lane per texel behind it — numProbes float4 from d_positions, numSets·numDirs RmProbeDir from d_dirs and as many rows
// of 64 floats from d_weights, numProbes RmProbeDepth into d_out.
int launch_probes_depth_kernel(const void *sb, int bulbClass, const float *d_positions, int numProbes, const void *d_dirs,
                               const float *d_weights, int numDirs, int numSets, float maxDistance, void *d_out, hipStream_t stream);
// The kernels that read a light grid at the primary hit (rm_shade_indirect.hip, rm_shade_rays_indirect; rm_light_probes_indirect.hip,
// rm_light_probes_indirect; translation units of their own for the same reason): launch_shade_kernel's and launch_probes_kernel's
// launches with the grid of the call — an RmLightGridRef's fields, checked, with k = strength · RM_INV_PI — by value in the kernel's
// arguments.  There is no bright output.
struct IndirectGridArgs { const void *d_probes, *d_depth; int dims[3]; float origin[3], step[3]; float k; unsigned flags; float normalBias; };
int launch_shade_indirect_kernel(const void *sb, int bulbClass, bool env, bool tex, bool sec, const void *d_rays, int numRays,
                                 const IndirectGridArgs &grid, float *d_rgba, hipStream_t stream);
int launch_probes_indirect_kernel(const void *sb, int bulbClass, bool env, bool tex, bool sec, const float *d_positions, int numProbes,
                                  const void *d_dirs, int numDirs, int numSets, const IndirectGridArgs &grid, void *d_out,
                                  hipStream_t stream);
// The layer kernels (rm_layers.hip, rm_shade_rays_layers and rm_trace_rays_layers; a translation unit of its own for the same
// reason), for the calls that have a layer bit — a call without one goes to the two launches above.  shade_rays_layers_kernel<tex,
// sec> (the env class; imageWidth feeds the sea normal's epsilon) and trace_layers_kernel<bulbClass> (closest mode only) over the
// ONE staged SceneBlock `sb`, one lane per ray.
int launch_shade_layers_kernel(const void *sb, bool tex, bool sec, const void *d_rays, int numRays, int imageWidth, float *d_rgba,
                               float *d_bright, hipStream_t stream);
int launch_trace_layers_kernel(const void *sb, int bulbClass, bool noNormal, const void *d_rays, int numRays, int imageWidth,
                               void *d_hits, hipStream_t stream);
// The lattice family — rm_sdf_grid, rm_sdf_mesh, the block-sparse forms, the lattice queries — declares itself in rm_lattice.h.
// The points kernels (rm_points.hip, rm_shade_points; a translation unit of its own for the same reason): the launch of
// shade_points_kernel<bulbClass, tex> over the ONE staged SceneBlock `sb`, one lane per point — numPoints float4 from d_points and,
// when d_view is not null, from d_view; into whichever of d_surface (numPoints RmSurfacePoint), d_ao (a float each) and d_rgba (a
// float4 each) are not null.
int launch_points_kernel(const void *sb, int bulbClass, bool tex, const float *d_points, const float *d_view, int numPoints,
                         int projectSteps, float iso, float maxMove, void *d_surface, float *d_ao, float *d_rgba,
                         hipStream_t stream);
// The kernels of rm_render_adaptive (rm_adaptive.hip, a translation unit of its own for the same reason).  Classify: the contrast
// test over frames f0 … f0 + grid.z − 1 of d_rgba (grid: their 8×8 tiles), into d_mask (may be null; whole-batch pointer) and the chunk's lists and
// counters (frame z of the chunk: W·H words from d_list + z·W·H, count in d_counts[z], zeroed by the caller).  Refine: the
// supersampling kernel of the class over those lists, grid.z = the chunk's frames, `sb` the chunk's first scene block.
int launch_adaptive_classify(const float *d_rgba, int W, int H, int f0, dim3 grid, dim3 block, float threshold, uint8_t *d_mask,
                             uint32_t *d_list, uint32_t *d_counts, hipStream_t stream);
int launch_adaptive_refine(const void *sb, int bulbClass, bool env, bool tex, bool sec, dim3 grid, dim3 block, int W, int H, int ss,
                           const uint32_t *d_list, const uint32_t *d_counts, float *d_rgba, float *d_bright, hipStream_t stream);
#endif
// ---- register budgets of the render kernels (rm_kernels.hip has the measurements; -DRM_*_WAVES=n overrides) --------------------
#ifndef RM_GENERIC_WAVES
#define RM_GENERIC_WAVES 6
#endif
#ifndef RM_BULB_WAVES
#define RM_BULB_WAVES 5
#endif
// the instantiations without main's secondary rays (SEC = false: no reflection / refraction anywhere in the frame) need far fewer
// registers — the bulb kernel 90 without a single spill — and take their own budgets (profiles/r04_d_secondary_rays.md)
#ifndef RM_BULB_NOSEC_WAVES
#define RM_BULB_NOSEC_WAVES 6
#endif
#ifndef RM_GENERIC_NOSEC_WAVES
#define RM_GENERIC_NOSEC_WAVES 6
#endif
#ifndef RM_ENV_NOSEC_WAVES
#define RM_ENV_NOSEC_WAVES 6
#endif
#ifndef RM_TEX_NOSEC_WAVES
#define RM_TEX_NOSEC_WAVES 6
#endif
#ifndef RM_ENV_WAVES
#define RM_ENV_WAVES 6
#endif
#ifndef RM_TEX_WAVES
#define RM_TEX_WAVES 6
#endif
// the register budget of a kernel class: the second launch bound of render_kernel
constexpr int render_waves(int bulb, bool env, bool tex, bool sec) {
  if (tex) return sec ? RM_TEX_WAVES : RM_TEX_NOSEC_WAVES;
  if (env) return sec ? RM_ENV_WAVES : RM_ENV_NOSEC_WAVES;
  if (bulb) return sec ? RM_BULB_WAVES : RM_BULB_NOSEC_WAVES;
  return sec ? RM_GENERIC_WAVES : RM_GENERIC_NOSEC_WAVES;
}
// The single-Mandelbulb class (the kernels' BULB template parameter; 0 = the table walk): any object transform, power and
// Julia seed, or the plain form that SceneBlock::bulbPlain describes.
constexpr int kBulbGeneral = 1, kBulbPlain = 2;
// The production kernel classes: the twelve <BULB, ENV, TEX, SEC> that render_kernel, render_ss_kernel, adaptive_refine_kernel,
// render_acc_kernel, render_anim_kernel, shade_rays_kernel and light_probes_kernel are instantiated with.  Layers and samplers (env, tex: the table walk,
// whatever the table holds) first, then the bulb class, then the plain table walk, each with main's secondary rays compiled in
// only where they can fire (sec).
template <int BULB, bool ENV, bool TEX, bool SEC>
struct KernelClass { static constexpr int bulb = BULB; static constexpr bool env = ENV, tex = TEX, sec = SEC; };
// Calls f(KernelClass<…>{}) for the class of a launch: `f` is a generic lambda that launches its kernel with the tag's members as
// template arguments, so a kernel has exactly the instantiations of this ladder.
template <class F>
void dispatch_class(int bulbClass, bool env, bool tex, bool sec, F &&f) {
  auto either = [&](auto on, auto off) { if (sec) f(on); else f(off); };
  if (env && tex) either(KernelClass<0, true, true, true>{}, KernelClass<0, true, true, false>{});
  else if (env) either(KernelClass<0, true, false, true>{}, KernelClass<0, true, false, false>{});
  else if (tex) either(KernelClass<0, false, true, true>{}, KernelClass<0, false, true, false>{});
  else if (bulbClass == kBulbPlain) either(KernelClass<kBulbPlain, false, false, true>{}, KernelClass<kBulbPlain, false, false, false>{});
  else if (bulbClass == kBulbGeneral) either(KernelClass<kBulbGeneral, false, false, true>{}, KernelClass<kBulbGeneral, false, false, false>{});
  else either(KernelClass<0, false, false, true>{}, KernelClass<0, false, false, false>{});
}
// The three march classes — the plain bulb, the general bulb, the table walk — of the kernels that march or evaluate the scene
// without shading it (rays, G-buffer, lattices): f(MarchClass<…>{}), as dispatch_class calls its f.
template <int BULB>
struct MarchClass { static constexpr int bulb = BULB; };
template <class F>
void dispatch_march_class(int bulbClass, F &&f) {
  if (bulbClass == kBulbPlain) f(MarchClass<kBulbPlain>{});
  else if (bulbClass == kBulbGeneral) f(MarchClass<kBulbGeneral>{});
  else f(MarchClass<0>{});
}

// The largest single workspace buffer stream_workspace may allocate, 0 = no limit (rm_set_workspace_limit).
unsigned long long workspace_limit();

// Baseline JPEG → RGBA8, top row first (rm_jpeg.cpp).
int jpeg_decode(const std::vector<uint8_t> &file, std::vector<uint8_t> &rgba, int &W, int &H);
// First frame of a GIF → RGBA8, top row first (rm_gif.cpp).
int gif_decode(const std::vector<uint8_t> &file, std::vector<uint8_t> &rgba, int &W, int &H);

// ---- the row-tile partition of a frame over the shards of a multi-GPU render ------------------------------------------------
// A frame of H rows is cut into tiles of tileRows rows.  relief = 0 (the classic deal): tile t belongs to shard t mod N.
// relief = K >= 2 ("root relief"): the deal runs in cycles of N·K − 1 tiles — K − 1 full rounds over shards 0 … N−1, then one
// round that leaves shard 0 out — so shard 0 (the gather's root, which also receives N − 1 slots and de-interleaves the whole
// frame every frame) owns (K − 1)/K of a peer's tiles.  A shard's tiles are packed in frame order either way.
// The process-wide setting (rm_set_root_relief; every rank of a job must use the same) is read by every entry point that deals
// tiles; the functions below take it as a parameter so that kernels receive it by value.
int root_relief();

// global tile → (shard, the shard's local tile ordinal)
__host__ __device__ inline void tile_owner(int t, int N, int K, int &shard, int &local) {
  if (K < 2 || N < 2) { shard = t % N; local = t / N; return; }
  const int L = N * K - 1, q = t / L, c = t % L;
  if (c < N * (K - 1)) { shard = c % N; local = q * (shard == 0 ? K - 1 : K) + c / N; }
  else { shard = c - N * (K - 1) + 1; local = q * K + (K - 1); }
}
// ---- the launcher's timed A/B tuners (tile shape, light split: rm_launcher.hip, Tuner) --------------------------------------
// A tuner runs candidate 0 for two frames, then candidate 1 for two frames, `rounds` times over, and times the second frame of
// each pair in timing slot 2·round + candidate.  After the schedule, and until every timing is in, it runs candidate 0: the
// enqueue path never waits for the timings.
struct TuneStep {
  int candidate;
  int slot;  // the timing slot this frame records, -1 for an untimed frame
};
inline TuneStep tune_schedule(int frame, int rounds) {
  if (frame >= 4 * rounds) return {0, -1};
  const int candidate = (frame >> 1) & 1;
  return {candidate, (frame & 1) ? 2 * (frame >> 2) + candidate : -1};
}
// The decision from the times ms[slot] of slots 0 … 2·rounds − 1: candidate 1 only if every time could be read and its best
// time is below 0.97 × candidate 0's best time (it must win by 3 %).
inline int tune_decide(const float *ms, int rounds, bool allRead) {
  float best[2] = {1e30f, 1e30f};
  for (int k = 0; k < 2 * rounds; k++) best[k & 1] = ms[k] < best[k & 1] ? ms[k] : best[k & 1];
  return (allRead && best[1] < 0.97f * best[0]) ? 1 : 0;
}

// a shard's local tile ordinal → global tile (increasing in j)
__host__ __device__ inline int tile_of(int shard, int j, int N, int K) {
  if (K < 2 || N < 2) return j * N + shard;
  const int L = N * K - 1, m = (shard == 0) ? K - 1 : K, q = j / m, i = j % m;
  return q * L + ((i < K - 1) ? i * N + shard : N * (K - 1) + shard - 1);
}
// Rows owned by `shard`.
__host__ __device__ inline int shard_rows(int H, int tileRows, int shard, int numShards, int relief = 0) {
  const int tiles = (H + tileRows - 1) / tileRows;
  int owned;
  if (relief < 2 || numShards < 2) {
    if (shard >= tiles) return 0;
    owned = (tiles - shard + numShards - 1) / numShards;
  } else {
    const int N = numShards, K = relief, L = N * K - 1, m = (shard == 0) ? K - 1 : K, rem = tiles % L;
    const int full = rem < N * (K - 1) ? rem : N * (K - 1);  // positions of the remainder that lie in the full rounds
    owned = (tiles / L) * m + (full > shard ? (full - shard + N - 1) / N : 0) + ((shard >= 1 && rem > N * (K - 1) + shard - 1) ? 1 : 0);
  }
  if (owned <= 0) return 0;
  int rows = owned * tileRows;
  const int lastRows = H - (tiles - 1) * tileRows;  // rows of the (possibly partial) last tile
  int s, l;
  tile_owner(tiles - 1, numShards, relief, s, l);
  if (s == shard) rows -= tileRows - lastRows;
  return rows;
}
// rows of the largest shard (the size of one gather slot): shard 0 without relief, shard 1 with it
__host__ __device__ inline int max_shard_rows(int H, int tileRows, int numShards, int relief = 0) {
  const int a = shard_rows(H, tileRows, 0, numShards, relief);
  const int b = numShards > 1 ? shard_rows(H, tileRows, 1, numShards, relief) : 0;
  return a > b ? a : b;
}

}  // namespace rm
