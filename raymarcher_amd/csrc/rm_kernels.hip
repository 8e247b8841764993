// rm_kernels.hip — the HIP kernels of the per-pixel raymarch and the functions that launch them (gfx950 only).
//
// Replaces Realtime::rayMarch() of the reference (src/realtimerender.cpp:53-87): instead of uploading
// ~600 uniforms by name and drawing a full-screen quad through resources/raymarch.{vert,frag}, the
// launcher (rm_launcher.hip) copies one constant SceneBlock to the device and launches one lane per pixel.
// Here: render_kernel and its class ladder, the scene-prep kernel, the tile-order kernels, the conversion kernels and the
// wavefront pipeline (rm_wavefront.hip.h).  The launch functions are declared in rm_internal.h; no state lives here.
#include <hip/hip_runtime.h>

#include "rm_device.hip.h"
#include "rm_wavefront.hip.h"
#include "rm_internal.h"
#include "rm_frame.h"
#include "rm_launch.h"

namespace rm {

// COUNT: 0 production, 1 reference-work counters, 2 executed-work counters (rm_device.hip.h), 3 production code plus clock
// stamps: every wave adds its (s_memtime, s_memrealtime) spans to counters[3], counters[4] — shader cycles and 100 MHz
// ticks — from which rm_render_clocked derives the clock the chip held under this kernel's own load.  The stamps go to a
// buffer of their own and no output value depends on them.
// Register budget = waves per SIMD (second launch bound), MEASURED per kernel class (profiles/r02_m_occupancy.md): the
// compiler's own choice for these kernels is 121-219 VGPRs (2-4 waves); bounding them tighter spills 29-90 registers, but
// the spills land outside the march / iteration loops (shading prologues and epilogues) and the extra resident waves hide the
// serial latency of an evaluation (scalar loads per object, dependent transcendental chains): at 3840x2160 a 5-object Phong
// scene gains 26 %, bump + reflection 28 %, textured / sky-box scenes 83-90 %, the 8K Menger frame 18 %, the terrain and
// sea frames 5-7 %, the headline bulb frame 2.3 % (5 waves; its hot loops stay spill-free).  Re-tuned on the final code: 6 / 5 / 6 / 6.  Frames too small to fill the
// chip (256x256, 1080p tails) lose 1-2 %.  -DRM_*_WAVES=n overrides, for the experiment script scripts/gpu_variants.sh.
// The budgets themselves (RM_*_WAVES, render_waves) are in rm_internal.h: the supersampling kernels of rm_supersample.hip take the same.
// SPLIT ("light split", launch_render): 1 = the launch of a frame whose heaviest tiles are rendered one light per workgroup — a 1-D
// grid: workgroups 0 … splitTiles·numLights − 1 are those tiles' partial workgroups (tile = tileOrder[b / numLights], light b mod
// numLights: primary march, surface, THAT light's shadow march, its result to splitStore), the last of which to arrive finishes
// the tile's pixels from the stored results (shadePixel's mode 2: no march); the rest render the other tiles whole.
// The production kernels (COUNT = 0, no SPLIT) render a (tilesX, tilesY, numFrames) grid over numFrames whole frames — frame
// blockIdx.z reads SceneBlock sb[blockIdx.z] and writes nRows·W pixels from out + sb->frame·nRows·W (and bright likewise; the
// block's own index, so that blockIdx.z is not live across the kernel).  A single frame (launch_render) is a grid of one frame;
// rm_render_batch launches the same kernels over many.
template <int BULB, int COUNT, bool ENV, bool TEX, bool SEC = true, int SPLIT = 0>
__global__ __launch_bounds__(256, render_waves(BULB, ENV, TEX, SEC)) void render_kernel(
    const SceneBlock *__restrict__ sb, RowMap map, int W, int H, int nRows, float4 *__restrict__ out, float4 *__restrict__ bright,
    unsigned long long *__restrict__ counters) {
  constexpr int CM = (COUNT == 3) ? 0 : COUNT;  // counting mode of the device code
  constexpr bool FRAMES = COUNT == 0 && SPLIT == 0;  // the production kernels: frame blockIdx.z of the grid
  if (FRAMES) sb += blockIdx.z;  // wave-uniform: the frame's own scene block
  unsigned long long t0 = 0, r0 = 0;
  if (COUNT == 3) { t0 = __builtin_amdgcn_s_memtime(); r0 = __builtin_amdgcn_s_memrealtime(); }
  // LDS copy of the object table for per-lane (divergent) material lookups; the single-bulb class reads one entry.
  __shared__ RmObject s_objs[BULB ? 1 : RM_MAX_OBJECTS];
  {
    const int nd = sb->numObjects * (int)(sizeof(RmObject) / 4);
    const uint32_t *src = reinterpret_cast<const uint32_t *>(sb->objs);
    uint32_t *dst = reinterpret_cast<uint32_t *>(s_objs);
    for (int i = threadIdx.x; i < nd; i += blockDim.x) dst[i] = src[i];
  }
  // the launches that read samplers build the byte→unorm table (wave-uniform condition; ends with a barrier)
  if (TEX || (ENV && (sb->s.features & (RM_FEAT_NIGHTSKY_BACKGROUND | RM_FEAT_SEA)))) initUnormTable();
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  // tile order: the workgroups of a grid start in blockIdx order; sb->tileOrder (if any) says which tile each one renders
  int tile = blockIdx.y * gridDim.x + blockIdx.x;
  const int32_t *order = sb->tileOrder;
  const int tsh = sb->tileShift, tw = 1 << tsh;  // wave-uniform (scalar): the tile is tw pixels wide, 64 / tw tall
  int tilesX = (int)gridDim.x;
  LightSplit split{-1, nullptr, 0};
  if (SPLIT) {  // one-wave workgroups, 1-D grid (launch_render)
    const int nl = sb->numLights, K = sb->splitTiles, b = (int)blockIdx.x;
    tilesX = (W + tw - 1) / tw;
    int h = b;  // position of the tile in tileOrder
    if (SPLIT == 1) {
      if (b < K * nl) { h = b / nl; split.part = b - h * nl; }
      else h = K + (b - K * nl);
    }
    tile = order[h];
    if (h < K) {  // K arrival counters, then per tile 64 pixels × (nl shadow results + the primary march's)
      split.tileIndex = h;
      split.slot = sb->splitStore + (((size_t)K + 63) & ~(size_t)63) + ((size_t)h * 64 + lane) * (size_t)(2 * nl + 6);
    }
  } else if (order && sb->tileCount == (int)(gridDim.x * gridDim.y)) {
    tile = order[tile];
  }
  const int tbx = tile % tilesX, tby = tile / tilesX;
  // the wave's start stamp waits in LDS (not in two scalar registers across the whole kernel — the register budget is tight)
  __shared__ unsigned long long s_c0[4];
  if (!SPLIT && sb->tileCost && lane == 0) s_c0[wave] = __builtin_amdgcn_s_memtime();
  const int x = (tbx * (blockDim.x >> 6) + wave) * tw + (lane & (tw - 1));
  const int r = tby * (64 >> tsh) + (lane >> tsh);
  if (x >= W || r >= nRows) return;
  const int y = map.frameRow(r);
  V4 col, br;
  Counters cnt{0, 0, 0, 0, 0, 0};
  bool hit;
  shadePixel<BULB, CM, optClass(ENV, TEX, SEC) | optSplit(SPLIT) | kShareBump | kPrep>(sb, s_objs, x, y, W, H, col, br, cnt, hit, split);
  if (SPLIT == 1 && split.part >= 0) {
    // A partial workgroup: its results are in memory.  The LAST of the tile's numLights workgroups to get here finishes the tile —
    // surface point, AO and the light sum from the stored results, no march (shadePixel in mode 2) — the others are done.  Release /
    // acquire at device scope around a counter per tile: the stores of the others are visible to the one that reads old == nl − 1.
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");  // this workgroup's records are written back before its arrival counts
    uint32_t *arrived = reinterpret_cast<uint32_t *>(sb->splitStore) + split.tileIndex;  // the counters precede the records (launch_render zeroes them)
    const int leader = __builtin_ctzll(__ballot(1));
    uint32_t old = 0;
    if ((int)__lane_id() == leader) old = __hip_atomic_fetch_add(arrived, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    old = __shfl(old, leader);
    if ((int)old != sb->numLights - 1) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // only the finisher invalidates its view before it reads the others' records
    split.part = -1;
    shadePixel<BULB, CM, optClass(ENV, TEX, SEC) | kSplitFinish | kShareBump | kPrep>(sb, s_objs, x, y, W, H, col, br, cnt, hit, split);
  }
  if (FRAMES) {
    const size_t f = (size_t)sb->frame * (size_t)nRows * (size_t)W;
    out += f;
    if (bright) bright += f;
  }
  const size_t o = (size_t)r * W + x;
  out[o] = make_float4(col.x, col.y, col.z, col.w);
  if (bright) bright[o] = make_float4(br.x, br.y, br.z, br.w);
  if (CM) {
    atomicAdd(&counters[0], cnt.evals);
    atomicAdd(&counters[1], cnt.iters);
    if (hit) atomicAdd(&counters[2], 1ull);
    if (cnt.shades) atomicAdd(&counters[6], cnt.shades);
    if (cnt.fbm9) atomicAdd(&counters[7], cnt.fbm9);
    if (cnt.fbmd8) atomicAdd(&counters[8], cnt.fbmd8);
    if (cnt.shapes) atomicAdd(&counters[9], cnt.shapes);
  }
  if (!SPLIT && sb->tileCost && sb->tileCount == (int)(gridDim.x * gridDim.y)) {  // wave-uniform
    const unsigned long long c1 = __builtin_amdgcn_s_memtime();
    int t2 = blockIdx.y * gridDim.x + blockIdx.x;  // recomputed rather than kept live
    if (sb->tileOrder) t2 = sb->tileOrder[t2];
    if ((int)__lane_id() == __builtin_ctzll(__ballot(1))) atomicAdd(&sb->tileCost[t2], (uint32_t)((c1 - s_c0[wave]) >> 6));
  }
  if (COUNT == 3) {
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    if ((int)__lane_id() == __builtin_ctzll(__ballot(1))) {  // first live lane of the wave
      atomicAdd(&counters[3], t1 - t0);
      atomicAdd(&counters[4], r1 - r0);
      // optional per-wave life span (100 MHz ticks) for occupancy timelines: counters[5] holds a device pointer or 0
      unsigned long long *spans = reinterpret_cast<unsigned long long *>(counters[5]);
      if (spans) {
        int t3 = blockIdx.y * gridDim.x + blockIdx.x;
        if (sb->tileOrder && sb->tileCount == (int)(gridDim.x * gridDim.y)) t3 = sb->tileOrder[t3];
        const size_t w = (size_t)t3 * (blockDim.x >> 6) + wave;
        spans[2 * w] = r0;
        spans[2 * w + 1] = r1;
      }
    }
  }
}

// sdMengerSponge's uniform prologue (frag:1052-1053), once per launch, with the device's own rm_math (bit-exactness with the
// oracle needs the contract's sin / cos / smoothstep, which only the device and the oracle implement).
RM_DEV void menger_uniforms(SceneBlock *sb) {
  sb->mengerAni = smoothstep_(-0.2f, 0.2f, -cos_(0.5f * sb->g.iTime));
  sb->mengerOff = 1.5f * sin_(0.01f * sb->g.iTime);
}
// one thread per scene block of the launch (one frame, or every frame of a batch), each with its own iTime
__global__ void scene_prep_batch_kernel(SceneBlock *sb, int n) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f < n) menger_uniforms(sb + f);
}

// ---- tile order ------------------------------------------------------------------------------------------
// The cost of a tile (one workgroup of render_kernel) spans three orders of magnitude: background tiles end after one
// evaluation, while an interior tile may hold ONE ray that creeps through a crevice for all 256 steps without ever
// converging — a sequential chain of ≈0.5 M instructions, ≈1 ms on its own.  Workgroups start in blockIdx order; with
// tiles in raster order such stragglers start at random times, the last of them late, and the kernel ends in a tail of a
// few lonely waves (profiles/r02_e_wave_timeline.md: the last 15 % of the kernel's life had ≤ 3 waves resident).
// Starting the heavy tiles first removes the tail: 3.11 → 2.43 ms on the 4K bulb frame with measured costs
// (profiles/r02_f_tile_order.md).  Nothing about a pixel changes, only when its tile starts.
// Where the straggler pixels are cannot be told from a sparse pre-pass (tried: 8 sample rays per tile, 0.24 ms, no gain);
// what does know is the previous frame.  render_kernel adds every wave's shader-cycle span to tileCost[tile]; the next
// frame of the same size on the same stream starts its tiles in descending order of those costs (a renderer's consecutive
// frames are nearly the same picture; a frame with no history, or after a change of size, runs in raster order).
// The order is a two-launch bucket sort by log2(cost): tile_hist_kernel counts, tile_scatter_kernel places.
constexpr int kOrderBuckets = 16;
RM_DEV int orderBucket(uint32_t cost) {  // heaviest = bucket 0; costs are shader cycles / 64, i.e. ≈2^5 … 2^17
  const int lg = 31 - __builtin_clz(cost | 1u);
  const int b = 17 - lg;
  return b < 0 ? 0 : (b >= kOrderBuckets ? kOrderBuckets - 1 : b);
}
__global__ __launch_bounds__(256) void tile_hist_kernel(const uint32_t *__restrict__ cost, int n, uint32_t *__restrict__ hist) {
  __shared__ uint32_t s_cnt[kOrderBuckets];
  if (threadIdx.x < kOrderBuckets) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = i < n ? orderBucket(cost[i]) : -1;
  for (int k = 0; k < kOrderBuckets; k++) {  // wave-aggregated: one LDS atomic per wave and bucket present
    const unsigned long long m = __ballot(b == k);
    if (m && (int)__lane_id() == __builtin_ctzll(m)) atomicAdd(&s_cnt[k], (uint32_t)__builtin_popcountll(m));
  }
  __syncthreads();
  if (threadIdx.x < kOrderBuckets && s_cnt[threadIdx.x]) atomicAdd(&hist[threadIdx.x], s_cnt[threadIdx.x]);
}
// hist[0..15] = bucket sizes (from tile_hist_kernel), hist[16..31] = cursors (zero on entry).  Consumes (clears) cost[] unless
// `keep` (the last sort of a settled picture: the costs stay as the stale costs of whatever picture comes next).
__global__ __launch_bounds__(256) void tile_scatter_kernel(uint32_t *__restrict__ cost, int n, uint32_t *__restrict__ hist,
                                                            int32_t *__restrict__ order, int keep) {
  __shared__ uint32_t s_cnt[kOrderBuckets], s_base[kOrderBuckets];
  if (threadIdx.x < kOrderBuckets) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = i < n ? orderBucket(cost[i]) : -1;
  uint32_t rank = 0;  // position inside the block's share of bucket b
  for (int k = 0; k < kOrderBuckets; k++) {
    const unsigned long long m = __ballot(b == k);
    if (!m) continue;
    uint32_t waveBase = 0;
    if ((int)__lane_id() == __builtin_ctzll(m)) waveBase = atomicAdd(&s_cnt[k], (uint32_t)__builtin_popcountll(m));
    waveBase = __shfl(waveBase, __builtin_ctzll(m));
    if (b == k) rank = waveBase + (uint32_t)__builtin_popcountll(m & ((1ull << __lane_id()) - 1ull));
  }
  __syncthreads();
  if (threadIdx.x < kOrderBuckets) {
    uint32_t start = 0;  // exclusive scan of the bucket sizes, heaviest bucket first
    for (int k = 0; k < (int)threadIdx.x; k++) start += hist[k];
    s_base[threadIdx.x] = start + (s_cnt[threadIdx.x] ? atomicAdd(&hist[kOrderBuckets + threadIdx.x], s_cnt[threadIdx.x]) : 0u);
  }
  __syncthreads();
  if (i < n) {
    order[s_base[b] + rank] = i;
    if (!keep) cost[i] = 0u;  // the next frame accumulates afresh
  }
}

// A frame WITHOUT usable history (the first of its size on a stream, or any frame whose scene or camera differs from the one that
// recorded the costs): stand-in costs from geometry alone.  One thread per tile: the tile centre's primary ray against every
// object's world-space bounding ball (SceneBlock::objBall) — closest approach inside [0.6·R, R + the tile's footprint] is a
// silhouette candidate (the rays that graze an object march longest), inside 0.6·R an interior tile, anything else background;
// the bucket sort above then starts rings first, interiors next, background last, raster order within a class.  Measured on cold
// 4K frames (scripts/cold_order_probe.py, profiles/r04_k_geometric_order.md): bulb 2.85 → 2.26 ms (measured costs: 1.99),
// directional_light_2.json 1.89 → 1.77-1.81, reflections_complex.json 8.70 → 8.39-8.44.  Same pixels.
__global__ __launch_bounds__(256) void tile_geom_kernel(const SceneBlock *__restrict__ sb, RowMap map, int W, int H, int nRows, int tilesX,
                                                        int tileW, int tileH, int n, const uint32_t *__restrict__ stale,
                                                        uint32_t *__restrict__ cost, int combine, int ringLog2, int dilate) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int x = (i % tilesX) * tileW + tileW / 2, r = (i / tilesX) * tileH + tileH / 2;
  x = x < W ? x : W - 1;
  r = r < nRows ? r : nRows - 1;
  V3 ro, rd;
  primaryRay(sb, x, map.frameRow(r), W, H, ro, rd);
  // angle of one tile seen from the eye ≈ the distance between neighbouring tile centres' directions
  V3 ro2, rd2;
  const int span = tileW > tileH ? tileW : tileH;  // the tile's larger side, in pixels
  primaryRay(sb, x < W - span ? x + span : x - span, map.frameRow(r), W, H, ro2, rd2);
  const float foot = len(sub(rd2, rd));
  int cls = 0;
  const int no = sb->numObjects;
  for (int k = 0; k < no; k++) {
    const V3 v = v3(sb->objBall[k][0] - ro.x, sb->objBall[k][1] - ro.y, sb->objBall[k][2] - ro.z);
    const float R = sb->objBall[k][3], tca = dot(v, rd);
    const float q2 = dot(v, v) - tca * tca, hi = fma(foot, tca, R), lo = 0.6f * R;
    if (tca > 0.0f && q2 <= hi * hi) cls = (q2 >= lo * lo) ? 2 : (cls > 1 ? cls : 1);
  }
  const uint32_t gv = cls == 2 ? (1u << ringLog2) : (cls == 1 ? (1u << 11) : (1u << 4));
  // combine: a frame of the same size rendered a DIFFERENT picture before (a moving camera) — its measured costs are stale but near;
  // the heavier of the two estimates decides.  dilate: the stale estimate of a tile is the heaviest within that many tiles of it (a
  // silhouette that the camera's motion shifted by a few tiles is still where its heavy tiles are looked for)
  uint32_t sv = 0u;
  if (combine) {
    const int tx = i % tilesX, ty = i / tilesX, tilesY = (n + tilesX - 1) / tilesX;
    for (int dy = -dilate; dy <= dilate; dy++)
      for (int dx = -dilate; dx <= dilate; dx++) {
        const int nx = tx + dx, ny = ty + dy;
        if (nx < 0 || ny < 0 || nx >= tilesX || ny >= tilesY || ny * tilesX + nx >= n) continue;
        const uint32_t c = stale[ny * tilesX + nx];
        sv = c > sv ? c : sv;
      }
  }
  cost[i] = sv > gv ? sv : gv;
}

// clamp → ×255 → round-half-up, vertical flip (src/realtime.cpp:337-338 + GL's RGBA8 conversion).  blockIdx.z = frame: each
// frame is flipped within itself.
__global__ void to_rgba8_kernel(const float4 *__restrict__ in, uchar4 *__restrict__ out, int W, int H) {
  int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= W) return;
  const size_t base = (size_t)blockIdx.z * W * H;
  float4 c = in[base + (size_t)y * W + x];
  auto q = [](float v) { v = !(v > 0.0f) ? 0.0f : (v > 1.0f ? 1.0f : v); return (unsigned char)(v * 255.0f + 0.5f); };  // NaN → 0 (UB12)
  out[base + (size_t)(H - 1 - y) * W + x] = make_uchar4(q(c.x), q(c.y), q(c.z), q(c.w));
}

// packed tiles → RGBA8, rows as they are (the multi-GPU shard's share of to_rgba8_kernel's conversion)
__global__ void tiles_to_rgba8_kernel(const float4 *__restrict__ in, uchar4 *__restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 c = in[i];
  auto q = [](float v) { v = !(v > 0.0f) ? 0.0f : (v > 1.0f ? 1.0f : v); return (unsigned char)(v * 255.0f + 0.5f); };  // NaN → 0 (UB12)
  out[i] = make_uchar4(q(c.x), q(c.y), q(c.z), q(c.w));
}
// gathered RGBA8 slots → frame rows (flip: row 0 of the output is the top of the image, as rm_frame_to_rgba8 writes it)
__global__ void deinterleave_rgba8_kernel(const uchar4 *__restrict__ in, uchar4 *__restrict__ out, int W, int H, int tileRows,
                                          int numShards, int strideRows, int flip, int relief) {
  int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;  // y = frame row (0 = bottom)
  if (x >= W) return;
  int shard, localTile;
  tile_owner(y / tileRows, numShards, relief, shard, localTile);
  int before = shard * strideRows;
  if (strideRows == 0)
    for (int s = 0; s < shard; s++) before += shard_rows(H, tileRows, s, numShards, relief);
  int local = localTile * tileRows + (y % tileRows);
  out[(size_t)(flip ? H - 1 - y : y) * W + x] = in[(size_t)(before + local) * W + x];
}
// gathered[shard-major packed rows] → frame rows
__global__ void deinterleave_kernel(const float4 *__restrict__ in, float4 *__restrict__ out, int W, int H, int tileRows,
                                    int numShards, int strideRows, int relief) {
  int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;  // y = frame row
  if (x >= W) return;
  int shard, localTile;
  tile_owner(y / tileRows, numShards, relief, shard, localTile);
  // rows owned by shards < shard, plus this shard's rows before frame row y
  int before = shard * strideRows;
  if (strideRows == 0)
    for (int s = 0; s < shard; s++) before += shard_rows(H, tileRows, s, numShards, relief);
  int local = localTile * tileRows + (y % tileRows);
  out[(size_t)y * W + x] = in[(size_t)(before + local) * W + x];
}

// ---- the launch functions (rm_internal.h) ------------------------------------------------------------------------------------
// Each frame's sponge uniforms, computed on the device: stream-ordered between the upload of the n blocks and the kernels that read them.
int launch_scene_prep(SceneBlock *sb, int n, hipStream_t stream) {
  hipLaunchKernelGGL(scene_prep_batch_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, sb, n);
  HIP_OK(hipGetLastError());
  return RM_OK;
}

// This frame's launch order — from the previous frame's tile costs or from geometry — ahead of the render.
int launch_tile_order(const TileOrderPlan &p, const RenderLaunch &r, int tileWpx, int tileH, int tileCount) {
  const dim3 sgrid((tileCount + 255) / 256);
  uint32_t *sortCost = p.cost;
  if (p.byGeom) {  // estimates into their own array (the kernel reads the stale costs of a tile's neighbourhood), stale costs cleared after
    hipLaunchKernelGGL(tile_geom_kernel, sgrid, dim3(256), 0, r.stream, r.sb, r.map, r.W, r.H, r.nRows, (int)r.grid.x, tileWpx, tileH,
                       tileCount, p.cost, p.cost2, p.combine ? 1 : 0, (p.combine ? p.ringLog2 : 16), p.dilate);
    HIP_OK(hipMemsetAsync(p.cost, 0, (size_t)tileCount * sizeof(uint32_t), r.stream));
    sortCost = p.cost2;
  }
  HIP_OK(hipMemsetAsync(p.hist, 0, 2 * kOrderBuckets * sizeof(uint32_t), r.stream));
  hipLaunchKernelGGL(tile_hist_kernel, sgrid, dim3(256), 0, r.stream, sortCost, tileCount, p.hist);
  hipLaunchKernelGGL(tile_scatter_kernel, sgrid, dim3(256), 0, r.stream, sortCost, tileCount, p.hist, p.order, p.lastSort ? 1 : 0);
  return RM_OK;
}

// The wavefront pipeline's generations: primary (gen 0) or bounce march, surface, shadow marches, lighting.
template <bool SKIP>
void launch_wavefront(const RenderLaunch &r, const Wavefront &wf, int bounces, int numLights, int numCUs) {
  const dim3 pgrid(wf.primaryWaves), mgrid(wf.shadowWaves), mblock(64), dense(numCUs * 16), block(256);
  for (int gen = 0; gen <= bounces; gen++) {
    if (gen == 0) hipLaunchKernelGGL((wf_march_kernel<0, SKIP>), pgrid, mblock, 0, r.stream, r.sb, r.map, r.W, r.H, r.nRows, r.o, r.b, wf.ws, gen, wf.flush, wf.pixelChunk, wf.maxChunk, wf.slotChunk);
    else hipLaunchKernelGGL((wf_march_kernel<1, SKIP>), pgrid, mblock, 0, r.stream, r.sb, r.map, r.W, r.H, r.nRows, r.o, r.b, wf.ws, gen, wf.flush, wf.rayChunk, wf.maxChunk, wf.slotChunk);
    hipLaunchKernelGGL(wf_surface_kernel<SKIP>, dense, block, 0, r.stream, r.sb, r.map, r.W, r.H, wf.ws, gen);
    if (numLights > 0) hipLaunchKernelGGL((wf_march_kernel<2, SKIP>), mgrid, mblock, 0, r.stream, r.sb, r.map, r.W, r.H, r.nRows, r.o, r.b, wf.ws, gen, wf.flush, wf.rayChunk, wf.maxChunk, wf.slotChunk);
    hipLaunchKernelGGL(wf_light_kernel, dense, block, 0, r.stream, r.sb, r.map, r.W, r.H, r.o, r.b, wf.ws, gen, bounces);
  }
}
void launch_wavefront(bool skip, const RenderLaunch &r, const Wavefront &wf, int bounces, int numLights, int numCUs) {
  if (skip) launch_wavefront<true>(r, wf, bounces, numLights, numCUs);
  else launch_wavefront<false>(r, wf, bounces, numLights, numCUs);
}

// render_kernel<BULB, COUNT, ENV, TEX, SEC, SPLIT>: the bulb class and the generic table walk, plain and counted, without
// procedural layers or textures; the generic kernel with either or both.  Features a launch does not need are compiled out so the
// common kernels keep their register budget.
template <int BULB, int COUNT, bool ENV, bool TEX, bool SEC = true, int SPLIT = 0>
void launch_kernel(const RenderLaunch &r) {
  hipLaunchKernelGGL((render_kernel<BULB, COUNT, ENV, TEX, SEC, SPLIT>), r.grid, r.block, 0, r.stream, r.sb, r.map, r.W, r.H, r.nRows, r.o, r.b, r.dc);
}
// the counted (1: reference work, 2: executed work) and clock-stamped (3) launches
template <int BULB>
void launch_counted(int count, const RenderLaunch &r) {
  if (count == 1) launch_kernel<BULB, 1, false, false>(r);
  else if (count == 2) launch_kernel<BULB, 2, false, false>(r);
  else launch_kernel<BULB, 3, false, false>(r);
}
// A batch (rm_render_batch, one class for every frame of the launch) comes with count = 0 and no light split, so it reaches only
// the production kernels; the counted and split kernels render single frames.
int dispatch_render(const FrameClass &fc, int count, bool plainBulb, const SplitPlan &ls, int numLights, int tileCount,
                    const RenderLaunch &r) {
  const int bulbClass = bulb_class(fc, plainBulb);
  if (count) {
    // the layer / sampler kernels count the reference's work only (they have no shortcuts to count apart); the bulb keeps the general form
    if (fc.envFeatures && fc.textured) launch_kernel<0, 1, true, true>(r);
    else if (fc.envFeatures) launch_kernel<0, 1, true, false>(r);
    else if (fc.textured) launch_kernel<0, 1, false, true>(r);
    else if (fc.bulb) launch_counted<kBulbGeneral>(count, r);
    else launch_counted<0>(count, r);
  } else if (!bulbClass && !fc.envFeatures && !fc.textured && !fc.secondary && ls.tiles > 0) {
    // light split: the heavy tiles one light per workgroup first, every other tile behind them in the same grid; the last of a
    // tile's workgroups to finish its march finishes the tile.  (A second launch for the finish cost 35-45 µs per frame —
    // more than the split gains on throughput-bound frames; the same launch on a side stream gained nothing.)
    HIP_OK(hipMemsetAsync(ls.store, 0, (size_t)ls.tiles * sizeof(uint32_t), r.stream));  // the tiles' arrival counters
    RenderLaunch split = r;
    split.grid = dim3((unsigned)(ls.tiles * numLights + tileCount - ls.tiles));
    split.block = dim3(64);
    launch_kernel<0, 0, false, false, false, 1>(split);
  } else {
    dispatch_class(bulbClass, fc.envFeatures, fc.textured, fc.secondary, [&](auto c) {
      using K = decltype(c);
      launch_kernel<K::bulb, 0, K::env, K::tex, K::sec>(r);
    });
  }
  return RM_OK;
}

int launch_to_rgba8(const float *d_rgba, uint8_t *d_out, int W, int H, int numFrames, hipStream_t stream) {
  dim3 grid((W + 255) / 256, H, numFrames), block(256);
  hipLaunchKernelGGL(to_rgba8_kernel, grid, block, 0, stream,
                     reinterpret_cast<const float4 *>(d_rgba), reinterpret_cast<uchar4 *>(d_out), W, H);
  HIP_OK(hipGetLastError());
  return RM_OK;
}
int launch_tiles_to_rgba8(const float *d_tiles, uint8_t *d_tiles8, size_t n, hipStream_t stream) {
  hipLaunchKernelGGL(tiles_to_rgba8_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                     reinterpret_cast<const float4 *>(d_tiles), reinterpret_cast<uchar4 *>(d_tiles8), n);
  HIP_OK(hipGetLastError());
  return RM_OK;
}
int launch_deinterleave_rgba8(const uint8_t *d_gathered8, uint8_t *d_frame8, int W, int H, int tileRows, int numShards,
                              int shardStrideRows, int flip, int relief, hipStream_t stream) {
  dim3 grid((W + 255) / 256, H), block(256);
  hipLaunchKernelGGL(deinterleave_rgba8_kernel, grid, block, 0, stream,
                     reinterpret_cast<const uchar4 *>(d_gathered8), reinterpret_cast<uchar4 *>(d_frame8), W, H, tileRows, numShards,
                     shardStrideRows, flip, relief);
  HIP_OK(hipGetLastError());
  return RM_OK;
}
int launch_deinterleave(const float *d_gathered, float *d_frame, int W, int H, int tileRows, int numShards, int shardStrideRows,
                        int relief, hipStream_t stream) {
  dim3 grid((W + 255) / 256, H), block(256);
  hipLaunchKernelGGL(deinterleave_kernel, grid, block, 0, stream,
                     reinterpret_cast<const float4 *>(d_gathered), reinterpret_cast<float4 *>(d_frame), W, H, tileRows,
                     numShards, shardStrideRows, relief);
  HIP_OK(hipGetLastError());
  return RM_OK;
}

}  // namespace rm
