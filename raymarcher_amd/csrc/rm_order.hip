// rm_order.hip — rm_rays_order and rm_rays_restore (gfx950 only): the coherence ordering of an RmRay array and its inverse.
// include/raymarcher_amd.h has the definitions, rm_ray_key.h the key.  Everything of the two entry points is here, as
// rm_sdf_mesh_blocks is in rm_blocks.hip.
//   1. order_bounds_kernel: lo and hi of the five coordinates over a workgroup's rays — lanes, then the wave (shuffles), then LDS —
//      one partial per workgroup; order_bounds_final_kernel merges the partials.  Minima and maxima are exact, so a store-and-merge
//      gives the bits of any other order; no float atomic.
//   2. order_keys_kernel: the key of every ray into keys[0] (and d_keys), the identity into idx[0], and the OR and the AND of all
//      keys (one integer atomic pair per workgroup): a digit on which OR and AND agree is the same in every key.
//   3. a least-significant-digit radix sort of the (key, index) pairs, 8 bits per pass, ping-pong between two buffer pairs.  Per
//      pass: order_hist_kernel (a workgroup's digit histogram of its tile), order_scan_kernel (a launch of its own: workgroup d
//      turns digit d's counts over the tiles into exclusive offsets) and order_scatter_kernel (ranks the tile's keys stably, stages
//      them by digit in LDS and stores each digit's run as contiguous words).  A pass whose digit is the same in every key — its
//      histogram has one bucket — is skipped by all three kernels: each works out from OR ^ AND which passes ran before it and so
//      which buffer pair holds the data.  No kernel waits for another workgroup.
//   4. order_emit_kernel: d_order and, gathered through it, d_sorted.
// order_restore_kernel is rm_rays_restore: one lane per 16 bytes.
#include <hip/hip_runtime.h>

#include <mutex>
#include <string>

#include "../../include/raymarcher_amd.h"
#include "rm_compact.hip.h"
#include "rm_internal.h"
#include "rm_ray_key.h"

namespace rm {

#define RO_DEV __device__ __forceinline__

constexpr int kSortLanes = 256, kSortWaves = kSortLanes / 64, kSortRounds = RM_RAYS_ORDER_TILE / kSortLanes;  // 8 keys per lane
constexpr int kSortTile = RM_RAYS_ORDER_TILE, kWaveShare = kSortTile / kSortWaves;                            // 512 keys per wave
static_assert(kSortRounds * kSortLanes == kSortTile && kSortLanes == 256, "a lane per digit, whole rounds per tile");
constexpr int kBoundsGroups = 512, kKeyGroups = 2048;  // the most workgroups of the two grid-stride kernels

// ---- 1. bounds -------------------------------------------------------------------------------------------------------------------
RO_DEV bool load_coords(const float4 *__restrict__ rays, size_t i, float c[rk::kCoords]) {
  const float4 a = rays[2 * i], b = rays[2 * i + 1];
  const float o[3] = {a.x, a.y, a.z}, d[3] = {b.x, b.y, b.z};
  return rk::coords(o, d, c);
}
// the merge of a workgroup's 256 lanes: valid in thread 0
RO_DEV void group_bounds(rk::Bounds &b, float (*waveLo)[rk::kCoords], float (*waveHi)[rk::kCoords]) {
#pragma unroll
  for (int k = 0; k < rk::kCoords; k++) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      b.lo[k] = rk::lower(b.lo[k], __shfl_xor(b.lo[k], d));
      b.hi[k] = rk::upper(b.hi[k], __shfl_xor(b.hi[k], d));
    }
  }
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (lane == 0u) {
#pragma unroll
    for (int k = 0; k < rk::kCoords; k++) waveLo[wave][k] = b.lo[k], waveHi[wave][k] = b.hi[k];
  }
  __syncthreads();
  if (threadIdx.x == 0u) {
    for (unsigned w = 1; w < 4u; w++) {
#pragma unroll
      for (int k = 0; k < rk::kCoords; k++) b.lo[k] = rk::lower(b.lo[k], waveLo[w][k]), b.hi[k] = rk::upper(b.hi[k], waveHi[w][k]);
    }
  }
}
RO_DEV void store_bounds(const rk::Bounds &b, float *out) {
#pragma unroll
  for (int k = 0; k < rk::kCoords; k++) out[k] = b.lo[k], out[rk::kCoords + k] = b.hi[k];
}
RO_DEV rk::Bounds read_bounds(const float *in) {
  rk::Bounds b;
#pragma unroll
  for (int k = 0; k < rk::kCoords; k++) b.lo[k] = in[k], b.hi[k] = in[rk::kCoords + k];
  return b;
}

__global__ __launch_bounds__(256) void order_bounds_kernel(const float4 *__restrict__ rays, unsigned n, float *__restrict__ partials) {
  __shared__ float waveLo[4][rk::kCoords], waveHi[4][rk::kCoords];
  rk::Bounds b;
  rk::bounds_empty(b);
  for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) {
    float c[rk::kCoords];
    if (load_coords(rays, i, c)) rk::bounds_add(b, c);
  }
  group_bounds(b, waveLo, waveHi);
  if (threadIdx.x == 0u) store_bounds(b, partials + 2 * rk::kCoords * (size_t)blockIdx.x);
}
// one workgroup: the partials into head[0 … 9], and the start values of the keys' OR and AND
__global__ __launch_bounds__(256) void order_bounds_final_kernel(const float *__restrict__ partials, unsigned groups, float *__restrict__ bounds,
                                                                 unsigned long long *__restrict__ orAnd) {
  __shared__ float waveLo[4][rk::kCoords], waveHi[4][rk::kCoords];
  rk::Bounds b;
  rk::bounds_empty(b);
  for (unsigned g = threadIdx.x; g < groups; g += 256u) rk::bounds_merge(b, read_bounds(partials + 2 * rk::kCoords * (size_t)g));
  group_bounds(b, waveLo, waveHi);
  if (threadIdx.x == 0u) {
    store_bounds(b, bounds);
    orAnd[0] = 0ull;
    orAnd[1] = ~0ull;
  }
}

// ---- 2. keys ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void order_keys_kernel(const float4 *__restrict__ rays, unsigned n, int originBits, int dirBits,
                                                         const float *__restrict__ bounds, unsigned long long *__restrict__ keys,
                                                         uint32_t *__restrict__ idx, unsigned long long *__restrict__ userKeys,
                                                         unsigned long long *__restrict__ orAnd) {
  __shared__ unsigned long long waveOr[4], waveAnd[4];
  const rk::Bounds b = read_bounds(bounds);
  unsigned long long any = 0ull, all = ~0ull;
  for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) {
    float c[rk::kCoords];
    const unsigned long long key = load_coords(rays, i, c) ? rk::valid_key(c, b, originBits, dirBits) : rk::invalid_key(originBits, dirBits);
    keys[i] = key;
    idx[i] = (uint32_t)i;
    if (userKeys) userKeys[i] = key;
    any |= key;
    all &= key;
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    any |= __shfl_xor(any, d);
    all &= __shfl_xor(all, d);
  }
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (lane == 0u) waveOr[wave] = any, waveAnd[wave] = all;
  __syncthreads();
  if (threadIdx.x == 0u) {
    atomicOr(&orAnd[0], waveOr[0] | waveOr[1] | waveOr[2] | waveOr[3]);
    atomicAnd(&orAnd[1], waveAnd[0] & waveAnd[1] & waveAnd[2] & waveAnd[3]);
  }
}

// ---- 3. the sort -----------------------------------------------------------------------------------------------------------------
// What a kernel of pass `pass` needs to know of the passes before it: whether its own digit is the same in every key (then it
// leaves at once), and how many passes before it were not skipped — an odd number: the data is in the second buffer pair.
// pass = the number of passes: where the sorted pairs are.
struct PassInfo { bool skipped; unsigned from; };
RO_DEV PassInfo pass_info(const unsigned long long *__restrict__ orAnd, int pass) {
  const unsigned long long differ = orAnd[0] ^ orAnd[1];
  unsigned ran = 0;
  for (int q = 0; q < pass; q++) ran += ((differ >> (8 * q)) & 0xffull) != 0ull ? 1u : 0u;
  return PassInfo{((differ >> (8 * pass)) & 0xffull) == 0ull, ran & 1u};
}
struct SortBuffers { unsigned long long *keys[2]; uint32_t *idx[2]; };

RO_DEV unsigned digit_of(unsigned long long key, int pass) { return (unsigned)(key >> (8 * pass)) & 0xffu; }
// the live lanes of the wave that hold digit d: eight ballots, 64 bits wide each
RO_DEV unsigned long long digit_peers(unsigned d, bool live) {
  unsigned long long m = __ballot(live);
#pragma unroll
  for (int b = 0; b < 8; b++) {
    const bool bit = ((d >> b) & 1u) != 0u;
    const unsigned long long v = __ballot(bit);
    m &= bit ? v : ~v;
  }
  return m;
}

// hist[d·numTiles + tile] = the tile's keys with digit d
__global__ __launch_bounds__(kSortLanes) void order_hist_kernel(SortBuffers s, unsigned n, int pass, const unsigned long long *__restrict__ orAnd,
                                                                uint32_t *__restrict__ hist) {
  __shared__ unsigned count[256];
  const PassInfo info = pass_info(orAnd, pass);
  if (info.skipped) return;
  const unsigned long long *__restrict__ keys = s.keys[info.from];
  count[threadIdx.x] = 0u;
  __syncthreads();
  const unsigned lane = threadIdx.x & 63u;
  const size_t base = (size_t)blockIdx.x * kSortTile;
#pragma unroll
  for (int r = 0; r < kSortRounds; r++) {
    const size_t i = base + (size_t)r * kSortLanes + threadIdx.x;
    const bool live = i < n;
    const unsigned d = live ? digit_of(keys[i], pass) : 0u;
    const unsigned long long peers = digit_peers(d, live);
    if (live && lanes_below(peers, lane) == 0u) atomicAdd(&count[d], (unsigned)__popcll(peers));  // one add per digit and wave
  }
  __syncthreads();
  hist[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = count[threadIdx.x];
}

// Workgroup d turns digit d's numTiles counts into exclusive offsets in place and stores their sum.
__global__ __launch_bounds__(1024) void order_scan_kernel(uint32_t *__restrict__ hist, unsigned numTiles, int pass,
                                                          const unsigned long long *__restrict__ orAnd, uint32_t *__restrict__ totals) {
  __shared__ uint32_t waveSum[16];
  if (pass_info(orAnd, pass).skipped) return;
  uint32_t *mine = hist + (size_t)blockIdx.x * (size_t)numTiles;
  uint32_t carry = 0;  // the same in every lane
  for (unsigned base = 0; base < numTiles; base += 1024u) {
    const unsigned i = base + threadIdx.x;
    const ScanRound<uint32_t> r = scan_round_1024(i < numTiles ? mine[i] : 0u, waveSum);
    if (i < numTiles) mine[i] = carry + r.before;
    carry += r.all;
  }
  if (threadIdx.x == 0u) totals[blockIdx.x] = carry;
}

// A workgroup scatters its tile.  Wave w holds keys w·512 … w·512 + 511 of the tile, 64 consecutive keys per round, so the order
// (wave, round, lane) is the input order.  A key's place among the tile's keys of its digit = the keys of that digit in the waves
// before (waveCount, after the rounds) + those in this wave's earlier rounds (waveCount, as the rounds run) + those in lower lanes
// (the ballots).  The pairs are staged at digitStart[digit] + that place, and position j of the staging goes to the digit's offset
// for this tile + (j − digitStart[digit]): consecutive lanes store consecutive words for as long as the digit lasts.
__global__ __launch_bounds__(kSortLanes) void order_scatter_kernel(SortBuffers s, unsigned n, int pass, const unsigned long long *__restrict__ orAnd,
                                                                   const uint32_t *__restrict__ hist, const uint32_t *__restrict__ totals) {
  __shared__ unsigned waveCount[kSortWaves][256];
  __shared__ unsigned digitStart[256], globalBase[256];
  __shared__ unsigned waveSumTile[kSortWaves], waveSumAll[kSortWaves];
  __shared__ unsigned long long stagedKeys[kSortTile];
  __shared__ uint32_t stagedIdx[kSortTile];
  const PassInfo info = pass_info(orAnd, pass);
  if (info.skipped) return;
  const unsigned long long *__restrict__ srcKeys = s.keys[info.from];
  const uint32_t *__restrict__ srcIdx = s.idx[info.from];
  unsigned long long *__restrict__ dstKeys = s.keys[info.from ^ 1u];
  uint32_t *__restrict__ dstIdx = s.idx[info.from ^ 1u];
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const size_t base = (size_t)blockIdx.x * kSortTile;
  const unsigned inTile = n - base < (size_t)kSortTile ? (unsigned)(n - base) : (unsigned)kSortTile;
#pragma unroll
  for (int w = 0; w < kSortWaves; w++) waveCount[w][threadIdx.x] = 0u;
  __syncthreads();
  unsigned long long key[kSortRounds];
  uint32_t index[kSortRounds];
  unsigned place[kSortRounds];
#pragma unroll
  for (int r = 0; r < kSortRounds; r++) {
    const unsigned local = wave * kWaveShare + (unsigned)r * 64u + lane;
    const bool live = local < inTile;
    key[r] = live ? srcKeys[base + local] : 0ull;
    index[r] = live ? srcIdx[base + local] : 0u;
    const unsigned d = digit_of(key[r], pass);
    const unsigned long long peers = digit_peers(d, live);
    const unsigned before = waveCount[wave][d];  // this wave's row: only its own lanes write it
    place[r] = before + lanes_below(peers, lane);
    __syncthreads();
    if (live && lanes_below(peers, lane) == 0u) waveCount[wave][d] = before + (unsigned)__popcll(peers);
    __syncthreads();
  }
  {  // lane = digit: the counts of the waves into offsets, the digits' starts in the tile and in the whole array
    const unsigned d = threadIdx.x;
    unsigned inTileOfDigit = 0;
#pragma unroll
    for (int w = 0; w < kSortWaves; w++) {
      const unsigned c = waveCount[w][d];
      waveCount[w][d] = inTileOfDigit;
      inTileOfDigit += c;
    }
    const unsigned inAllOfDigit = totals[d];
    unsigned a = inTileOfDigit, b = inAllOfDigit;  // inclusive within the wave
#pragma unroll
    for (unsigned k = 1; k < 64u; k <<= 1) {
      const unsigned ta = __shfl_up(a, k), tb = __shfl_up(b, k);
      if (lane >= k) a += ta, b += tb;
    }
    if (lane == 63u) waveSumTile[wave] = a, waveSumAll[wave] = b;
    __syncthreads();
    unsigned beforeTile = 0, beforeAll = 0;
    for (unsigned w = 0; w < wave; w++) beforeTile += waveSumTile[w], beforeAll += waveSumAll[w];
    digitStart[d] = beforeTile + a - inTileOfDigit;
    globalBase[d] = beforeAll + b - inAllOfDigit + hist[(size_t)d * gridDim.x + blockIdx.x];
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kSortRounds; r++) {
    const unsigned local = wave * kWaveShare + (unsigned)r * 64u + lane;
    if (local < inTile) {
      const unsigned d = digit_of(key[r], pass);
      const unsigned at = digitStart[d] + waveCount[wave][d] + place[r];  // below inTile: the places of a digit are dense
      if (at < (unsigned)kSortTile) {  // always; the bound is checked all the same, next to the store
        stagedKeys[at] = key[r];
        stagedIdx[at] = index[r];
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kSortRounds; r++) {
    const unsigned j = (unsigned)r * kSortLanes + threadIdx.x;
    if (j < inTile) {
      const unsigned long long k = stagedKeys[j];
      const unsigned d = digit_of(k, pass);
      const size_t to = (size_t)globalBase[d] + (j - digitStart[d]);  // below n: the offsets count exactly the array's keys
      if (to < n) {  // always, likewise
        dstKeys[to] = k;
        dstIdx[to] = stagedIdx[j];
      }
    }
  }
}

// ---- 4. the outputs --------------------------------------------------------------------------------------------------------------
// One lane per 16 bytes of d_sorted: lane 2·k + part copies that half of ray order[k]; part 0 also stores order[k].
__global__ __launch_bounds__(256) void order_emit_kernel(SortBuffers s, unsigned n, int numPasses, const unsigned long long *__restrict__ orAnd,
                                                         const float4 *__restrict__ rays, int32_t *__restrict__ order, float4 *__restrict__ sorted) {
  const size_t g = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (g >= 2 * (size_t)n) return;
  const uint32_t *__restrict__ idx = s.idx[pass_info(orAnd, numPasses).from];
  const size_t k = g >> 1, part = g & 1u;
  const uint32_t from = idx[k];  // below n: a permutation of the identity the keys kernel stored
  if (part == 0u) order[k] = (int32_t)from;
  if (sorted && from < n) sorted[g] = rays[2 * (size_t)from + part];
}

// rm_rays_restore: lane g holds 16 bytes of row g / parts.  An entry of the order outside [0, numRows) is skipped.
__global__ __launch_bounds__(256) void order_restore_kernel(const uint4 *__restrict__ rows, const int32_t *__restrict__ order, unsigned numRows,
                                                            unsigned parts, uint4 *__restrict__ out) {
  const size_t g = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (g >= (size_t)numRows * parts) return;
  const size_t k = parts == 2u ? g >> 1 : g, part = parts == 2u ? (g & 1u) : 0u;
  const int32_t to = order[k];
  if (to < 0 || (unsigned)to >= numRows) return;
  out[(size_t)to * parts + part] = rows[g];
}

// The workspace of a call: 24 B per ray — two key buffers, two index buffers —, the histograms (1 KB per tile), the digits' totals,
// the bounds' partials, then 256 B of head: the bounds and, 64 B in, the keys' OR and AND.  Measured where mem is null.
struct OrderWs { SortBuffers sb; uint32_t *hist, *totals; float *partials, *bounds; unsigned long long *orAnd; size_t bytes; };
static OrderWs order_workspace(size_t n, size_t numTiles, void *mem) {
  Carve c(mem);
  OrderWs w;
  w.sb.keys[0] = c.take<unsigned long long>(n);
  w.sb.keys[1] = c.take<unsigned long long>(n);
  w.sb.idx[0] = c.take<uint32_t>(n);
  w.sb.idx[1] = c.take<uint32_t>(n);
  w.hist = c.take<uint32_t>(256 * numTiles);
  w.totals = c.take<uint32_t>(256);
  w.partials = c.take<float>((size_t)kBoundsGroups * 2 * rk::kCoords);
  w.bounds = c.take<float>(64);
  w.orAnd = mem ? reinterpret_cast<unsigned long long *>(w.bounds + 16) : nullptr;
  w.bytes = c.bytes();
  return w;
}
static bool aligned(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace rm

using namespace rm;

extern "C" int rm_rays_order(const RmRay *d_rays, int numRays, int originBits, int dirBits, int32_t *d_order, RmRay *d_sorted, uint64_t *d_keys,
                             void *stream) {
  auto bad = [](const char *msg) { set_error(msg); return (int)RM_ERR_INVALID_ARGUMENT; };
  if (numRays < 0) return bad("negative numRays");
  if (originBits < 0 || originBits > rk::kMaxOriginBits || dirBits < 0 || dirBits > rk::kMaxDirBits)
    return bad("originBits must be 0 … 10 and dirBits 0 … 11");
  if (numRays == 0) return RM_OK;
  if (!d_rays || !d_order) return bad("null d_rays or d_order");
  if (!aligned(d_rays, 16) || !aligned(d_sorted, 16) || !aligned(d_keys, 8) || !aligned(d_order, 4))
    return bad("misaligned d_rays or d_sorted (16 bytes), d_keys (8 bytes) or d_order (4 bytes)");
  if (d_sorted == d_rays) return bad("d_sorted must not be d_rays");
  if (int st = require_device_pointers({{"d_rays", d_rays}, {"d_order", d_order}, {"d_sorted", d_sorted}, {"d_keys", d_keys}})) return st;
  const hipStream_t hs = static_cast<hipStream_t>(stream);
  const size_t n = (size_t)numRays, numTiles = (n + kSortTile - 1) / kSortTile;
  const size_t groups = (n + 255) / 256;
  const unsigned boundsGroups = (unsigned)(groups < (size_t)kBoundsGroups ? groups : (size_t)kBoundsGroups);
  const unsigned keyGroups = (unsigned)(groups < (size_t)kKeyGroups ? groups : (size_t)kKeyGroups);
  // the workspace is in use until the last launch is enqueued: the device's launcher lock keeps rm_release_workspaces away
  std::unique_lock<std::mutex> lock;
  if (int st = lock_current_device(lock)) return st;
  void *mem = nullptr;
  if (int st = stream_workspace(kWsRayOrder, hs, order_workspace(n, numTiles, nullptr).bytes, &mem)) return st;
  const OrderWs ws = order_workspace(n, numTiles, mem);
  const float4 *rays = reinterpret_cast<const float4 *>(d_rays);

  hipLaunchKernelGGL(order_bounds_kernel, dim3(boundsGroups), dim3(256), 0, hs, rays, (unsigned)n, ws.partials);
  hipLaunchKernelGGL(order_bounds_final_kernel, dim3(1), dim3(256), 0, hs, ws.partials, boundsGroups, ws.bounds, ws.orAnd);
  hipLaunchKernelGGL(order_keys_kernel, dim3(keyGroups), dim3(256), 0, hs, rays, (unsigned)n, originBits, dirBits, ws.bounds, ws.sb.keys[0], ws.sb.idx[0],
                     reinterpret_cast<unsigned long long *>(d_keys), ws.orAnd);
  const int numPasses = (rk::key_bits(originBits, dirBits) + 7) / 8;  // at most 7
  for (int pass = 0; pass < numPasses; pass++) {
    hipLaunchKernelGGL(order_hist_kernel, dim3((unsigned)numTiles), dim3(kSortLanes), 0, hs, ws.sb, (unsigned)n, pass, ws.orAnd, ws.hist);
    hipLaunchKernelGGL(order_scan_kernel, dim3(256), dim3(1024), 0, hs, ws.hist, (unsigned)numTiles, pass, ws.orAnd, ws.totals);
    hipLaunchKernelGGL(order_scatter_kernel, dim3((unsigned)numTiles), dim3(kSortLanes), 0, hs, ws.sb, (unsigned)n, pass, ws.orAnd, ws.hist, ws.totals);
  }
  hipLaunchKernelGGL(order_emit_kernel, dim3((unsigned)((2 * n + 255) / 256)), dim3(256), 0, hs, ws.sb, (unsigned)n, numPasses, ws.orAnd, rays, d_order,
                     reinterpret_cast<float4 *>(d_sorted));
  HIP_OK(hipGetLastError());
  return RM_OK;
}

extern "C" int rm_rays_restore(const void *d_rows, const int32_t *d_order, int numRows, int rowBytes, void *d_out, void *stream) {
  auto bad = [](const char *msg) { set_error(msg); return (int)RM_ERR_INVALID_ARGUMENT; };
  if (numRows < 0) return bad("negative numRows");
  if (rowBytes != 16 && rowBytes != 32) return bad("rowBytes must be 16 or 32");
  if (numRows == 0) return RM_OK;
  if (!d_rows || !d_order || !d_out) return bad("null d_rows, d_order or d_out");
  if (!aligned(d_rows, 16) || !aligned(d_out, 16) || !aligned(d_order, 4)) return bad("misaligned d_rows or d_out (16 bytes) or d_order (4 bytes)");
  if (d_out == d_rows) return bad("d_out must not be d_rows");
  if (int st = require_device_pointers({{"d_rows", d_rows}, {"d_order", d_order}, {"d_out", d_out}})) return st;
  const unsigned parts = (unsigned)rowBytes / 16u;
  const size_t lanes = (size_t)numRows * parts;
  hipLaunchKernelGGL(order_restore_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<const uint4 *>(d_rows), d_order, (unsigned)numRows, parts, reinterpret_cast<uint4 *>(d_out));
  HIP_OK(hipGetLastError());
  return RM_OK;
}
