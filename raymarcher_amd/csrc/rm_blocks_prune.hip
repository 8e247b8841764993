// rm_blocks_prune.hip — rm_sdf_blocks_select_pruned (gfx950 only): rm_sdf_blocks_select's list without the sweep over every block.
// The corners of the blocks are evaluated once; a block whose eight corners are all far from the iso surface on the same side is
// discarded (rm_blocks_prune.h has the rule, include/raymarcher_amd.h the definition), and only the others — the candidates — get
// the exact evaluation of their 729 points.  The argument checks and the staging are launch_sdf_blocks_select in
// rm_queries.hip; the count / scan / emit compaction is rm_blocks.hip's.  A translation unit of its own, so that adding it leaves
// the code objects of the existing kernels as they were.
#include <hip/hip_runtime.h>

#include "rm_blocks_prune.h"
#include "rm_device.hip.h"
#include "rm_internal.h"
#include "rm_surface_nets.h"

namespace rm {

// ---- 1. the corner lattice ------------------------------------------------------------------------------------------------------
// One lane per corner, x fastest: corner (i, j, k) is lattice point (8i, 8j, 8k), the point blocks_eval_kernel evaluates as local
// point 0 of block (i, j, k) — the same instantiation of the evaluator on the same origin + (float)(8i) · step.  A lane past the
// last corner leaves before the evaluation, so a corner's value does not depend on its wave.
template <int BULB>
__global__ __launch_bounds__(256) void prune_corners_kernel(const SceneBlock *__restrict__ sb, BlockLattice L, size_t numCorners,
                                                            float *__restrict__ corners) {
  const size_t q = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (q >= numCorners) return;
  const size_t row = q / (size_t)(L.mx + 1);
  const int i = (int)(q % (size_t)(L.mx + 1)), j = (int)(row % (size_t)(L.my + 1)), k = (int)(row / (size_t)(L.my + 1));
  const float fx = (float)(8 * i) * L.sx, fy = (float)(8 * j) * L.sy, fz = (float)(8 * k) * L.sz;
  const V3 p = v3(L.ox + fx, L.oy + fy, L.oz + fz);
  Counters cnt{0, 0, 0, 0, 0, 0};
  float unused;
  corners[q] = sdSceneImpl<BULB, 0, kTrapNone>(sb, p, cnt, __builtin_inff(), unused).d;
}

// ---- 2. the classification ------------------------------------------------------------------------------------------------------
// One lane per block in linear order: flags[q] = 1 for a candidate, 0 for a discarded block.
__global__ __launch_bounds__(256) void prune_classify_kernel(const float *__restrict__ corners, int mx, int my, size_t numBlocks, float iso,
                                                             prune::Bounds bounds, uint32_t *__restrict__ flags) {
  const size_t q = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (q >= numBlocks) return;
  const size_t row = q / (size_t)mx;
  float c[8];
  prune::block_corners(corners, mx, my, (int)(q % (size_t)mx), (int)(row % (size_t)my), (int)(row / (size_t)my), c);
  flags[q] = prune::discarded(c, iso, bounds) ? 0u : 1u;
}
// select_emit_kernel's numbering (rm_blocks.hip) of the set flags behind the share's offset; what is stored is the block's linear
// index, and every candidate has a place: the list holds as many words as the lattice has blocks.
__global__ __launch_bounds__(64) void prune_candidates_kernel(const uint32_t *__restrict__ flags, size_t numFlags,
                                                              const unsigned long long *__restrict__ off, uint32_t *__restrict__ list) {
  unsigned long long base = off[blockIdx.x];  // wave-uniform
  for (int r = 0; r < kShareRounds; r++) {
    const size_t q = ((size_t)blockIdx.x * kShareRounds + r) * 64u + threadIdx.x;
    const bool set = q < numFlags && flags[q] != 0u;
    const unsigned long long ballot = __ballot(set);
    if (set) list[base + (unsigned long long)__popcll(ballot & ((1ull << threadIdx.x) - 1ull))] = (uint32_t)q;
    base += (unsigned long long)__popcll(ballot);
  }
}

// ---- 3. the exact evaluation of the candidates ----------------------------------------------------------------------------------
// blocks_eval_kernel's workgroup (rm_blocks.hip: twelve waves, the 729 points in runs of 64 of the block's x-fastest order, lanes past
// them masked off before the evaluation, the waves' ballots of inside and of !inside ORed) on a loop over the candidate list.  The
// list's length is read from device memory — the host never waits for it — and the grid is sized from the device, not from the
// length.  A trip resets `seen` and synchronises before the first wave may set a bit; the lane that reads `seen` at a trip's end is
// the one that resets it, so no trip sees another's bits.  The candidate's flag becomes the block's ACTIVE flag.
constexpr int kEvalWaves = 12, kBlockPoints = 729;

template <int BULB>
__global__ __launch_bounds__(64 * kEvalWaves) void prune_eval_kernel(const SceneBlock *__restrict__ sb, BlockLattice L, float iso,
                                                                     const uint32_t *__restrict__ list,
                                                                     const unsigned long long *__restrict__ count,
                                                                     uint32_t *__restrict__ flags) {
  __shared__ unsigned seen;  // bit 0: a point of the block is inside, bit 1: one is outside
  const unsigned long long total = *count;
  const bool live = threadIdx.x < (unsigned)kBlockPoints;
  const int a = (int)(threadIdx.x % 9u), b = (int)((threadIdx.x / 9u) % 9u), c = (int)(threadIdx.x / 81u);
  for (unsigned long long n = blockIdx.x; n < total; n += gridDim.x) {  // the same trips for the whole workgroup
    if (threadIdx.x == 0) seen = 0u;
    __syncthreads();
    const uint32_t q = list[n];
    const uint32_t row = q / (uint32_t)L.mx;
    const int bi = (int)(q % (uint32_t)L.mx), bj = (int)(row % (uint32_t)L.my), bk = (int)(row / (uint32_t)L.my);
    bool in = false, out = false;
    if (live) {
      const float fx = (float)(8 * bi + a) * L.sx, fy = (float)(8 * bj + b) * L.sy, fz = (float)(8 * bk + c) * L.sz;
      const V3 p = v3(L.ox + fx, L.oy + fy, L.oz + fz);
      Counters cnt{0, 0, 0, 0, 0, 0};
      float unused;
      const SceneMin m = sdSceneImpl<BULB, 0, kTrapNone>(sb, p, cnt, __builtin_inff(), unused);
      in = sn::inside(m.d, iso);
      out = !in;
    }
    const unsigned bits = (__ballot(in) != 0ull ? 1u : 0u) | (__ballot(out) != 0ull ? 2u : 0u);  // wave-uniform
    if ((threadIdx.x & 63u) == 0u) atomicOr(&seen, bits);
    __syncthreads();
    if (threadIdx.x == 0) flags[q] = seen == 3u ? 1u : 0u;
  }
}

// ---- the launches (rm_queries.hip checks and stages) ---------------------------------------------------------------------------
static size_t align256(size_t v) { return (v + 255) & ~size_t(255); }
static size_t corner_count(int mx, int my, int mz) { return (size_t)(mx + 1) * (size_t)(my + 1) * (size_t)(mz + 1); }

// the corner lattice, a flag per block, the candidate list, the scan's words
size_t blocks_prune_workspace(int mx, int my, int mz) {
  const size_t blocks = (size_t)mx * (size_t)my * (size_t)mz;
  return align256(corner_count(mx, my, mz) * sizeof(float)) + 2 * align256(blocks * sizeof(uint32_t)) +
         align256((flag_shares(blocks) + 1) * sizeof(unsigned long long));
}

int launch_blocks_prune_kernels(const void *sbv, int bulbClass, const float origin[3], const float step[3], int mx, int my, int mz, float iso,
                                float lipschitzOut, float lipschitzIn, int maxBlocks, int32_t *d_blocks, uint32_t *d_count, void *workspace,
                                hipStream_t stream) {
  const SceneBlock *sb = static_cast<const SceneBlock *>(sbv);
  const size_t blocks = (size_t)mx * (size_t)my * (size_t)mz, numCorners = corner_count(mx, my, mz), shares = flag_shares(blocks);
  char *mem = static_cast<char *>(workspace);
  float *corners = reinterpret_cast<float *>(mem);
  uint32_t *flags = reinterpret_cast<uint32_t *>(mem += align256(numCorners * sizeof(float)));
  uint32_t *list = reinterpret_cast<uint32_t *>(mem += align256(blocks * sizeof(uint32_t)));
  unsigned long long *off = reinterpret_cast<unsigned long long *>(mem += align256(blocks * sizeof(uint32_t)));
  int dev = 0, numCUs = 0;
  HIP_OK(hipGetDevice(&dev));
  HIP_OK(hipDeviceGetAttribute(&numCUs, hipDeviceAttributeMultiprocessorCount, dev));
  const BlockLattice L{origin[0], origin[1], origin[2], step[0], step[1], step[2], mx, my, mz};
  const prune::Bounds bounds = prune::bounds(step, lipschitzOut, lipschitzIn);
  // at most 513³ corners and 512³ blocks: 2^20 workgroups of 256 at the most, far below the limit of grid.x
  const dim3 cornerGrid((unsigned)((numCorners + 255) / 256)), blockGrid((unsigned)((blocks + 255) / 256));
  // the candidates' workgroups: a few per CU, so that a slow block holds up few others, and never more than there are blocks
  const size_t evalGroups = (size_t)(numCUs > 0 ? numCUs : 256) * 4;
  const dim3 evalGrid((unsigned)(blocks < evalGroups ? blocks : evalGroups)), evalBlock(64 * kEvalWaves);
  dispatch_march_class(bulbClass, [&](auto c) {
    constexpr int BULB = decltype(c)::bulb;
    hipLaunchKernelGGL(prune_corners_kernel<BULB>, cornerGrid, dim3(256), 0, stream, sb, L, numCorners, corners);
    hipLaunchKernelGGL(prune_classify_kernel, blockGrid, dim3(256), 0, stream, (const float *)corners, mx, my, blocks, iso, bounds, flags);
    enqueue_flags_count(flags, blocks, off, d_count + 1, stream);  // the candidates' number: off[shares] and d_count[1]
    hipLaunchKernelGGL(prune_candidates_kernel, dim3((unsigned)shares), dim3(64), 0, stream, (const uint32_t *)flags, blocks,
                       (const unsigned long long *)off, list);
    hipLaunchKernelGGL(prune_eval_kernel<BULB>, evalGrid, evalBlock, 0, stream, sb, L, iso, (const uint32_t *)list,
                       (const unsigned long long *)(off + shares), flags);
  });
  // the flags are the active flags now (a discarded block's is still 0): rm_sdf_blocks_select's compaction
  enqueue_flags_count(flags, blocks, off, d_count, stream);
  if (maxBlocks > 0) enqueue_flags_emit(flags, blocks, mx, my, off, maxBlocks, d_blocks, stream);
  HIP_OK(hipGetLastError());
  return RM_OK;
}

}  // namespace rm
