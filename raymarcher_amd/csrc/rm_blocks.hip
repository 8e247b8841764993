// rm_blocks.hip — block-sparse lattices (gfx950 only): the kernels of rm_sdf_blocks_select (which 8×8×8-cell blocks of a virtual
// lattice hold surface), of rm_sdf_blocks_select_pruned (the same list without the sweep over every block), of rm_sdf_grid_blocks
// (sdScene on the 9×9×9 points of listed blocks only) and the kernels and the entry point of rm_sdf_mesh_blocks (rm_sdf_mesh's quad
// mesh over a block list).  include/raymarcher_amd.h has the definitions.  The argument checks and staging of the first three are
// launch_sdf_blocks_select / launch_sdf_grid_blocks in rm_queries.hip; everything of rm_sdf_mesh_blocks is here, as rm_sdf_mesh is
// in rm_volume.hip.  rm_lattice.h declares what other units call, rm_compact.hip.h has the scan, rm_blocks_prune.h the pruning rule.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "rm_blocks_prune.h"
#include "rm_compact.hip.h"
#include "rm_device.hip.h"
#include "rm_lattice.h"
#include "rm_surface_nets_blocks.h"

namespace rm {

// ---- the evaluation of a block's 729 points (rm_sdf_blocks_select, rm_sdf_grid_blocks) ------------------------------------------
// One workgroup per block, one lane per lattice point of it.  How the 729 points map onto waves (RM_BLOCKS_MAP):
//   0: runs of 64 in the block's own linear order (c·9 + b)·9 + a, x fastest: twelve waves, the last with 25 live lanes (95 % of
//      the lanes live); a wave covers seven rows of 9 and a bit, in at most two z-slabs: stores of rm_sdf_grid_blocks are 256 B runs
//   1: compact sub-boxes of 9×3×2 points, 54 live lanes of 64: fifteen waves (five z-pairs, the last one slab thick, times three
//      y-triples; 76 % live), whose lanes are closer in space
// profiles/sdf_blocks.md has the measurement.  A lane outside the 729 points is masked off before the evaluation, as the lanes of
// sdf_grid_kernel past the lattice are: the evaluator's ballots are proofs about the lanes that are live, so a point's value does
// not depend on which other points share its wave, and is rm_sdf_grid's for that lattice point — the same instantiation
// sdSceneImpl<BULB, 0, kTrapNone> on the same point origin + (float)i · step.
#ifndef RM_BLOCKS_MAP
#define RM_BLOCKS_MAP 0
#endif
static_assert(RM_BLOCKS_MAP == 0 || RM_BLOCKS_MAP == 1, "RM_BLOCKS_MAP: 0 = runs of 64 in x-fastest order, 1 = 9×3×2 sub-boxes");
constexpr int kEvalWaves = RM_BLOCKS_MAP ? 15 : 12;

// the lattice as the evaluation kernels take it
struct BlockLattice { float ox, oy, oz, sx, sy, sz; int mx, my, mz; };
static BlockLattice block_lattice(const float origin[3], const float step[3], int mx, int my, int mz) {
  return BlockLattice{origin[0], origin[1], origin[2], step[0], step[1], step[2], mx, my, mz};
}

// the block-local point index of a lane, −1 for a lane with no point
RM_DEV int eval_point_of(unsigned wave, unsigned lane) {
  if (RM_BLOCKS_MAP == 0) {
    const unsigned t = wave * 64u + lane;
    return t < (unsigned)snb::kBlockPoints ? (int)t : -1;
  }
  if (lane >= 54u) return -1;
  const unsigned a = lane % 9u, b = (wave % 3u) * 3u + (lane / 9u) % 3u, c = (wave / 3u) * 2u + lane / 27u;
  return c <= 8u ? snb::point_index((int)a, (int)b, (int)c) : -1;
}

// Point t of block (bi, bj, bk): rm_sdf_grid's point origin + (float)i · step.  The kernels call the evaluator on it themselves, as
// sdf_grid_kernel does: with the call inside this function the compiler schedules the evaluator's body differently
// (profiles/lattice_units.md).
RM_DEV V3 block_point(const BlockLattice &L, int bi, int bj, int bk, int t) {
  const int a = t % 9, b = (t / 9) % 9, c = t / 81;
  const float fx = (float)(8 * bi + a) * L.sx, fy = (float)(8 * bj + b) * L.sy, fz = (float)(8 * bk + c) * L.sz;
  return v3(L.ox + fx, L.oy + fy, L.oz + fz);
}
// The workgroup's vote, every lane in it: the block is ACTIVE iff one of its points is inside and one is outside (a lane with no
// point has neither).  `seen` is the kernel's LDS word — bit 0: a point is inside, bit 1: one is outside.  The lane that resets it
// is the one that reads it, behind a barrier each, so a kernel may vote again at once.  The result is thread 0's; false elsewhere.
RM_DEV bool block_active(unsigned *seen, bool in, bool out) {
  if (threadIdx.x == 0) *seen = 0u;
  __syncthreads();
  const unsigned bits = (__ballot(in) != 0ull ? 1u : 0u) | (__ballot(out) != 0ull ? 2u : 0u);  // wave-uniform
  if ((threadIdx.x & 63u) == 0u) atomicOr(seen, bits);
  __syncthreads();
  return threadIdx.x == 0 && *seen == 3u;
}

// SELECT: the grid is the virtual lattice's blocks, flags[(bk·my + bj)·mx + bi] = 1 iff the block is active.
// otherwise: the grid is the list, entry n's values go to dist[n·729 …] (and ids); a void entry's workgroup leaves at once.
template <int BULB, bool SELECT>
__global__ __launch_bounds__(64 * kEvalWaves) void blocks_eval_kernel(const SceneBlock *__restrict__ sb, BlockLattice L, float iso,
                                                                      const int32_t *__restrict__ list, const uint32_t *__restrict__ first,
                                                                      uint32_t *__restrict__ flags, float *__restrict__ dist,
                                                                      int32_t *__restrict__ ids) {
  __shared__ unsigned seen;
  int bi, bj, bk;
  if (SELECT) {
    bi = (int)blockIdx.x, bj = (int)blockIdx.y, bk = (int)blockIdx.z;
  } else {
    bi = list[4 * (size_t)blockIdx.x], bj = list[4 * (size_t)blockIdx.x + 1], bk = list[4 * (size_t)blockIdx.x + 2];
    if (!snb::entry_listed(snb::Blocks{first, L.mx, L.my, L.mz}, bi, bj, bk, blockIdx.x)) return;  // the same for the whole workgroup
  }
  const int t = eval_point_of(threadIdx.x >> 6, threadIdx.x & 63u);
  bool in = false;
  if (t >= 0) {
    Counters cnt{0, 0, 0, 0, 0, 0};
    float unused;
    const SceneMin m = sdSceneImpl<BULB, 0, kTrapNone>(sb, block_point(L, bi, bj, bk, t), cnt, __builtin_inff(), unused);
    if (SELECT) {
      in = sn::inside(m.d, iso);
    } else {
      const size_t at = (size_t)blockIdx.x * (size_t)snb::kBlockPoints + (size_t)t;
      dist[at] = m.d;
      if (ids) ids[at] = m.idx;
    }
  }
  if (SELECT) {
    const bool active = block_active(&seen, in, t >= 0 && !in);
    if (threadIdx.x == 0) flags[((size_t)bk * (size_t)L.my + (size_t)bj) * (size_t)L.mx + (size_t)bi] = active ? 1u : 0u;
  }
}

// ---- the compaction's scan -----------------------------------------------------------------------------------------------------
// Workgroup q turns the n counts off[q·n …] into exclusive offsets in place, carrying the total from one round of 1024 to the next,
// and stores the total in totals[q] and, saturated at 2^32 − 1, in counts[q].
__global__ __launch_bounds__(1024) void blocks_scan_kernel(unsigned long long *__restrict__ off, unsigned n, unsigned long long *__restrict__ totals,
                                                           uint32_t *__restrict__ counts) {
  __shared__ unsigned long long waveSum[16];
  unsigned long long *mine = off + (size_t)blockIdx.x * (size_t)n;
  unsigned long long carry = 0;  // the same in every lane
  for (unsigned base = 0; base < n; base += 1024u) {
    const unsigned i = base + threadIdx.x;
    const ScanRound<unsigned long long> r = scan_round_1024(i < n ? mine[i] : 0ull, waveSum);
    if (i < n) mine[i] = carry + r.before;
    carry += r.all;
  }
  if (threadIdx.x == 0) {
    totals[blockIdx.x] = carry;
    counts[blockIdx.x] = carry > 0xffffffffull ? 0xffffffffu : (uint32_t)carry;
  }
}

// ---- the compaction of one flag per block ----------------------------------------------------------------------------------------
// The flags in the blocks' linear order are dealt to workgroups of ONE wave, kShare = 1024 consecutive flags each (16 rounds of 64):
// select_count_kernel counts a share into off[share], blocks_scan_kernel turns the counts into exclusive offsets, and a third kernel
// numbers the set flags behind its share's offset (number_set_flags: ballot + popcount) and stores what it has to say of each.
constexpr int kShareRounds = 16, kShare = 64 * kShareRounds;
static size_t flag_shares(size_t numFlags) { return (numFlags + kShare - 1) / kShare; }

__global__ __launch_bounds__(64) void select_count_kernel(const uint32_t *__restrict__ flags, size_t numFlags, unsigned long long *__restrict__ off) {
  unsigned count = 0;  // wave-uniform
  for (int r = 0; r < kShareRounds; r++) {
    const size_t q = ((size_t)blockIdx.x * kShareRounds + r) * 64u + threadIdx.x;
    count += (unsigned)__popcll(__ballot(q < numFlags && flags[q] != 0u));
  }
  if (threadIdx.x == 0) off[blockIdx.x] = count;
}
// store(q, number) for every set flag q of the workgroup's share, `number` its place among all set flags
template <class Store>
RM_DEV void number_set_flags(const uint32_t *__restrict__ flags, size_t numFlags, const unsigned long long *__restrict__ off, Store store) {
  unsigned long long base = off[blockIdx.x];  // wave-uniform
  for (int r = 0; r < kShareRounds; r++) {
    const size_t q = ((size_t)blockIdx.x * kShareRounds + r) * 64u + threadIdx.x;
    const bool set = q < numFlags && flags[q] != 0u;
    const unsigned long long ballot = __ballot(set);
    if (set) store(q, base + lanes_below(ballot, threadIdx.x));
    base += (unsigned long long)__popcll(ballot);
  }
}
// the rows (bi, bj, bk, 0) of the set flags numbered below maxBlocks
__global__ __launch_bounds__(64) void select_emit_kernel(const uint32_t *__restrict__ flags, size_t numFlags, int mx, int my,
                                                         const unsigned long long *__restrict__ off, int maxBlocks, int32_t *__restrict__ list) {
  number_set_flags(flags, numFlags, off, [=](size_t q, unsigned long long number) {
    if (number >= (unsigned long long)maxBlocks) return;
    const size_t row = q / (size_t)mx;
    int32_t *o = list + 4 * (size_t)number;
    o[0] = (int32_t)(q % (size_t)mx);
    o[1] = (int32_t)(row % (size_t)my);
    o[2] = (int32_t)(row / (size_t)my);
    o[3] = 0;
  });
}
// counts, scans, and stores the total in off[shares] and, saturated at 2^32 − 1, in *d_count
static void enqueue_flags_count(const uint32_t *flags, size_t numFlags, unsigned long long *off, uint32_t *d_count, hipStream_t stream) {
  const size_t shares = flag_shares(numFlags);
  hipLaunchKernelGGL(select_count_kernel, dim3((unsigned)shares), dim3(64), 0, stream, flags, numFlags, off);
  hipLaunchKernelGGL(blocks_scan_kernel, dim3(1), dim3(1024), 0, stream, off, (unsigned)shares, off + shares, d_count);
}
static void enqueue_flags_emit(const uint32_t *flags, size_t numFlags, int mx, int my, const unsigned long long *off, int maxBlocks, int32_t *d_blocks,
                               hipStream_t stream) {
  hipLaunchKernelGGL(select_emit_kernel, dim3((unsigned)flag_shares(numFlags)), dim3(64), 0, stream, flags, numFlags, mx, my, off, maxBlocks,
                     d_blocks);
}

// ---- the block map ----------------------------------------------------------------------------------------------------------------
// first[block] = the smallest list position that names the block: filled with kNoEntry (all bits set), then a scatter with atomicMin.
__global__ __launch_bounds__(256) void blocks_map_kernel(const int32_t *__restrict__ list, unsigned numBlocks, int mx, int my, int mz,
                                                         uint32_t *__restrict__ first) {
  const unsigned n = blockIdx.x * 256u + threadIdx.x;
  if (n >= numBlocks) return;
  const int bi = list[4 * (size_t)n], bj = list[4 * (size_t)n + 1], bk = list[4 * (size_t)n + 2];
  const snb::Blocks B{first, mx, my, mz};
  if (snb::in_range(B, bi, bj, bk)) atomicMin(&first[snb::block_linear(B, bi, bj, bk)], n);
}
int enqueue_block_map(const int32_t *d_blocks, int numBlocks, int mx, int my, int mz, uint32_t *first, hipStream_t stream) {
  HIP_OK(hipMemsetAsync(first, 0xff, (size_t)mx * (size_t)my * (size_t)mz * sizeof(uint32_t), stream));
  if (numBlocks == 0) return RM_OK;  // an empty list: no block is listed
  hipLaunchKernelGGL(blocks_map_kernel, dim3(((unsigned)numBlocks + 255u) / 256u), dim3(256), 0, stream, d_blocks, (unsigned)numBlocks, mx, my,
                     mz, first);
  return RM_OK;
}

// ---- rm_sdf_blocks_select_pruned ------------------------------------------------------------------------------------------------
// The corners of the blocks are evaluated once; a block whose eight corners are all far from the iso surface on the same side is
// discarded (rm_blocks_prune.h has the rule), and only the others — the candidates — get the exact evaluation of their 729 points.
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
// the candidates' list: the block's linear index, and every candidate has a place — the list holds as many words as the lattice
// has blocks
__global__ __launch_bounds__(64) void prune_candidates_kernel(const uint32_t *__restrict__ flags, size_t numFlags,
                                                              const unsigned long long *__restrict__ off, uint32_t *__restrict__ list) {
  number_set_flags(flags, numFlags, off, [=](size_t q, unsigned long long number) { list[number] = (uint32_t)q; });
}

// ---- 3. the exact evaluation of the candidates ----------------------------------------------------------------------------------
// blocks_eval_kernel's workgroup, lane → point mapping, evaluation and vote on a loop over the candidate list.  The list's length is
// read from device memory — the host never waits for it — and the grid is sized from the device, not from the length.  The
// candidate's flag becomes the block's ACTIVE flag.
template <int BULB>
__global__ __launch_bounds__(64 * kEvalWaves) void prune_eval_kernel(const SceneBlock *__restrict__ sb, BlockLattice L, float iso,
                                                                     const uint32_t *__restrict__ list,
                                                                     const unsigned long long *__restrict__ count,
                                                                     uint32_t *__restrict__ flags) {
  __shared__ unsigned seen;
  const unsigned long long total = *count;
  const int t = eval_point_of(threadIdx.x >> 6, threadIdx.x & 63u);
  for (unsigned long long n = blockIdx.x; n < total; n += gridDim.x) {  // the same trips for the whole workgroup
    const uint32_t q = list[n];
    const uint32_t row = q / (uint32_t)L.mx;
    const int bi = (int)(q % (uint32_t)L.mx), bj = (int)(row % (uint32_t)L.my), bk = (int)(row / (uint32_t)L.my);
    bool in = false;
    if (t >= 0) {
      Counters cnt{0, 0, 0, 0, 0, 0};
      float unused;
      in = sn::inside(sdSceneImpl<BULB, 0, kTrapNone>(sb, block_point(L, bi, bj, bk, t), cnt, __builtin_inff(), unused).d, iso);
    }
    const bool active = block_active(&seen, in, t >= 0 && !in);
    if (threadIdx.x == 0) flags[q] = active ? 1u : 0u;
  }
}

// ---- the launches of the three staged entry points (rm_queries.hip checks and stages) --------------------------------------------
// Each workspace is laid out once: with mem = nullptr the same lines measure it.
template <bool SELECT, class... Args>
static void launch_eval(int bulbClass, dim3 grid, hipStream_t stream, Args... args) {
  const dim3 block(64 * kEvalWaves);
  dispatch_march_class(bulbClass, [&](auto c) {
    hipLaunchKernelGGL((blocks_eval_kernel<decltype(c)::bulb, SELECT>), grid, block, 0, stream, args...);
  });
}
static size_t block_count(int mx, int my, int mz) { return (size_t)mx * (size_t)my * (size_t)mz; }
static size_t corner_count(int mx, int my, int mz) { return (size_t)(mx + 1) * (size_t)(my + 1) * (size_t)(mz + 1); }

// a flag per block and the scan's words: a count per share, then the total
struct SelectWs { uint32_t *flags; unsigned long long *off; size_t bytes; };
static SelectWs select_workspace(int mx, int my, int mz, void *mem) {
  Carve c(mem);  // a braced list is evaluated left to right: the members' order is the layout
  return SelectWs{c.take<uint32_t>(block_count(mx, my, mz)), c.take<unsigned long long>(flag_shares(block_count(mx, my, mz)) + 1), c.bytes()};
}
size_t blocks_select_workspace(int mx, int my, int mz) { return select_workspace(mx, my, mz, nullptr).bytes; }
int launch_blocks_select_kernels(const void *sbv, int bulbClass, const float origin[3], const float step[3], int mx, int my, int mz, float iso,
                                 int maxBlocks, int32_t *d_blocks, uint32_t *d_count, void *workspace, hipStream_t stream) {
  const size_t blocks = block_count(mx, my, mz);
  const SelectWs ws = select_workspace(mx, my, mz, workspace);
  // at most 512 blocks along every axis: every grid dimension is far below its limit of 65535
  launch_eval<true>(bulbClass, dim3((unsigned)mx, (unsigned)my, (unsigned)mz), stream, static_cast<const SceneBlock *>(sbv),
                    block_lattice(origin, step, mx, my, mz), iso, (const int32_t *)nullptr, (const uint32_t *)nullptr, ws.flags, (float *)nullptr,
                    (int32_t *)nullptr);
  enqueue_flags_count(ws.flags, blocks, ws.off, d_count, stream);
  if (maxBlocks > 0) enqueue_flags_emit(ws.flags, blocks, mx, my, ws.off, maxBlocks, d_blocks, stream);
  HIP_OK(hipGetLastError());
  return RM_OK;
}

// the corner lattice, a flag per block, the candidate list, the scan's words
struct PruneWs { float *corners; uint32_t *flags, *list; unsigned long long *off; size_t bytes; };
static PruneWs prune_workspace(int mx, int my, int mz, void *mem) {
  Carve c(mem);
  const size_t blocks = block_count(mx, my, mz);
  return PruneWs{c.take<float>(corner_count(mx, my, mz)), c.take<uint32_t>(blocks), c.take<uint32_t>(blocks),
                 c.take<unsigned long long>(flag_shares(blocks) + 1), c.bytes()};
}
size_t blocks_prune_workspace(int mx, int my, int mz) { return prune_workspace(mx, my, mz, nullptr).bytes; }
int launch_blocks_prune_kernels(const void *sbv, int bulbClass, const float origin[3], const float step[3], int mx, int my, int mz, float iso,
                                float lipschitzOut, float lipschitzIn, int maxBlocks, int32_t *d_blocks, uint32_t *d_count, void *workspace,
                                hipStream_t stream) {
  const SceneBlock *sb = static_cast<const SceneBlock *>(sbv);
  const size_t blocks = block_count(mx, my, mz), numCorners = corner_count(mx, my, mz), shares = flag_shares(blocks);
  const PruneWs ws = prune_workspace(mx, my, mz, workspace);
  int dev = 0, numCUs = 0;
  HIP_OK(hipGetDevice(&dev));
  HIP_OK(hipDeviceGetAttribute(&numCUs, hipDeviceAttributeMultiprocessorCount, dev));
  const BlockLattice L = block_lattice(origin, step, mx, my, mz);
  const prune::Bounds bounds = prune::bounds(step, lipschitzOut, lipschitzIn);
  // at most 513³ corners and 512³ blocks: 2^20 workgroups of 256 at the most, far below the limit of grid.x
  const dim3 cornerGrid((unsigned)((numCorners + 255) / 256)), blockGrid((unsigned)((blocks + 255) / 256));
  // the candidates' workgroups: a few per CU, so that a slow block holds up few others, and never more than there are blocks
  const size_t evalGroups = (size_t)(numCUs > 0 ? numCUs : 256) * 4;
  const dim3 evalGrid((unsigned)(blocks < evalGroups ? blocks : evalGroups)), evalBlock(64 * kEvalWaves);
  dispatch_march_class(bulbClass, [&](auto c) {
    constexpr int BULB = decltype(c)::bulb;
    hipLaunchKernelGGL(prune_corners_kernel<BULB>, cornerGrid, dim3(256), 0, stream, sb, L, numCorners, ws.corners);
    hipLaunchKernelGGL(prune_classify_kernel, blockGrid, dim3(256), 0, stream, (const float *)ws.corners, mx, my, blocks, iso, bounds, ws.flags);
    enqueue_flags_count(ws.flags, blocks, ws.off, d_count + 1, stream);  // the candidates' number: off[shares] and d_count[1]
    hipLaunchKernelGGL(prune_candidates_kernel, dim3((unsigned)shares), dim3(64), 0, stream, (const uint32_t *)ws.flags, blocks,
                       (const unsigned long long *)ws.off, ws.list);
    hipLaunchKernelGGL(prune_eval_kernel<BULB>, evalGrid, evalBlock, 0, stream, sb, L, iso, (const uint32_t *)ws.list,
                       (const unsigned long long *)(ws.off + shares), ws.flags);
  });
  // the flags are the active flags now (a discarded block's is still 0): rm_sdf_blocks_select's compaction
  enqueue_flags_count(ws.flags, blocks, ws.off, d_count, stream);
  if (maxBlocks > 0) enqueue_flags_emit(ws.flags, blocks, mx, my, ws.off, maxBlocks, d_blocks, stream);
  HIP_OK(hipGetLastError());
  return RM_OK;
}

// the block map's layout is rm_lattice.h's take_block_map
int launch_blocks_grid_kernels(const void *sbv, int bulbClass, const float origin[3], const float step[3], int mx, int my, int mz,
                               const int32_t *d_blocks, int numBlocks, float *d_dist, int32_t *d_objectId, void *workspace, hipStream_t stream) {
  Carve c(workspace);
  uint32_t *first = take_block_map(c, mx, my, mz);
  if (int st = enqueue_block_map(d_blocks, numBlocks, mx, my, mz, first, stream)) return st;
  launch_eval<false>(bulbClass, dim3((unsigned)numBlocks), stream, static_cast<const SceneBlock *>(sbv), block_lattice(origin, step, mx, my, mz),
                     0.0f, d_blocks, (const uint32_t *)first, (uint32_t *)nullptr, d_dist, d_objectId);
  HIP_OK(hipGetLastError());
  return RM_OK;
}

// ---- rm_sdf_mesh_blocks ---------------------------------------------------------------------------------------------------------
// One workgroup of 512 lanes per list entry, lane = local cell (c·8 + b)·8 + a: wave w is the z-slab c = w.  The entry's 729 values
// are staged in LDS; a void entry's workgroup stores zeros (count) or leaves (emit).  A lane stands for its cell and for the three
// lattice edges that start at the cell's corner 0, the edges its block owns — so the order of the lanes is the definition's order
// of vertices and of quads within an entry.
//   1. blocks_map_kernel: the block map
//   2. mesh_blocks_count_kernel: per entry the active cells, the stored quads and the open vertices → off[0 … 2][entry], and the
//      512-bit mask of active cells → masks[entry]
//   3. blocks_scan_kernel, three workgroups: exclusive offsets over the entries, the totals → d_counts
//   4. mesh_blocks_emit_kernel: classifies again; the vertex of an active cell is numbered base + (active cells of the block below
//      it), the four vertices of a quad likewise through the block map, from the bases and masks of the (up to four) blocks around
//      the edge — 68 B per entry stand in for rm_sdf_mesh's 4 B per cell.
// Step 4 is left out of a counting call.  Workspace (kWsBlocks, per device and stream, grow-only): 4 B per block of the virtual
// lattice, 24 B + 64 B per list entry.
struct BlockCell { float v[8]; unsigned mask; bool active; int state[3]; };
RM_DEV BlockCell classify_block_cell(const float *vals, float iso, const snb::Blocks &B, const snb::Self &s, int a, int b, int c) {
  BlockCell cc;
  snb::cell_corners(vals, a, b, c, cc.v);
  cc.mask = sn::corner_mask(cc.v, iso);
  cc.active = sn::cell_active(cc.mask);
#pragma unroll
  for (int axis = 0; axis < 3; axis++) cc.state[axis] = snb::owned_edge_state(B, s, cc.mask, axis, a, b, c);
  return cc;
}
// stages entry n's values; false (for the whole workgroup) where the entry is void
RM_DEV bool stage_entry(const float *__restrict__ dist, const int32_t *__restrict__ list, const snb::Blocks &B, float *vals, snb::Self *s) {
  const uint32_t n = blockIdx.x;
  *s = snb::Self{list[4 * (size_t)n], list[4 * (size_t)n + 1], list[4 * (size_t)n + 2], n};
  if (!snb::entry_listed(B, s->bi, s->bj, s->bk, n)) return false;
  for (unsigned t = threadIdx.x; t < (unsigned)snb::kBlockPoints; t += 512u) vals[t] = dist[(size_t)n * snb::kBlockPoints + t];
  __syncthreads();
  return true;
}

__global__ __launch_bounds__(512) void mesh_blocks_count_kernel(const float *__restrict__ dist, const int32_t *__restrict__ list, unsigned numBlocks,
                                                                snb::Blocks B, float iso, unsigned long long *__restrict__ off,
                                                                uint32_t *__restrict__ masks) {
  __shared__ float vals[snb::kBlockPoints];
  __shared__ unsigned waveCount[3][8];
  const unsigned n = blockIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  snb::Self s;
  if (!stage_entry(dist, list, B, vals, &s)) {
    if (threadIdx.x < 3u) off[(size_t)threadIdx.x * numBlocks + n] = 0ull;
    if (threadIdx.x < (unsigned)snb::kMaskWords) masks[(size_t)n * snb::kMaskWords + threadIdx.x] = 0u;
    return;
  }
  const int a = (int)(threadIdx.x & 7u), b = (int)((threadIdx.x >> 3) & 7u), c = (int)(threadIdx.x >> 6);
  const BlockCell cc = classify_block_cell(vals, iso, B, s, a, b, c);
  const bool open = cc.active && snb::cell_open(B, s, cc.mask, a, b, c);
  const unsigned long long act = __ballot(cc.active);
  const unsigned nq = (unsigned)(__popcll(__ballot(cc.state[0] == snb::kEdgeQuad)) + __popcll(__ballot(cc.state[1] == snb::kEdgeQuad)) +
                                 __popcll(__ballot(cc.state[2] == snb::kEdgeQuad)));
  const unsigned no = (unsigned)__popcll(__ballot(open));
  if (lane == 0u) {
    waveCount[0][wave] = (unsigned)__popcll(act);
    waveCount[1][wave] = nq;
    waveCount[2][wave] = no;
    masks[(size_t)n * snb::kMaskWords + 2u * wave] = (uint32_t)act;
    masks[(size_t)n * snb::kMaskWords + 2u * wave + 1u] = (uint32_t)(act >> 32);
  }
  __syncthreads();
  if (threadIdx.x < 3u) {
    unsigned long long sum = 0;
    for (int w = 0; w < 8; w++) sum += waveCount[threadIdx.x][w];
    off[(size_t)threadIdx.x * numBlocks + n] = sum;
  }
}

__global__ __launch_bounds__(512) void mesh_blocks_emit_kernel(const float *__restrict__ dist, const int32_t *__restrict__ objectId,
                                                               const int32_t *__restrict__ list, unsigned numBlocks, snb::Blocks B, float iso,
                                                               BlockLattice L, const unsigned long long *__restrict__ off,
                                                               const unsigned long long *__restrict__ totals, const uint32_t *__restrict__ masks,
                                                               int maxVertices, int maxQuads, float *__restrict__ vertices,
                                                               int32_t *__restrict__ vertexObject, int32_t *__restrict__ quads) {
  __shared__ float vals[snb::kBlockPoints];
  __shared__ unsigned waveCount[2][8];
  const unsigned n = blockIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  snb::Self s;
  if (!stage_entry(dist, list, B, vals, &s)) return;
  const int a = (int)(threadIdx.x & 7u), b = (int)((threadIdx.x >> 3) & 7u), c = (int)(threadIdx.x >> 6);
  const BlockCell cc = classify_block_cell(vals, iso, B, s, a, b, c);
  const unsigned long long act = __ballot(cc.active), q0 = __ballot(cc.state[0] == snb::kEdgeQuad), q1 = __ballot(cc.state[1] == snb::kEdgeQuad),
                           q2 = __ballot(cc.state[2] == snb::kEdgeQuad);
  if (lane == 0u) {
    waveCount[0][wave] = (unsigned)__popcll(act);
    waveCount[1][wave] = (unsigned)(__popcll(q0) + __popcll(q1) + __popcll(q2));
  }
  __syncthreads();
  unsigned long long vNumber = off[n], qNumber = off[(size_t)numBlocks + n];
  for (unsigned w = 0; w < wave; w++) {
    vNumber += waveCount[0][w];
    qNumber += waveCount[1][w];
  }
  vNumber += lanes_below(act, lane);
  // the quads of the cells before this one in the wave, then this cell's own, in axis order
  qNumber += lanes_below(q0, lane) + lanes_below(q1, lane) + lanes_below(q2, lane);
  if (cc.active && vNumber < (unsigned long long)maxVertices) {
    float local[3];
    sn::cell_vertex(cc.v, iso, cc.mask, local);
    float *o = vertices + 4 * (size_t)vNumber;  // four words: the ABI asks no alignment of d_vertices beyond a float's
    o[0] = sn::vertex_world(L.ox, L.sx, 8 * s.bi + a, local[0]);
    o[1] = sn::vertex_world(L.oy, L.sy, 8 * s.bj + b, local[1]);
    o[2] = sn::vertex_world(L.oz, L.sz, 8 * s.bk + c, local[2]);
    o[3] = 0.0f;
    if (vertexObject) {
      int32_t id = -1;
      if (objectId) {
        const int k = sn::first_inside_corner(cc.mask);
        id = objectId[(size_t)n * snb::kBlockPoints + (size_t)snb::point_index(a + (k & 1), b + ((k >> 1) & 1), c + ((k >> 2) & 1))];
      }
      vertexObject[vNumber] = id;
    }
  }
  if (maxQuads == 0) return;
  const unsigned long long total = totals[0];
#pragma unroll
  for (int axis = 0; axis < 3; axis++) {
    if (cc.state[axis] != snb::kEdgeQuad) continue;
    if (qNumber < (unsigned long long)maxQuads) {
      int32_t vtx[4];
      snb::quad_vertices(B, s, off, masks, total, axis, a, b, c, (cc.mask & 1u) != 0u, vtx);
#pragma unroll
      for (int k = 0; k < 4; k++) quads[4 * (size_t)qNumber + k] = vtx[k];
    }
    qNumber++;
  }
}

// the block map; the entries' three counts (vertices, quads, open vertices) and behind them the three totals; the entries' masks
struct MeshBlocksWs { uint32_t *first; unsigned long long *off, *totals; uint32_t *masks; size_t bytes; };
static MeshBlocksWs mesh_blocks_workspace(int mx, int my, int mz, int numBlocks, void *mem) {
  Carve c(mem);
  MeshBlocksWs w;
  w.first = take_block_map(c, mx, my, mz);
  w.off = c.take<unsigned long long>(3 * (size_t)numBlocks + 3);
  w.totals = w.off + 3 * (size_t)numBlocks;
  w.masks = c.take<uint32_t>((size_t)numBlocks * snb::kMaskWords);
  w.bytes = c.bytes();
  return w;
}

}  // namespace rm

using namespace rm;

extern "C" int rm_sdf_mesh_blocks(const float *d_dist, const int32_t *d_objectId, const int32_t *d_blocks, int numBlocks, int mx, int my, int mz,
                                  const float origin[3], const float step[3], float iso, int maxVertices, int maxQuads, float *d_vertices,
                                  int32_t *d_vertexObject, int32_t *d_quads, uint32_t *d_counts, void *stream) {
  auto bad = [](const char *msg) { set_error(msg); return (int)RM_ERR_INVALID_ARGUMENT; };
  if (int st = check_block_lattice(origin, step, mx, my, mz)) return st;
  if (!std::isfinite(iso)) return bad("iso must be finite");
  if (numBlocks < 0 || numBlocks > RM_MAX_BLOCK_LIST) return bad("numBlocks must be 0 … RM_MAX_BLOCK_LIST");
  if (maxVertices < 0 || maxQuads < 0) return bad("negative capacity");
  if ((maxVertices > 0 && !d_vertices) || (maxQuads > 0 && !d_quads)) return bad("null d_vertices or d_quads with a capacity above 0");
  if (!d_counts || (numBlocks > 0 && (!d_dist || !d_blocks))) return bad("null d_dist, d_blocks or d_counts");
  if (int st = require_device_pointers({{"d_dist", d_dist}, {"d_objectId", d_objectId}, {"d_blocks", d_blocks}, {"d_vertices", d_vertices},
                                        {"d_vertexObject", d_vertexObject}, {"d_quads", d_quads}, {"d_counts", d_counts}}))
    return st;
  const hipStream_t hs = static_cast<hipStream_t>(stream);
  if (numBlocks == 0) {  // no entry, so no vertex, no quad and no open vertex
    HIP_OK(hipMemsetAsync(d_counts, 0, 3 * sizeof(uint32_t), hs));
    return RM_OK;
  }
  // the workspace is in use until the last launch is enqueued: the device's launcher lock keeps rm_release_workspaces away
  std::unique_lock<std::mutex> lock;
  if (int st = lock_current_device(lock)) return st;
  void *mem = nullptr;
  if (int st = stream_workspace(kWsBlocks, hs, mesh_blocks_workspace(mx, my, mz, numBlocks, nullptr).bytes, &mem)) return st;
  const MeshBlocksWs ws = mesh_blocks_workspace(mx, my, mz, numBlocks, mem);
  if (int st = enqueue_block_map(d_blocks, numBlocks, mx, my, mz, ws.first, hs)) return st;
  const snb::Blocks B{ws.first, mx, my, mz};
  hipLaunchKernelGGL(mesh_blocks_count_kernel, dim3((unsigned)numBlocks), dim3(512), 0, hs, d_dist, d_blocks, (unsigned)numBlocks, B, iso, ws.off, ws.masks);
  hipLaunchKernelGGL(blocks_scan_kernel, dim3(3), dim3(1024), 0, hs, ws.off, (unsigned)numBlocks, ws.totals, d_counts);
  if (maxVertices > 0 || maxQuads > 0) {
    hipLaunchKernelGGL(mesh_blocks_emit_kernel, dim3((unsigned)numBlocks), dim3(512), 0, hs, d_dist, d_objectId, d_blocks, (unsigned)numBlocks, B,
                       iso, block_lattice(origin, step, mx, my, mz), ws.off, ws.totals, ws.masks, maxVertices, maxQuads, d_vertices, d_vertexObject, d_quads);
  }
  HIP_OK(hipGetLastError());
  return RM_OK;
}
