// rm_blocks.hip — block-sparse lattices (gfx950 only): the kernels of rm_sdf_blocks_select (which 8×8×8-cell blocks of a virtual
// lattice hold surface), of rm_sdf_grid_blocks (sdScene on the 9×9×9 points of listed blocks only) and the kernels and the entry
// point of rm_sdf_mesh_blocks (rm_sdf_mesh's quad mesh over a block list).  include/raymarcher_amd.h has the definitions.  The
// argument checks and staging of the first two are launch_sdf_blocks_select / launch_sdf_grid_blocks in rm_queries.hip; everything
// of rm_sdf_mesh_blocks is here, as rm_sdf_mesh is in rm_volume.hip.  A translation unit of its own, so that adding it leaves the
// code objects of the existing kernels as they were.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <string>

#include "rm_device.hip.h"
#include "rm_internal.h"
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

// SELECT: the grid is the virtual lattice's blocks, flags[(bk·my + bj)·mx + bi] = 1 iff the block is active.
// otherwise: the grid is the list, entry n's values go to dist[n·729 …] (and ids); a void entry's workgroup leaves at once.
template <int BULB, bool SELECT>
__global__ __launch_bounds__(64 * kEvalWaves) void blocks_eval_kernel(const SceneBlock *__restrict__ sb, BlockLattice L, float iso,
                                                                      const int32_t *__restrict__ list, const uint32_t *__restrict__ first,
                                                                      uint32_t *__restrict__ flags, float *__restrict__ dist,
                                                                      int32_t *__restrict__ ids) {
  __shared__ unsigned seen;  // bit 0: a point of the block is inside, bit 1: one is outside
  int bi, bj, bk;
  if (SELECT) {
    bi = (int)blockIdx.x, bj = (int)blockIdx.y, bk = (int)blockIdx.z;
    if (threadIdx.x == 0) seen = 0u;
    __syncthreads();
  } else {
    bi = list[4 * (size_t)blockIdx.x], bj = list[4 * (size_t)blockIdx.x + 1], bk = list[4 * (size_t)blockIdx.x + 2];
    if (!snb::entry_listed(snb::Blocks{first, L.mx, L.my, L.mz}, bi, bj, bk, blockIdx.x)) return;  // the same for the whole workgroup
  }
  const int t = eval_point_of(threadIdx.x >> 6, threadIdx.x & 63u);
  bool in = false, out = false;
  if (t >= 0) {
    const int a = t % 9, b = (t / 9) % 9, c = t / 81;
    const float fx = (float)(8 * bi + a) * L.sx, fy = (float)(8 * bj + b) * L.sy, fz = (float)(8 * bk + c) * L.sz;
    const V3 p = v3(L.ox + fx, L.oy + fy, L.oz + fz);
    Counters cnt{0, 0, 0, 0, 0, 0};
    float unused;
    const SceneMin m = sdSceneImpl<BULB, 0, kTrapNone>(sb, p, cnt, __builtin_inff(), unused);
    if (SELECT) {
      in = sn::inside(m.d, iso);
      out = !in;
    } else {
      const size_t at = (size_t)blockIdx.x * (size_t)snb::kBlockPoints + (size_t)t;
      dist[at] = m.d;
      if (ids) ids[at] = m.idx;
    }
  }
  if (SELECT) {
    const unsigned bits = (__ballot(in) != 0ull ? 1u : 0u) | (__ballot(out) != 0ull ? 2u : 0u);  // wave-uniform
    if ((threadIdx.x & 63u) == 0u) atomicOr(&seen, bits);
    __syncthreads();
    if (threadIdx.x == 0) flags[((size_t)bk * (size_t)L.my + (size_t)bj) * (size_t)L.mx + (size_t)bi] = seen == 3u ? 1u : 0u;
  }
}

// ---- the compaction's scan (mesh_scan_kernel's pattern, rm_volume.hip) ----------------------------------------------------------
// Workgroup q turns the n counts off[q·n …] into exclusive offsets in place, carrying the total from one round of 1024 to the next,
// and stores the total in totals[q] and, saturated at 2^32 − 1, in counts[q].
__global__ __launch_bounds__(1024) void blocks_scan_kernel(unsigned long long *__restrict__ off, unsigned n, unsigned long long *__restrict__ totals,
                                                           uint32_t *__restrict__ counts) {
  __shared__ unsigned long long waveSum[16];
  unsigned long long *mine = off + (size_t)blockIdx.x * (size_t)n;
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  unsigned long long carry = 0;  // the same in every lane
  for (unsigned base = 0; base < n; base += 1024u) {
    const unsigned i = base + threadIdx.x;
    const unsigned long long v = i < n ? mine[i] : 0ull;
    unsigned long long s = v;  // inclusive within the wave
    for (unsigned d = 1; d < 64u; d <<= 1) {
      const unsigned long long t = __shfl_up(s, d);
      if (lane >= d) s += t;
    }
    if (lane == 63u) waveSum[wave] = s;
    __syncthreads();
    unsigned long long before = 0, all = 0;
    for (unsigned w = 0; w < 16u; w++) {
      if (w < wave) before += waveSum[w];
      all += waveSum[w];
    }
    if (i < n) mine[i] = carry + before + s - v;
    carry += all;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    totals[blockIdx.x] = carry;
    counts[blockIdx.x] = carry > 0xffffffffull ? 0xffffffffu : (uint32_t)carry;
  }
}
RM_DEV unsigned below(unsigned long long ballot, unsigned lane) { return (unsigned)__popcll(ballot & ((1ull << lane) - 1ull)); }

// ---- rm_sdf_blocks_select's compaction ------------------------------------------------------------------------------------------
// The flags in the blocks' linear order are dealt to workgroups of ONE wave, 1024 consecutive flags each (16 rounds of 64):
// select_count_kernel → blocks_scan_kernel → select_emit_kernel, which numbers the set flags behind its share's offset (ballot +
// popcount) and stores the entries numbered below maxBlocks.  kShareRounds and kShare are rm_internal.h's.

__global__ __launch_bounds__(64) void select_count_kernel(const uint32_t *__restrict__ flags, size_t numFlags, unsigned long long *__restrict__ off) {
  unsigned count = 0;  // wave-uniform
  for (int r = 0; r < kShareRounds; r++) {
    const size_t q = ((size_t)blockIdx.x * kShareRounds + r) * 64u + threadIdx.x;
    count += (unsigned)__popcll(__ballot(q < numFlags && flags[q] != 0u));
  }
  if (threadIdx.x == 0) off[blockIdx.x] = count;
}
__global__ __launch_bounds__(64) void select_emit_kernel(const uint32_t *__restrict__ flags, size_t numFlags, int mx, int my,
                                                         const unsigned long long *__restrict__ off, int maxBlocks, int32_t *__restrict__ list) {
  unsigned long long base = off[blockIdx.x];  // wave-uniform
  for (int r = 0; r < kShareRounds; r++) {
    const size_t q = ((size_t)blockIdx.x * kShareRounds + r) * 64u + threadIdx.x;
    const bool set = q < numFlags && flags[q] != 0u;
    const unsigned long long ballot = __ballot(set);
    const unsigned long long number = base + below(ballot, threadIdx.x);
    if (set && number < (unsigned long long)maxBlocks) {
      const size_t row = q / (size_t)mx;
      int32_t *o = list + 4 * (size_t)number;
      o[0] = (int32_t)(q % (size_t)mx);
      o[1] = (int32_t)(row % (size_t)my);
      o[2] = (int32_t)(row / (size_t)my);
      o[3] = 0;
    }
    base += (unsigned long long)__popcll(ballot);
  }
}
void enqueue_flags_count(const uint32_t *flags, size_t numFlags, unsigned long long *off, uint32_t *d_count, hipStream_t stream) {
  const size_t shares = flag_shares(numFlags);
  hipLaunchKernelGGL(select_count_kernel, dim3((unsigned)shares), dim3(64), 0, stream, flags, numFlags, off);
  hipLaunchKernelGGL(blocks_scan_kernel, dim3(1), dim3(1024), 0, stream, off, (unsigned)shares, off + shares, d_count);
}
void enqueue_flags_emit(const uint32_t *flags, size_t numFlags, int mx, int my, const unsigned long long *off, int maxBlocks, int32_t *d_blocks,
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
  hipLaunchKernelGGL(blocks_map_kernel, dim3(((unsigned)numBlocks + 255u) / 256u), dim3(256), 0, stream, d_blocks, (unsigned)numBlocks, mx, my,
                     mz, first);
  return RM_OK;
}

// ---- the launches of the two staged entry points (rm_queries.hip checks and stages) ----------------------------------------------
static size_t align256(size_t v) { return (v + 255) & ~size_t(255); }
template <bool SELECT, class... Args>
static void launch_eval(int bulbClass, dim3 grid, hipStream_t stream, Args... args) {
  const dim3 block(64 * kEvalWaves);
  dispatch_march_class(bulbClass, [&](auto c) {
    hipLaunchKernelGGL((blocks_eval_kernel<decltype(c)::bulb, SELECT>), grid, block, 0, stream, args...);
  });
}

size_t blocks_select_workspace(int mx, int my, int mz) {
  const size_t blocks = (size_t)mx * (size_t)my * (size_t)mz;
  return align256(blocks * sizeof(uint32_t)) + align256((flag_shares(blocks) + 1) * sizeof(unsigned long long));
}
int launch_blocks_select_kernels(const void *sbv, int bulbClass, const float origin[3], const float step[3], int mx, int my, int mz, float iso,
                                 int maxBlocks, int32_t *d_blocks, uint32_t *d_count, void *workspace, hipStream_t stream) {
  const size_t blocks = (size_t)mx * (size_t)my * (size_t)mz;
  uint32_t *flags = static_cast<uint32_t *>(workspace);
  unsigned long long *off = reinterpret_cast<unsigned long long *>(static_cast<char *>(workspace) + align256(blocks * sizeof(uint32_t)));
  const BlockLattice L{origin[0], origin[1], origin[2], step[0], step[1], step[2], mx, my, mz};
  // at most 512 blocks along every axis: every grid dimension is far below its limit of 65535
  launch_eval<true>(bulbClass, dim3((unsigned)mx, (unsigned)my, (unsigned)mz), stream, static_cast<const SceneBlock *>(sbv), L, iso,
                    (const int32_t *)nullptr, (const uint32_t *)nullptr, flags, (float *)nullptr, (int32_t *)nullptr);
  enqueue_flags_count(flags, blocks, off, d_count, stream);
  if (maxBlocks > 0) enqueue_flags_emit(flags, blocks, mx, my, off, maxBlocks, d_blocks, stream);
  HIP_OK(hipGetLastError());
  return RM_OK;
}

size_t blocks_map_workspace(int mx, int my, int mz) { return align256((size_t)mx * (size_t)my * (size_t)mz * sizeof(uint32_t)); }
int launch_blocks_grid_kernels(const void *sbv, int bulbClass, const float origin[3], const float step[3], int mx, int my, int mz,
                               const int32_t *d_blocks, int numBlocks, float *d_dist, int32_t *d_objectId, void *workspace, hipStream_t stream) {
  uint32_t *first = static_cast<uint32_t *>(workspace);
  if (int st = enqueue_block_map(d_blocks, numBlocks, mx, my, mz, first, stream)) return st;
  const BlockLattice L{origin[0], origin[1], origin[2], step[0], step[1], step[2], mx, my, mz};
  launch_eval<false>(bulbClass, dim3((unsigned)numBlocks), stream, static_cast<const SceneBlock *>(sbv), L, 0.0f, d_blocks,
                     (const uint32_t *)first, (uint32_t *)nullptr, d_dist, d_objectId);
  HIP_OK(hipGetLastError());
  return RM_OK;
}

// The rules the three entry points share for origin, step and the block dimensions, in the header's order.  No HIP call.
int check_block_lattice(const float *origin, const float *step, int mx, int my, int mz) {
  auto bad = [](const char *msg) { set_error(msg); return (int)RM_ERR_INVALID_ARGUMENT; };
  if (!origin || !step) return bad("null origin or step");
  for (int a = 0; a < 3; a++)
    if (!std::isfinite(origin[a])) return bad("origin must be finite");
  for (int a = 0; a < 3; a++)
    if (!std::isfinite(step[a]) || !(step[a] > 0.0f)) return bad("step must be finite and greater than 0 on every axis");
  if (mx < 1 || my < 1 || mz < 1 || mx > RM_MAX_LATTICE_BLOCKS || my > RM_MAX_LATTICE_BLOCKS || mz > RM_MAX_LATTICE_BLOCKS)
    return bad("every block dimension must be 1 … RM_MAX_LATTICE_BLOCKS (512)");
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
  vNumber += below(act, lane);
  // the quads of the cells before this one in the wave, then this cell's own, in axis order
  qNumber += below(q0, lane) + below(q1, lane) + below(q2, lane);
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
  const size_t mapBytes = blocks_map_workspace(mx, my, mz), offBytes = align256((3 * (size_t)numBlocks + 3) * sizeof(unsigned long long)),
               maskBytes = align256((size_t)numBlocks * snb::kMaskWords * sizeof(uint32_t));
  // the workspace is in use until the last launch is enqueued: the device's launcher lock keeps rm_release_workspaces away
  std::unique_lock<std::mutex> lock;
  if (int st = lock_current_device(lock)) return st;
  void *mem = nullptr;
  if (int st = stream_workspace(kWsBlocks, hs, mapBytes + offBytes + maskBytes, &mem)) return st;
  uint32_t *first = static_cast<uint32_t *>(mem);
  unsigned long long *off = reinterpret_cast<unsigned long long *>(static_cast<char *>(mem) + mapBytes), *totals = off + 3 * (size_t)numBlocks;
  uint32_t *masks = reinterpret_cast<uint32_t *>(static_cast<char *>(mem) + mapBytes + offBytes);
  if (int st = enqueue_block_map(d_blocks, numBlocks, mx, my, mz, first, hs)) return st;
  const snb::Blocks B{first, mx, my, mz};
  hipLaunchKernelGGL(mesh_blocks_count_kernel, dim3((unsigned)numBlocks), dim3(512), 0, hs, d_dist, d_blocks, (unsigned)numBlocks, B, iso, off, masks);
  hipLaunchKernelGGL(blocks_scan_kernel, dim3(3), dim3(1024), 0, hs, off, (unsigned)numBlocks, totals, d_counts);
  if (maxVertices > 0 || maxQuads > 0) {
    const BlockLattice L{origin[0], origin[1], origin[2], step[0], step[1], step[2], mx, my, mz};
    hipLaunchKernelGGL(mesh_blocks_emit_kernel, dim3((unsigned)numBlocks), dim3(512), 0, hs, d_dist, d_objectId, d_blocks, (unsigned)numBlocks, B,
                       iso, L, off, totals, masks, maxVertices, maxQuads, d_vertices, d_vertexObject, d_quads);
  }
  HIP_OK(hipGetLastError());
  return RM_OK;
}
