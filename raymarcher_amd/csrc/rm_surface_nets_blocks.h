// rm_surface_nets_blocks.h — the block-local arithmetic of rm_sdf_blocks_select, rm_sdf_grid_blocks and rm_sdf_mesh_blocks
// (include/raymarcher_amd.h has the definitions): local and global indices of a block of 8×8×8 cells (9×9×9 lattice points), the
// block map and the neighbour lookup through it, which lattice edge gives a stored quad, the open-vertex test and a cell's vertex
// number from its block's base and 512-bit mask of active cells.  The per-cell and per-edge arithmetic is rm_surface_nets.h's,
// called with GLOBAL indices.  Plain C++ with no device built-in, so the kernels of rm_blocks.hip and a host program
// (tests/sdf_blocks_spec/rm_sdf_blocks_cpu.cpp) run the very same code.
#pragma once
#include <cstddef>
#include <cstdint>

#include "rm_surface_nets.h"

namespace rm {
namespace snb {

constexpr int kBlockPoints = 9 * 9 * 9, kBlockCells = 8 * 8 * 8, kMaskWords = kBlockCells / 32;
constexpr uint32_t kNoEntry = 0xffffffffu;  // the block map's value for a block no entry names

// local point (a, b, c), each 0 … 8, in its block's 729 values; local cell (a, b, c), each 0 … 7, among its block's 512 cells
RM_SN_FN int point_index(int a, int b, int c) { return (c * 9 + b) * 9 + a; }
RM_SN_FN int cell_index(int a, int b, int c) { return (c * 8 + b) * 8 + a; }

// The virtual lattice of mx × my × mz blocks and its block map: first[(bk·my + bj)·mx + bi] is the list position of the FIRST
// entry that names block (bi, bj, bk), kNoEntry where none does (a scatter with a minimum over the list).
struct Blocks { const uint32_t *first; int mx, my, mz; };
RM_SN_FN bool in_range(const Blocks &B, int bi, int bj, int bk) { return bi >= 0 && bj >= 0 && bk >= 0 && bi < B.mx && bj < B.my && bk < B.mz; }
RM_SN_FN size_t block_linear(const Blocks &B, int bi, int bj, int bk) { return ((size_t)bk * (size_t)B.my + (size_t)bj) * (size_t)B.mx + (size_t)bi; }
// entry n = (bi, bj, bk) counts (is not void): inside the lattice and the first of its equals
RM_SN_FN bool entry_listed(const Blocks &B, int bi, int bj, int bk, uint32_t n) {
  return in_range(B, bi, bj, bk) && B.first[block_linear(B, bi, bj, bk)] == n;
}
// The entry at work: its block and its list position.  The list position of the block that holds GLOBAL cell (i, j, k) — the
// entry's own without a look at the map —, kNoEntry for a cell outside the lattice or in an unlisted block.
struct Self { int bi, bj, bk; uint32_t n; };
RM_SN_FN uint32_t cell_entry(const Blocks &B, const Self &s, int i, int j, int k) {
  if (i < 0 || j < 0 || k < 0) return kNoEntry;
  const int bi = i >> 3, bj = j >> 3, bk = k >> 3;
  if (bi == s.bi && bj == s.bj && bk == s.bk) return s.n;
  return in_range(B, bi, bj, bk) ? B.first[block_linear(B, bi, bj, bk)] : kNoEntry;
}

// rm_sdf_blocks_select's rule on a block's own 729 values: inside is not the same for all of them
RM_SN_FN bool block_active(const float *vals, float iso) {
  bool anyIn = false, anyOut = false;
  for (int t = 0; t < kBlockPoints; t++) {
    const bool in = sn::inside(vals[t], iso);
    anyIn = anyIn || in;
    anyOut = anyOut || !in;
  }
  return anyIn && anyOut;
}
// the eight corner values of local cell (a, b, c) from its block's values, in rm_surface_nets.h's corner order
RM_SN_FN void cell_corners(const float *vals, int a, int b, int c, float v[8]) {
#pragma unroll
  for (int n = 0; n < 8; n++) v[n] = vals[point_index(a + (n & 1), b + ((n >> 1) & 1), c + ((n >> 2) & 1))];
}

// The lattice edge from GLOBAL point P = (i, j, k) along `axis`, known to be crossed: no quad where it is not interior on the
// virtual lattice (kEdgeNone), a stored quad where all four cells around it lie in listed blocks (kEdgeQuad), else a quad of the
// dense mesh that this list drops (kEdgeDropped).
enum { kEdgeNone = 0, kEdgeQuad = 1, kEdgeDropped = 2 };
RM_SN_FN int crossed_edge_state(const Blocks &B, const Self &s, int axis, int i, int j, int k) {
  if (!sn::edge_interior(axis, i, j, k, 8 * B.mx + 1, 8 * B.my + 1, 8 * B.mz + 1)) return kEdgeNone;
  int cells[4][3];
  sn::edge_cells(axis, i, j, k, true, cells);
  for (int q = 0; q < 4; q++)
    if (cell_entry(B, s, cells[q][0], cells[q][1], cells[q][2]) == kNoEntry) return kEdgeDropped;
  return kEdgeQuad;
}
// The edge from corner 0 of the entry's local cell (a, b, c), corner mask `mask`, along `axis`: the edge that cell's block owns.
RM_SN_FN int owned_edge_state(const Blocks &B, const Self &s, unsigned mask, int axis, int a, int b, int c) {
  if ((((mask >> (1 << axis)) ^ mask) & 1u) == 0u) return kEdgeNone;
  return crossed_edge_state(B, s, axis, 8 * s.bi + a, 8 * s.bj + b, 8 * s.bk + c);
}
// An ACTIVE cell's vertex is open iff one of the cell's twelve edges (rm_surface_nets.h's order) is crossed and gives a dropped quad.
RM_SN_FN bool cell_open(const Blocks &B, const Self &s, unsigned mask, int a, int b, int c) {
  for (int axis = 0; axis < 3; axis++)
    for (int e = 0; e < 4; e++) {
      const int lo = axis == 0 ? 2 * e : (axis == 1 ? (e & 1) + 4 * (e >> 1) : e), hi = lo + (1 << axis);
      if ((((mask >> lo) ^ (mask >> hi)) & 1u) == 0u) continue;
      if (crossed_edge_state(B, s, axis, 8 * s.bi + a + (lo & 1), 8 * s.bj + b + ((lo >> 1) & 1), 8 * s.bk + c + ((lo >> 2) & 1)) == kEdgeDropped)
        return true;
    }
  return false;
}

// The number of set bits of a block's 512-bit mask below bit `cell` (bit n of word w is local cell 32·w + n).
RM_SN_FN uint32_t mask_rank(const uint32_t *mask, unsigned cell) {
  uint32_t r = 0;
  for (unsigned w = 0; w < (cell >> 5); w++) r += (uint32_t)__builtin_popcount(mask[w]);
  return r + (uint32_t)__builtin_popcount(mask[cell >> 5] & ((1u << (cell & 31u)) - 1u));
}
// The vertex number of GLOBAL cell (i, j, k), which lies in the block of listed entry e: that entry's base plus the active cells
// of its block before the cell.  Never above total − 1, whatever the masks hold (a list whose shared faces differ).
RM_SN_FN int32_t vertex_number(const unsigned long long *base, const uint32_t *masks, uint32_t e, int i, int j, int k, unsigned long long total) {
  const unsigned long long n = base[e] + mask_rank(masks + (size_t)e * kMaskWords, (unsigned)cell_index(i & 7, j & 7, k & 7));
  return (int32_t)(n < total ? n : total - 1ull);
}
// The four vertex numbers of the STORED quad of the edge from corner 0 of the entry's local cell (a, b, c) along `axis`.
RM_SN_FN void quad_vertices(const Blocks &B, const Self &s, const unsigned long long *base, const uint32_t *masks, unsigned long long total,
                            int axis, int a, int b, int c, bool pInside, int32_t out[4]) {
  int cells[4][3];
  sn::edge_cells(axis, 8 * s.bi + a, 8 * s.bj + b, 8 * s.bk + c, pInside, cells);
  for (int q = 0; q < 4; q++)
    out[q] = vertex_number(base, masks, cell_entry(B, s, cells[q][0], cells[q][1], cells[q][2]), cells[q][0], cells[q][1], cells[q][2], total);
}

}  // namespace snb
}  // namespace rm
