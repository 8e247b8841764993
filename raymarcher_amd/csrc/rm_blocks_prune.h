// rm_blocks_prune.h — the classification of rm_sdf_blocks_select_pruned (include/raymarcher_amd.h has the definition): the bounds
// from the lattice step and the two constants, whether a corner value is far from the iso surface, and the eight-corner rule that
// discards a block.  Plain C++ with no device built-in, so the kernel of rm_blocks.hip and a host program
// (tests/sdf_prune_spec/rm_blocks_prune_cpu.cpp) run the very same code.  Every operation is one binary32 operation as written:
// compile with -ffp-contract=off (the library's flags).
#pragma once
#include <cmath>
#include <cstddef>

#ifdef __HIPCC__
#define RM_PRUNE_FN __host__ __device__ inline
#else
#define RM_PRUNE_FN inline
#endif

namespace rm {
namespace prune {

// bOut = lipschitzOut · h and bIn = lipschitzIn · h: how far beyond iso a corner value has to lie for the corner to be FAR
struct Bounds { float out, in; };

// h = 4 · sqrt((sx·sx + sy·sy) + sz·sz), half the diagonal of a block: no point of a block is farther from its nearest corner.
// HOST ONLY (the library computes it before the launch): std::sqrt of a float is correctly rounded there.  A step whose square
// overflows gives +inf.
inline float half_diagonal(const float step[3]) {
  const float xx = step[0] * step[0], yy = step[1] * step[1], zz = step[2] * step[2];
  const float xy = xx + yy;
  return 4.0f * std::sqrt(xy + zz);
}
// One rounded multiplication each; 0 · inf is NaN, a bound no value exceeds: it discards nothing.
inline Bounds bounds(const float step[3], float lipschitzOut, float lipschitzIn) {
  const float h = half_diagonal(step);
  return Bounds{lipschitzOut * h, lipschitzIn * h};
}

// Bit 0: the corner is far outside (c − iso > bOut), bit 1: far inside (c − iso < −bIn).  A NaN value is neither, and a value
// exactly at a bound is not far.
RM_PRUNE_FN unsigned corner_far(float c, float iso, Bounds b) {
  const float d = c - iso;
  return (d > b.out ? 1u : 0u) | (d < -b.in ? 2u : 0u);
}
// A block is DISCARDED iff all eight of its corners are far outside, or all eight are far inside.
RM_PRUNE_FN bool discarded(const float c[8], float iso, Bounds b) {
  unsigned all = 3u;
#pragma unroll
  for (int k = 0; k < 8; k++) all &= corner_far(c[k], iso, b);
  return all != 0u;
}

// The corner lattice has (mx + 1)(my + 1)(mz + 1) values, x fastest: corner (i, j, k) is lattice point (8i, 8j, 8k).
RM_PRUNE_FN size_t corner_index(int mx, int my, int i, int j, int k) {
  return ((size_t)k * (size_t)(my + 1) + (size_t)j) * (size_t)(mx + 1) + (size_t)i;
}
// The eight corners of block (bi, bj, bk) in corner order cx + 2·cy + 4·cz.
RM_PRUNE_FN void block_corners(const float *corners, int mx, int my, int bi, int bj, int bk, float c[8]) {
#pragma unroll
  for (int k = 0; k < 8; k++) c[k] = corners[corner_index(mx, my, bi + (k & 1), bj + ((k >> 1) & 1), bk + (k >> 2))];
}

}  // namespace prune
}  // namespace rm
