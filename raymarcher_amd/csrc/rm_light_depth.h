// rm_light_depth.h — the arithmetic of rm_light_probes_depth behind the marched ray (include/raymarcher_amd.h has the definition):
// the two leaves of a (row, texel) pair — the row's weight on the texel times the ray's distance and times its square — and the
// fixed pairwise tree of rm_light_probes over the rows, walked in leaf order by ONE lane: texel_sums folds up to 64 leaves with
// the pending sums of six levels in registers, fold_in_order joins the 64-leaf sums of the passes of a probe of more than 64
// directions (rm_light_probes.h's walk, two words wide).  A serial walk adds the same operands in the same pairs as the tree, so
// it has the tree's words; which lane does it is the only freedom.  probe_depth does all of it for one probe from distances that
// are already there, the whole of the host program's work; the kernel of rm_light_depth.hip calls the same ray_moments, texel_sums,
// texel_sums_pass and fold_in_order with lane x as texel x.
//   Plain C++ with no device built-in, so the kernel and a host program (tests/light_depth_spec/rm_light_depth_cpu.cpp) run the
// very same code.  Every operation is one binary32 operation as written: compile with -ffp-contract=off.
#pragma once
#include <cstdint>

#include "rm_light_probes.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RM_LD_FN __host__ __device__ inline
#else
#define RM_LD_FN inline
#endif

namespace rm {
namespace ld {

constexpr int kTexels = 64;      // RM_PROBE_DEPTH_TEXELS: an 8×8 octahedral map
constexpr int kPass = 64;        // leaves that texel_sums folds at the most: one pass of a wave
constexpr int kPassLevels = 6;   // log2(kPass)
constexpr int kJoinLevels = 4;   // log2(RM_MAX_PROBE_DIRS / kPass): the pending sums above the passes of one probe
static_assert(lp::kMaxDirs == kPass << kJoinLevels, "sixteen passes of 64 at the most");
struct Depth { float moments[kTexels][2]; };  // RmProbeDepth

// What a ray leaves for the texels: its distance and the square of it, ONE multiplication.  r = +0 for an invalid row.
RM_LD_FN void ray_moments(float r, float out[2]) { out[0] = r, out[1] = r * r; }

// One leaf pair joins the walk of the tree s[m] = s[2m] + s[2m + 1] in leaf order: s arrives as leaf k of n, the levels at which
// k + 1 is even fold upwards, left operand first, and what is left waits at its level — but for the last leaf, whose s is the root.
// Called from unrolled loops only, so that k and with it every level is known to the compiler and `pending` stays in registers.
RM_LD_FN void join_leaf(int k, int n, float s[2], float pending[][2], int levels) {
  int level = 0;
  for (int done = k + 1; (done & 1) == 0; done >>= 1, level++) s[0] = pending[level][0] + s[0], s[1] = pending[level][1] + s[1];
  // the sum of n leaves is complete at level log2(n) and is the result; below `levels` something may still follow
  if (level < levels && k != n - 1) pending[level][0] = s[0], pending[level][1] = s[1];
}

// The tree over leaves 0 … n − 1 of one texel, n a power of two up to kPass and uniform over a wave, walked by one lane:
// weight(k) is w[k][x], moments(k, float[2]) what ray_moments left for row k.  The rows are asked for one by one.
template <class Weight, class Moments>
RM_LD_FN void texel_sums(int n, Weight &&weight, Moments &&moments, float s[2]) {
  float pending[kPassLevels][2];
#if defined(__clang__)
#pragma unroll
#endif
  for (int k = 0; k < kPass; k++) {
    if (k >= n) break;
    float m[2];
    moments(k, m);
    const float w = weight(k);
    s[0] = w * m[0], s[1] = w * m[1];
    join_leaf(k, n, s, pending, kPassLevels);
  }
}

// The same walk over the kPass leaves of a whole pass, with the weights asked for kAhead rows at a time ahead of their use, so
// that a lane has kAhead loads in flight and not one: behind texel_sums' `break` the compiler may not start the next row's load
// early, and one load per round trip to the cache made the walk of a pass cost as much as a short march.  (Asking ahead with n
// known only at run time needs a clamped row index per load; the compiler's report shows those spilling hundreds of SGPRs.)
constexpr int kAhead = 16;
static_assert(kPass % kAhead == 0, "whole groups");
template <class Weight, class Moments>
RM_LD_FN void texel_sums_pass(Weight &&weight, Moments &&moments, float s[2]) {
  float pending[kPassLevels][2];
#if defined(__clang__)
#pragma unroll
#endif
  for (int base = 0; base < kPass; base += kAhead) {
    float w[kAhead];
#if defined(__clang__)
#pragma unroll
#endif
    for (int j = 0; j < kAhead; j++) w[j] = weight(base + j);
#if defined(__clang__)
#pragma unroll
#endif
    for (int j = 0; j < kAhead; j++) {
      float m[2];
      moments(base + j, m);
      s[0] = w[j] * m[0], s[1] = w[j] * m[1];
      join_leaf(base + j, kPass, s, pending, kPassLevels);
    }
  }
}

// rm_light_probes.h's fold_in_order on two words: s arrives as the sum of group k of `count` equal groups (count a power of two).
template <class Load, class Store>
RM_LD_FN void fold_in_order(int k, int count, float s[2], Load &&load, Store &&store) {
  int level = 0;
  for (int done = k + 1; (done & 1) == 0; done >>= 1, level++) s[0] = load(level, 0) + s[0], s[1] = load(level, 1) + s[1];
  if (k != count - 1) store(level, 0, s[0]), store(level, 1, s[1]);
}

// rm_light_probes_depth on one probe whose rays are marched: t — the numDirs distances rm_trace_rays stores, read only of a valid
// row —, the numDirs rows of the probe's set and their numDirs × kTexels weights.  numDirs a power of two, at most lp::kMaxDirs.
RM_LD_FN Depth probe_depth(const float position[3], const float *t, const lp::Row *rows, const float *weights, int numDirs) {
  Depth r{};
  if (!lp::valid_position(position)) return r;
  const int n = numDirs < kPass ? numDirs : kPass, passes = numDirs / n;
  for (int x = 0; x < kTexels; x++) {
    float join[kJoinLevels][2];
    float s[2] = {0.0f, 0.0f};
    for (int pass = 0; pass < passes; pass++) {
      const int k0 = pass * n;
      const auto weight = [&](int k) { return weights[(size_t)(k0 + k) * kTexels + (size_t)x]; };
      const auto moments = [&](int k, float m[2]) { ray_moments(lp::valid_direction(rows[k0 + k].dir) ? t[k0 + k] : 0.0f, m); };
      if (n == kPass) texel_sums_pass(weight, moments, s);  // the kernel's choice of the form
      else texel_sums(n, weight, moments, s);
      fold_in_order(pass, passes, s, [&](int level, int w) { return join[level][w]; }, [&](int level, int w, float v) { join[level][w] = v; });
    }
    r.moments[x][0] = s[0], r.moments[x][1] = s[1];
  }
  return r;
}

}  // namespace ld
}  // namespace rm
