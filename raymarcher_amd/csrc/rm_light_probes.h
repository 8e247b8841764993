// rm_light_probes.h — the arithmetic of rm_light_probes behind the shaded ray (include/raymarcher_amd.h has the definition): which
// probes and table rows are valid, the leaf of one ray — its colour and hit flag times the nine basis values of its row — and the
// fixed pairwise tree over the leaves, walked in leaf order.  probe_record does all of it for one probe from colours and hit flags
// that are already there, the whole of the host program's work; the kernel of rm_light_probes.hip calls the same valid_position,
// valid_direction and ray_leaf, folds the 64 leaves a wave holds by an xor butterfly instead — binary32 addition is commutative in
// every bit for operands that are not NaNs (rm_field_ambient.h has the argument), so s[2m] + s[2m + 1] and s[2m + 1] + s[2m] are the
// same word and both walks of the tree give the same sums — and joins the passes of a probe of more than 64 directions by the same
// fold_in_order.
//   Plain C++ with no device built-in, so the kernel and a host program (tests/light_probes_spec/rm_light_probes_cpu.cpp) run the
// very same code.  Every operation is one binary32 operation as written: compile with -ffp-contract=off.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RM_LP_FN __host__ __device__ inline
#else
#define RM_LP_FN inline
#endif

namespace rm {
namespace lp {

constexpr int kBasis = 9, kWords = 4 * kBasis;  // a leaf: (basis·r, basis·g, basis·b, basis·hit) per basis function
constexpr int kMaxDirs = 1024, kMaxLevels = 10; // RM_MAX_PROBE_DIRS and its log2
constexpr int kInvalid = -2;                    // RM_RAY_INVALID
struct Row { float dir[3]; float reserved; float basis[kBasis]; float pad[3]; };      // RmProbeDir
struct Probe { float sh[kBasis][4]; int32_t hits; int32_t reserved[3]; };             // RmLightProbe

RM_LP_FN bool finite(float v) { return v - v == 0.0f; }  // false for ±inf and NaN
// A probe evaluates its rays iff its position is finite.
RM_LP_FN bool valid_position(const float p[3]) { return finite(p[0]) && finite(p[1]) && finite(p[2]); }
// rm_shade_rays' rule for the direction of a ray: every component finite, not all three zero.
RM_LP_FN bool valid_direction(const float d[3]) {
  return finite(d[0]) && finite(d[1]) && finite(d[2]) && (d[0] != 0.0f || d[1] != 0.0f || d[2] != 0.0f);
}

// The leaf of one ray: c = the r, g, b that rm_shade_rays stores for it and hit = whether its primary march found a surface, or
// zeros and false for a row whose direction is invalid.  Nine times four multiplications; a zero colour keeps the basis' sign.
RM_LP_FN void ray_leaf(const float basis[kBasis], const float c[3], bool hit, float leaf[kWords]) {
  const float h = hit ? 1.0f : 0.0f;
#if defined(__clang__)
#pragma unroll
#endif
  for (int j = 0; j < kBasis; j++) {
    leaf[4 * j] = basis[j] * c[0], leaf[4 * j + 1] = basis[j] * c[1], leaf[4 * j + 2] = basis[j] * c[2], leaf[4 * j + 3] = basis[j] * h;
  }
}

// The tree s[m] = s[2m] + s[2m + 1] walked in the order of its leaves with one pending left operand per level: s arrives as the
// sum of group k of `count` equal groups of leaves (count a power of two) — a single leaf on the host, the 64 leaves of a pass in
// the kernel.  The levels at which k + 1 is even are complete on the right and fold upwards, left operand first; what is left waits
// at its level for its right neighbour, but for the last group, whose s is the root.  load(level, word) reads a waiting sum and
// store(level, word, value) leaves one: levels 0 … log2(count) − 1 are used.
template <class Load, class Store>
RM_LP_FN void fold_in_order(int k, int count, float s[kWords], Load &&load, Store &&store) {
  int level = 0;
  for (int done = k + 1; (done & 1) == 0; done >>= 1, level++) {
#if defined(__clang__)
#pragma unroll
#endif
    for (int w = 0; w < kWords; w++) s[w] = load(level, w) + s[w];
  }
  if (k != count - 1) {
#if defined(__clang__)
#pragma unroll
#endif
    for (int w = 0; w < kWords; w++) store(level, w, s[w]);
  }
}

// rm_light_probes on one probe whose rays are shaded: colours — numDirs times (r, g, b, unread) —, hit flags and the numDirs rows
// of the probe's set.  numDirs a power of two, at most kMaxDirs.
RM_LP_FN Probe probe_record(const float position[3], const float *colours, const uint8_t *hit, const Row *rows, int numDirs) {
  Probe r{};
  if (!valid_position(position)) {
    r.hits = kInvalid;
    return r;
  }
  float stack[kMaxLevels][kWords];
  float s[kWords];
  for (int k = 0; k < numDirs; k++) {
    const bool valid = valid_direction(rows[k].dir), h = valid && hit[k] != 0;
    const float zero[3] = {0.0f, 0.0f, 0.0f};
    ray_leaf(rows[k].basis, valid ? colours + 4 * k : zero, h, s);
    r.hits += h ? 1 : 0;
    fold_in_order(k, numDirs, s, [&](int level, int w) { return stack[level][w]; }, [&](int level, int w, float v) { stack[level][w] = v; });
  }
  for (int j = 0; j < kBasis; j++)
    for (int c = 0; c < 4; c++) r.sh[j][c] = s[4 * j + c];
  return r;
}

}  // namespace lp
}  // namespace rm
