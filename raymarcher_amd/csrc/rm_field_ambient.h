// rm_field_ambient.h — the arithmetic of rm_field_ambient (include/raymarcher_amd.h has the definition): hemisphere occlusion and
// the bent normal of a point on a baked lattice — the point's normal, the frame around it, the ray of one table entry marched by
// rm_field_skip.h's march as it is, the ray's leaf, and the fixed pairwise tree over the leaves.  ambient_point does all of it for
// one point, a lane's work in the sequential mapping and the whole of the host program's; the kernel of rm_field.hip calls the same
// point_normal, tangent_frame and ray_leaf and folds the leaves of a segment of lanes by an xor butterfly instead: binary32 addition
// is commutative in every bit for operands that are not NaNs, so s[2j] + s[2j + 1] and s[2j + 1] + s[2j] are the same word and both
// walks of the tree give the same sums.
//   Plain C++ with no device built-in, so the kernel and a host program (tests/field_ambient_spec/rm_field_ambient_cpu.cpp) run the
// very same code.  Every operation is one binary32 operation as written: compile with -ffp-contract=off.
#pragma once
#include "rm_field_skip.h"

namespace rm {
namespace fa {

struct Ambient { float bent[3]; float visibility; float normal[3]; int32_t hits; };  // RmAmbient
constexpr int kMaxDirs = 256, kMaxLevels = 8;                                         // RM_MAX_AMBIENT_DIRS and its log2

// Steps a and b: the normal of point p.  given: the caller's normal, or nullptr for the lattice's own gradient at p.  Returns 0
// with n filled, or the code the record stores in `hits` beside zeros.
template <class Field>
RM_SN_FN int point_normal(const Field &F, const fm::Frame &L, const float p[3], const float *given, float n[3]) {
  using namespace fm;
  if (!finite(p[0]) || !finite(p[1]) || !finite(p[2])) return kInvalid;
  if (given) {
    n[0] = given[0], n[1] = given[1], n[2] = given[2];
    if (!finite(n[0]) || !finite(n[1]) || !finite(n[2])) return kInvalid;
    if (n[0] == 0.0f && n[1] == 0.0f && n[2] == 0.0f) return kInvalid;
    return 0;
  }
  const Sample s = sample_point(F, L, p);
  if (s.objectId == kOutside || s.objectId == kUnlisted) return s.objectId;
  const float len = __builtin_sqrtf((s.gradient[0] * s.gradient[0] + s.gradient[1] * s.gradient[1]) + s.gradient[2] * s.gradient[2]);
  if (!finite(len) || len == 0.0f) return kInvalid;
#pragma unroll
  for (int a = 0; a < 3; a++) n[a] = s.gradient[a] / len;
  return 0;
}

// Step c: the branch-free basis of Duff et al. 2017 around n, with the association the definition writes out.  No singular
// direction: n.z = −1 has s = −1 and a = −1 / −2 = 0.5.
RM_SN_FN void tangent_frame(const float n[3], float T[3], float B[3]) {
  const float s = __builtin_copysignf(1.0f, n[2]);
  const float a = -1.0f / (s + n[2]);
  const float b = (n[0] * n[1]) * a;
  T[0] = 1.0f + (s * (n[0] * n[0])) * a;
  T[1] = s * b;
  T[2] = (-s) * n[0];
  B[0] = b;
  B[1] = s + (n[1] * n[1]) * a;
  B[2] = -n[1];
}

// Step d: the ray of table entry e = (local x, y, z, weight) from p, marched; leaf = (c·d.x, c·d.y, c·d.z, c), c = e.w·v.
// Returns whether the ray hit.
template <bool kSoft, class Field>
RM_SN_FN bool ray_leaf(const Field &F, const fs::Coarse &C, const fm::Frame &L, const float p[3], const float n[3], const float T[3],
                       const float B[3], const float e[4], float bias, float maxDistance, float iso, int maxSteps, float leaf[4]) {
  fm::Ray r;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    r.d[a] = (e[0] * T[a] + e[1] * B[a]) + e[2] * n[a];
    r.o[a] = p[a] + n[a] * bias;
  }
  r.tMax = maxDistance;
  const fm::Hit h = fs::march_ray<kSoft>(F, C, L, r, iso, maxSteps, true);
  float v = 0.0f;  // a hit and an invalid ray
  if (h.objectId == fm::kMiss) v = kSoft ? (h.t > 0.0f ? h.t : 0.0f) : 1.0f;
  const float c = e[3] * v;
  leaf[0] = c * r.d[0], leaf[1] = c * r.d[1], leaf[2] = c * r.d[2], leaf[3] = c;
  return h.objectId != fm::kMiss && h.objectId != fm::kInvalid;
}

// rm_field_ambient on one point, steps a to e.  given: the point's normal or nullptr; dirs: the numDirs entries of the point's set,
// four floats each; numDirs a power of two, at most kMaxDirs.  The tree is walked in leaf order with one partial sum per level: when
// leaf k arrives, the levels at which k + 1 is even are complete on the right and fold upwards, left operand first.
template <bool kSoft, class Field>
RM_SN_FN Ambient ambient_point(const Field &F, const fs::Coarse &C, const fm::Frame &L, const float p[3], const float *given, const float *dirs,
                               int numDirs, float bias, float maxDistance, float iso, int maxSteps) {
  Ambient r{{0.0f, 0.0f, 0.0f}, 0.0f, {0.0f, 0.0f, 0.0f}, 0};
  float n[3] = {0.0f, 0.0f, 0.0f}, T[3], B[3];
  if (const int code = point_normal(F, L, p, given, n)) {
    r.hits = code;
    return r;
  }
  tangent_frame(n, T, B);
  float stack[kMaxLevels + 1][4];
  int hits = 0;
  for (int k = 0; k < numDirs; k++) {
    float s[4];
    hits += ray_leaf<kSoft>(F, C, L, p, n, T, B, dirs + 4 * k, bias, maxDistance, iso, maxSteps, s) ? 1 : 0;
    int level = 0;
    for (int done = k + 1; (done & 1) == 0; done >>= 1, level++)
#pragma unroll
      for (int c = 0; c < 4; c++) s[c] = stack[level][c] + s[c];
#pragma unroll
    for (int c = 0; c < 4; c++) stack[level][c] = s[c];
    if (k == numDirs - 1) r.bent[0] = s[0], r.bent[1] = s[1], r.bent[2] = s[2], r.visibility = s[3];
  }
  r.normal[0] = n[0], r.normal[1] = n[1], r.normal[2] = n[2];
  r.hits = hits;
  return r;
}

}  // namespace fa
}  // namespace rm
