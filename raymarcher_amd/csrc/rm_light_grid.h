// rm_light_grid.h — the arithmetic of rm_light_grid_irradiance (include/raymarcher_amd.h has the definition, steps 1 to 9): which
// points are valid, the cell of a point and its trilinear weights, which corner probes take part, DDGI's facing weight, the
// cosine-lobe weights of the normal, the convolution of one probe and the fixed three-level tree over the eight corners.
// grid_light does all of it for one point: a lane's work in the kernel of rm_light_grid.hip and the whole of the host program's.
// The probe records are read through a loader — hits(index) first, sh(index, j, float[4]) only of a probe whose hits >= 0 — so
// that the kernel reads them where rm_light_probes left them and the host program from its own vector.
//   Behind them, and beside them: rm_light_grid_irradiance_visible's step 5a — texel_of, visibility — and grid_light_visible, the
// nine steps with that step between 5 and 6, a lane's work in rm_light_grid_visible.hip; its loader also has depth(index, texel,
// float[2]).  The functions of the nine steps are shared and stay as they are: rm_light_grid.hip's code does not change with this.
//   Plain C++ with no device built-in, so the kernel and a host program (tests/light_grid_spec/rm_light_grid_cpu.cpp) run the very
// same code.  Every operation is one binary32 operation as written: compile with -ffp-contract=off.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RM_LG_FN __host__ __device__ inline
#else
#define RM_LG_FN inline
#endif

namespace rm {
namespace lg {

constexpr int kBasis = 9;              // SH9: the coefficients of one RmLightProbe
constexpr int kInvalid = -2;           // RM_RAY_INVALID
constexpr unsigned kFacing = 1u;       // RM_LIGHT_GRID_FACING
constexpr int kMaxDim = 1024;          // RM_MAX_LIGHT_GRID_DIM
constexpr int kMaxProbes = 1 << 24;    // RM_MAX_LIGHT_GRID_PROBES
struct GridLight { float e[4]; float weight; int32_t probes; int32_t reserved[2]; };  // RmGridLight
struct Grid { int dims[3]; float origin[3], step[3]; };

// Step 7's constants: A_band·(the basis function's factor), in binary64, rounded once.
constexpr float K0 = (float)0.8862269254527579;   // π·sqrt(1/4π)
constexpr float K1 = (float)1.0233267079464883;   // (2π/3)·sqrt(3/4π)
constexpr float K2 = (float)0.8580855308097834;   // (π/4)·sqrt(15/4π)
constexpr float K6 = (float)0.24770795610037571;  // (π/4)·sqrt(5/16π)
constexpr float K8 = (float)0.4290427654048917;   // (π/4)·sqrt(15/16π)

RM_LG_FN bool finite(float v) { return v - v == 0.0f; }  // false for ±inf and NaN

// Step 1: every component of p and n finite, n not all zeros.
RM_LG_FN bool valid_point(const float p[3], const float n[3]) {
  return finite(p[0]) && finite(p[1]) && finite(p[2]) && finite(n[0]) && finite(n[1]) && finite(n[2]) &&
         (n[0] != 0.0f || n[1] != 0.0f || n[2] != 0.0f);
}

// Step 2 on one axis: the cell and the fraction of p.  dim >= 2; u ends in [0, dim − 1], so the conversion truncates a value that
// is not negative: floor.
RM_LG_FN void cell_of(float p, float origin, float step, int dim, int *cell, float *f) {
  float u = (p - origin) / step;
  const float top = (float)(dim - 1);
  if (!(u > 0.0f)) u = 0.0f;
  if (u > top) u = top;
  int c = (int)u;
  if (c > dim - 2) c = dim - 2;
  *cell = c;
  *f = u - (float)c;
}

// The linear index of probe (i, j, k): at most kMaxProbes − 1.  Byte offsets of it need 64 bits (160 B a record).
RM_LG_FN size_t probe_index(const Grid &G, int i, int j, int k) { return (size_t)i + (size_t)G.dims[0] * ((size_t)j + (size_t)G.dims[1] * (size_t)k); }

// Step 5 behind the flag: the backface term of Majercik et al. 2019 for the probe at q seen from p with normal n.
RM_LG_FN float facing(const float q[3], const float p[3], const float n[3]) {
  const float dx = q[0] - p[0], dy = q[1] - p[1], dz = q[2] - p[2];
  const float len = __builtin_sqrtf((dx * dx + dy * dy) + dz * dz);
  if (len == 0.0f) return 1.0f;
  const float cosv = ((dx * n[0] + dy * n[1]) + dz * n[2]) / len;
  const float b = (cosv + 1.0f) * 0.5f;
  return b * b + 0.2f;
}

// Step 7: the nine weights of the clamped-cosine lobe around n, rm_sphere_directions' order of Y0 … Y8.
RM_LG_FN void lobe_weights(const float n[3], float k[kBasis]) {
  const float x = n[0], y = n[1], z = n[2];
  k[0] = K0;
  k[1] = K1 * y, k[2] = K1 * z, k[3] = K1 * x;
  k[4] = K2 * (x * y), k[5] = K2 * (y * z), k[7] = K2 * (x * z);
  k[6] = K6 * (3.0f * (z * z) - 1.0f);
  k[8] = K8 * (x * x - y * y);
}

// Steps 6 and 8: ((v0 + v1) + (v2 + v3)) + ((v4 + v5) + (v6 + v7)).
RM_LG_FN float tree8(const float v[8]) { return ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7])); }

// rm_light_grid_irradiance on one point, steps 1 to 9.  load.hits(index) → the record's hits; load.sh(index, j, out) → its sh[j],
// four floats — asked only of a probe with hits >= 0, and of none when no corner takes part.
template <class Load>
RM_LG_FN GridLight grid_light(const Grid &G, const float p[3], const float n[3], unsigned flags, Load &&load) {
  GridLight r{{0.0f, 0.0f, 0.0f, 0.0f}, 0.0f, 0, {0, 0}};
  if (!valid_point(p, n)) {
    r.probes = kInvalid;
    return r;
  }
  int cell[3];
  float f[3];
#if defined(__clang__)
#pragma unroll
#endif
  for (int a = 0; a < 3; a++) cell_of(p[a], G.origin[a], G.step[a], G.dims[a], &cell[a], &f[a]);
  size_t index[8];
  bool valid[8];
  float w[8];
  int probes = 0;
#if defined(__clang__)
#pragma unroll
#endif
  for (int c = 0; c < 8; c++) {
    const int at[3] = {cell[0] + (c & 1), cell[1] + ((c >> 1) & 1), cell[2] + ((c >> 2) & 1)};
    index[c] = probe_index(G, at[0], at[1], at[2]);
    valid[c] = load.hits(index[c]) >= 0;
    w[c] = 0.0f;
    if (valid[c]) {
      const float wx = (c & 1) ? f[0] : 1.0f - f[0], wy = (c & 2) ? f[1] : 1.0f - f[1], wz = (c & 4) ? f[2] : 1.0f - f[2];
      float face = 1.0f;
      if (flags & kFacing) {
        float q[3];
        for (int a = 0; a < 3; a++) q[a] = G.origin[a] + (float)at[a] * G.step[a];
        face = facing(q, p, n);
      }
      w[c] = ((wx * wy) * wz) * face;
      probes += w[c] > 0.0f ? 1 : 0;
    }
  }
  const float W = tree8(w);
  r.weight = W;
  r.probes = probes;
  if (probes == 0) return r;
  float k[kBasis];
  lobe_weights(n, k);
  float leaf[4][8];
#if defined(__clang__)
#pragma unroll
#endif
  for (int c = 0; c < 8; c++) {
    leaf[0][c] = leaf[1][c] = leaf[2][c] = leaf[3][c] = 0.0f;
    if (valid[c]) {
      float E[4], s[4];
      load.sh(index[c], 0, s);
      for (int ch = 0; ch < 4; ch++) E[ch] = k[0] * s[ch];
#if defined(__clang__)
#pragma unroll
#endif
      for (int j = 1; j < kBasis; j++) {
        load.sh(index[c], j, s);
        for (int ch = 0; ch < 4; ch++) E[ch] = E[ch] + k[j] * s[ch];
      }
      for (int ch = 0; ch < 4; ch++) leaf[ch][c] = w[c] * E[ch];
    }
  }
  for (int ch = 0; ch < 4; ch++) r.e[ch] = tree8(leaf[ch]) / W;
  return r;
}

// ---- rm_light_grid_irradiance_visible: the nine steps with step 5a between 5 and 6 ------------------------------------------------
constexpr float kVisFloor = 1.0e-6f;   // RM_LIGHT_GRID_VIS_FLOOR
constexpr int kDepthSide = 8;          // an RmProbeDepth is an 8×8 octahedral map, texel tx + 8·ty

// One axis of the map: the octahedral coordinate o in [−1, 1] → the left texel of the pair to blend and the fraction.  Texel
// centres are at −0.875 … 0.875, so u = o·4 + 3.5 counts texels from the first centre; it is clamped as cell_of clamps (a u not
// greater than 0 becomes +0): outside the centres the blend repeats the edge texel, the octahedral wrap is not followed.
RM_LG_FN void texel_of(float o, int *i, float *f) {
  float u = o * 4.0f + 3.5f;
  if (!(u > 0.0f)) u = 0.0f;
  if (u > 7.0f) u = 7.0f;
  int c = (int)u;
  if (c > kDepthSide - 2) c = kDepthSide - 2;
  *i = c;
  *f = u - (float)c;
}

// Step 5a: the Chebyshev visibility (Majercik et al. 2019) of the biased point q from the probe at pp, whose depth moments
// load.depth(index, texel, float[2]) gives — asked only of a valid probe, four texels, and of none when q is at the probe.
template <class Load>
RM_LG_FN float visibility(const float q[3], const float pp[3], size_t index, Load &&load) {
  const float vx = q[0] - pp[0], vy = q[1] - pp[1], vz = q[2] - pp[2];
  const float r = __builtin_sqrtf((vx * vx + vy * vy) + vz * vz);
  if (r == 0.0f) return 1.0f;
  const float l1 = (__builtin_fabsf(vx) + __builtin_fabsf(vy)) + __builtin_fabsf(vz);
  float ox = vx / l1, oy = vy / l1;
  if (vz < 0.0f) {
    const float fx = (1.0f - __builtin_fabsf(oy)) * (ox >= 0.0f ? 1.0f : -1.0f), fy = (1.0f - __builtin_fabsf(ox)) * (oy >= 0.0f ? 1.0f : -1.0f);
    ox = fx, oy = fy;
  }
  int ix, iy;
  float fx, fy;
  texel_of(ox, &ix, &fx);
  texel_of(oy, &iy, &fy);
  float a[2], b[2], c[2], d[2];
  const int x0 = ix + kDepthSide * iy;
  load.depth(index, x0, a);
  load.depth(index, x0 + 1, b);
  load.depth(index, x0 + kDepthSide, c);
  load.depth(index, x0 + kDepthSide + 1, d);
  const float gx = 1.0f - fx, gy = 1.0f - fy;
  const float m = (a[0] * gx + b[0] * fx) * gy + (c[0] * gx + d[0] * fx) * fy;
  const float m2 = (a[1] * gx + b[1] * fx) * gy + (c[1] * gx + d[1] * fx) * fy;
  if (r <= m) return 1.0f;
  const float var = __builtin_fabsf(m2 - m * m), dd = r - m, den = var + dd * dd;
  const float cheb = den == 0.0f ? 1.0f : var / den;
  const float v = (cheb * cheb) * cheb;
  return v > kVisFloor ? v : kVisFloor;
}

// rm_light_grid_irradiance_visible on one point: grid_light's steps 1 to 9 with w_c = (t_c·face)·vis.  The loader has grid_light's
// hits and sh and visibility's depth.
template <class Load>
RM_LG_FN GridLight grid_light_visible(const Grid &G, const float p[3], const float n[3], unsigned flags, float normalBias, Load &&load) {
  GridLight r{{0.0f, 0.0f, 0.0f, 0.0f}, 0.0f, 0, {0, 0}};
  if (!valid_point(p, n)) {
    r.probes = kInvalid;
    return r;
  }
  int cell[3];
  float f[3], q[3];
#if defined(__clang__)
#pragma unroll
#endif
  for (int a = 0; a < 3; a++) {
    cell_of(p[a], G.origin[a], G.step[a], G.dims[a], &cell[a], &f[a]);
    q[a] = p[a] + normalBias * n[a];
  }
  size_t index[8];
  bool valid[8];
  float w[8];
  int probes = 0;
#if defined(__clang__)
#pragma unroll
#endif
  for (int c = 0; c < 8; c++) {
    const int at[3] = {cell[0] + (c & 1), cell[1] + ((c >> 1) & 1), cell[2] + ((c >> 2) & 1)};
    index[c] = probe_index(G, at[0], at[1], at[2]);
    valid[c] = load.hits(index[c]) >= 0;
    w[c] = 0.0f;
    if (valid[c]) {
      const float wx = (c & 1) ? f[0] : 1.0f - f[0], wy = (c & 2) ? f[1] : 1.0f - f[1], wz = (c & 4) ? f[2] : 1.0f - f[2];
      float pp[3];
      for (int a = 0; a < 3; a++) pp[a] = G.origin[a] + (float)at[a] * G.step[a];
      const float face = (flags & kFacing) ? facing(pp, p, n) : 1.0f;
      w[c] = (((wx * wy) * wz) * face) * visibility(q, pp, index[c], load);
      probes += w[c] > 0.0f ? 1 : 0;
    }
  }
  const float W = tree8(w);
  r.weight = W;
  r.probes = probes;
  if (probes == 0) return r;
  float k[kBasis];
  lobe_weights(n, k);
  float leaf[4][8];
#if defined(__clang__)
#pragma unroll
#endif
  for (int c = 0; c < 8; c++) {
    leaf[0][c] = leaf[1][c] = leaf[2][c] = leaf[3][c] = 0.0f;
    if (valid[c]) {
      float E[4], s[4];
      load.sh(index[c], 0, s);
      for (int ch = 0; ch < 4; ch++) E[ch] = k[0] * s[ch];
#if defined(__clang__)
#pragma unroll
#endif
      for (int j = 1; j < kBasis; j++) {
        load.sh(index[c], j, s);
        for (int ch = 0; ch < 4; ch++) E[ch] = E[ch] + k[j] * s[ch];
      }
      for (int ch = 0; ch < 4; ch++) leaf[ch][c] = w[c] * E[ch];
    }
  }
  for (int ch = 0; ch < 4; ch++) r.e[ch] = tree8(leaf[ch]) / W;
  return r;
}

}  // namespace lg
}  // namespace rm
