// rm_field_march.h — the arithmetic of rm_sdf_sample, rm_sdf_sample_blocks, rm_sdf_trace and rm_sdf_trace_blocks
// (include/raymarcher_amd.h has the definition): lattice coordinates, the trilinear cell sample and its gradient, the sample of a
// point, and the march of a ray through a dense lattice or through a block list — the same loop over an accessor.  Plain C++ with no
// device built-in, so the kernels of rm_field.hip and a host program (tests/field_spec/rm_field_cpu.cpp) run the very same code.
// Every operation is one binary32 operation as written: compile with -ffp-contract=off (the library's flags), or the lerps fuse.
#pragma once
#include <cstddef>
#include <cstdint>

#include "rm_surface_nets_blocks.h"

// 1: a marching lane keeps the slot of its current block and looks the block map up only when the block changes; 0: it looks the
// map up at every step.  The results are the same bits; profiles/field_trace.md has the measurement.
#ifndef RM_FIELD_KEEP_SLOT
#define RM_FIELD_KEEP_SLOT 1
#endif

namespace rm {
namespace fm {

constexpr int kInvalid = -2, kOutside = -5, kUnlisted = -6;  // RM_RAY_INVALID, RM_FIELD_OUTSIDE, RM_FIELD_UNLISTED
constexpr int kMiss = -1;

// min, max and clamp as the definition has them: a NaN x clamps to lo
RM_SN_FN float fmin2(float a, float b) { return a < b ? a : b; }
RM_SN_FN float fmax2(float a, float b) { return a > b ? a : b; }
RM_SN_FN float clampf(float x, float lo, float hi) { return fmin2(fmax2(x, lo), hi); }
RM_SN_FN bool finite(float x) { return __builtin_isfinite(x); }
RM_SN_FN int imin(int a, int b) { return a < b ? a : b; }
// (int)floor(x) of an x in [0, 4096]
RM_SN_FN int floor_int(float x) { return (int)__builtin_floorf(x); }
RM_SN_FN float lerp(float a, float b, float w) { return a + w * (b - a); }

// origin and step of the lattice
struct Frame { float o[3], s[3]; };

// ---- the cell sample ---------------------------------------------------------------------------------------------------------------
// v[c], c = cx + 2·cy + 4·cz: the cell's corner values; f: the point's coordinates within the cell.
RM_SN_FN float cell_value(const float v[8], const float f[3]) {
  const float x0 = lerp(v[0], v[1], f[0]), x1 = lerp(v[2], v[3], f[0]), x2 = lerp(v[4], v[5], f[0]), x3 = lerp(v[6], v[7], f[0]);
  return lerp(lerp(x0, x1, f[1]), lerp(x2, x3, f[1]), f[2]);
}
RM_SN_FN void cell_gradient(const float v[8], const float f[3], const float step[3], float g[3]) {
  g[0] = lerp(lerp(v[1] - v[0], v[3] - v[2], f[1]), lerp(v[5] - v[4], v[7] - v[6], f[1]), f[2]) / step[0];
  g[1] = lerp(lerp(v[2] - v[0], v[3] - v[1], f[0]), lerp(v[6] - v[4], v[7] - v[5], f[0]), f[2]) / step[1];
  g[2] = lerp(lerp(v[4] - v[0], v[5] - v[1], f[0]), lerp(v[6] - v[2], v[7] - v[3], f[0]), f[1]) / step[2];
}
// the corner whose id a sample reports: the nearest one, the upper on a tie
RM_SN_FN int id_corner(const float f[3]) { return (f[0] >= 0.5f ? 1 : 0) | (f[1] >= 0.5f ? 2 : 0) | (f[2] >= 0.5f ? 4 : 0); }

// ---- the accessors -----------------------------------------------------------------------------------------------------------------
// Both give the extent per axis, the eight values of a cell and the id at one of its corners.  A SLOT is where a block's values
// live: a list position for Blocks; Dense has one region, slot 0, in which everything is listed.
struct Dense {
  static constexpr bool kSparse = false;
  const float *dist;
  const int32_t *ids;  // may be null
  int n[3];
  RM_SN_FN int extent(int a) const { return n[a] - 1; }
  RM_SN_FN size_t at(const int cell[3], int c) const {
    return ((size_t)(cell[2] + ((c >> 2) & 1)) * (size_t)n[1] + (size_t)(cell[1] + ((c >> 1) & 1))) * (size_t)n[0] + (size_t)(cell[0] + (c & 1));
  }
  // cell: GLOBAL, each 0 … n − 2
  RM_SN_FN void corners(uint32_t, const int cell[3], const int[3], float v[8]) const {
#pragma unroll
    for (int c = 0; c < 8; c++) v[c] = dist[at(cell, c)];
  }
  RM_SN_FN int32_t id(uint32_t, const int cell[3], const int[3], int c) const { return ids[at(cell, c)]; }
};
struct Blocks {
  static constexpr bool kSparse = true;
  const float *dist;
  const int32_t *ids;  // may be null
  snb::Blocks B;       // the block map of the list
  RM_SN_FN int blocks(int a) const { return a == 0 ? B.mx : (a == 1 ? B.my : B.mz); }
  RM_SN_FN int extent(int a) const { return 8 * blocks(a); }
  // the slot of block b, each b_a in [0, m_a): kNoEntry where no entry that counts names it
  RM_SN_FN uint32_t slot(const int b[3]) const { return B.first[snb::block_linear(B, b[0], b[1], b[2])]; }
  RM_SN_FN size_t at(uint32_t slot, const int cell[3], const int b[3], int c) const {
    return (size_t)slot * (size_t)snb::kBlockPoints +
           (size_t)snb::point_index(cell[0] - 8 * b[0] + (c & 1), cell[1] - 8 * b[1] + ((c >> 1) & 1), cell[2] - 8 * b[2] + ((c >> 2) & 1));
  }
  // cell: GLOBAL, in block b
  RM_SN_FN void corners(uint32_t slot, const int cell[3], const int b[3], float v[8]) const {
#pragma unroll
    for (int c = 0; c < 8; c++) v[c] = dist[at(slot, cell, b, c)];
  }
  RM_SN_FN int32_t id(uint32_t slot, const int cell[3], const int b[3], int c) const { return ids[at(slot, cell, b, c)]; }
};

// ---- rm_sdf_sample / rm_sdf_sample_blocks ---------------------------------------------------------------------------------------------
struct Sample { float gradient[3]; float value; int32_t cell[3]; int32_t objectId; };  // RmFieldSample

template <class Field>
RM_SN_FN Sample sample_point(const Field &F, const Frame &L, const float p[3]) {
  Sample s{{0.0f, 0.0f, 0.0f}, 0.0f, {0, 0, 0}, kInvalid};
  if (!finite(p[0]) || !finite(p[1]) || !finite(p[2])) return s;
  float u[3];
  bool in = true;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    u[a] = (p[a] - L.o[a]) / L.s[a];
    in = in && u[a] >= 0.0f && u[a] <= (float)F.extent(a);
  }
  s.objectId = kOutside;
  if (!in) return s;
  int cell[3], b[3] = {0, 0, 0};
  float f[3];
#pragma unroll
  for (int a = 0; a < 3; a++) {
    cell[a] = imin(floor_int(u[a]), F.extent(a) - 1);
    f[a] = u[a] - (float)cell[a];
    s.cell[a] = cell[a];
  }
  uint32_t slot = 0u;
  if constexpr (Field::kSparse) {
#pragma unroll
    for (int a = 0; a < 3; a++) b[a] = imin(cell[a] >> 3, F.blocks(a) - 1);
    slot = F.slot(b);
    if (slot == snb::kNoEntry) {
      s.objectId = kUnlisted;
      return s;
    }
  }
  float v[8];
  F.corners(slot, cell, b, v);
  s.value = cell_value(v, f);
  cell_gradient(v, f, L.s, s.gradient);
  s.objectId = F.ids ? F.id(slot, cell, b, id_corner(f)) : -1;
  return s;
}

// ---- rm_sdf_trace / rm_sdf_trace_blocks -----------------------------------------------------------------------------------------------
struct Ray { float o[3]; float tMax; float d[3]; };
struct Hit { float normal[3]; float t; float position[3]; int32_t objectId; };  // RmRayHit

template <class Field>
RM_SN_FN Hit march_ray(const Field &F, const Frame &L, const Ray &r, float iso, int maxSteps, bool noNormal) {
  Hit h{{0.0f, 0.0f, 0.0f}, 0.0f, {0.0f, 0.0f, 0.0f}, kInvalid};
  // 1. the ray in lattice units
  bool ok = r.tMax >= 0.0f;  // a NaN is not
  float uo[3], ud[3];
#pragma unroll
  for (int a = 0; a < 3; a++) {
    uo[a] = (r.o[a] - L.o[a]) / L.s[a];
    ud[a] = r.d[a] / L.s[a];
    ok = ok && finite(r.o[a]) && finite(r.d[a]) && finite(uo[a]) && finite(ud[a]);
  }
  if (!ok || (ud[0] == 0.0f && ud[1] == 0.0f && ud[2] == 0.0f)) return h;  // dir all zeros has ud all zeros
  h.objectId = kMiss;
  h.t = r.tMax;
  // 2. the box
  float tNear = -__builtin_inff(), tFar = __builtin_inff();
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const float N = (float)F.extent(a);
    if (ud[a] != 0.0f) {
      const float t1 = (0.0f - uo[a]) / ud[a], t2 = (N - uo[a]) / ud[a];
      tNear = fmax2(tNear, fmin2(t1, t2));
      tFar = fmin2(tFar, fmax2(t1, t2));
    } else if (uo[a] < 0.0f || uo[a] > N) {
      return h;
    }
  }
  float t = fmax2(tNear, 0.0f);
  const float tEnd = fmin2(r.tMax, tFar);
  if (!(t <= tEnd)) return h;
  // 3. the march
  bool forced = false;
  int b[3] = {0, 0, 0}, cell[3];
  float u[3], f[3], v[8];
  int kept[3] = {-1, -1, -1};  // the block whose slot `slot` is: a lane looks the map up only when its block changes
  uint32_t slot = 0u;
  for (int i = 0; i < maxSteps; i++) {
    if (t > tEnd) return h;
#pragma unroll
    for (int a = 0; a < 3; a++) {
      u[a] = uo[a] + ud[a] * t;
      if constexpr (Field::kSparse) {
        if (!forced) {
          u[a] = clampf(u[a], 0.0f, (float)F.extent(a));
          b[a] = imin(floor_int(u[a]) >> 3, F.blocks(a) - 1);
        } else {
          u[a] = clampf(u[a], (float)(8 * b[a]), (float)(8 * b[a] + 8));
        }
      } else {
        u[a] = clampf(u[a], 0.0f, (float)F.extent(a));
      }
    }
    if constexpr (Field::kSparse) {
      if (!RM_FIELD_KEEP_SLOT || b[0] != kept[0] || b[1] != kept[1] || b[2] != kept[2]) {
        slot = F.slot(b);
        kept[0] = b[0], kept[1] = b[1], kept[2] = b[2];
      }
      if (slot == snb::kNoEntry) {  // skip to the block's exit
        int axis = -1, dirStep = 0;  // afterwards axis >= 0: ud is not all zeros
        float best = 0.0f;
#pragma unroll
        for (int a = 0; a < 3; a++) {
          if (ud[a] == 0.0f) continue;
          const int up = ud[a] > 0.0f ? 1 : 0;
          const float face = (float)(8 * (b[a] + up)), ta = (face - uo[a]) / ud[a];
          if (axis < 0 || ta < best) axis = a, best = ta, dirStep = 2 * up - 1;
        }
#pragma unroll
        for (int a = 0; a < 3; a++)  // b[axis] without a variable index
          if (a == axis) {
            b[a] += dirStep;
            if (b[a] < 0 || b[a] >= F.blocks(a)) return h;
          }
        t = fmax2(best, t);
        forced = true;
        continue;
      }
    }
#pragma unroll
    for (int a = 0; a < 3; a++) {
      cell[a] = Field::kSparse ? imin(floor_int(u[a]), 8 * b[a] + 7) : imin(floor_int(u[a]), F.extent(a) - 1);
      f[a] = u[a] - (float)cell[a];
    }
    F.corners(slot, cell, b, v);
    forced = false;
    const float value = cell_value(v, f);
    if (value < iso) {  // 4. the hit
      h.t = t;
      h.objectId = F.ids ? F.id(slot, cell, b, id_corner(f)) : 0;
      if (!noNormal) {
        float g[3];
        cell_gradient(v, f, L.s, g);
        const float len = __builtin_sqrtf((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
        const bool unit = finite(len) && len != 0.0f;
#pragma unroll
        for (int a = 0; a < 3; a++) {
          h.normal[a] = unit ? g[a] / len : 0.0f;
          h.position[a] = r.o[a] + r.d[a] * t;
        }
      }
      return h;
    }
    t = t + value;
  }
  return h;
}

}  // namespace fm
}  // namespace rm
