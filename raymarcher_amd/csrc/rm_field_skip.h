// rm_field_skip.h — the arithmetic of rm_field_trace (include/raymarcher_amd.h has the definition): the march of rm_field_march.h
// over the same accessors, with three differences.  maxSteps counts SAMPLES only, a skip of an unlisted block is free; the mode
// RM_TRACE_OCCLUSION tracks the renderer's penumbra factor beside the same t sequence; and a block handle answers "is this block
// listed?" from a COARSE LEVEL — one 64-bit occupancy mask per group of 4×4×4 blocks, kept in registers while the group does not
// change — so that the block map is loaded for listed blocks only, and an EMPTY group is left in one step.
//   Why that step has the bits of the fine skips.  In an empty group the fine march skips block after block; nothing is sampled, so
// all that the run leaves behind is the block it ends in and t.  Per axis a the fine skips meet the faces F_a,0, F_a,1, … in order,
// ta_a,k = (F_a,k − uo_a) / ud_a, and ta_a,k does not decrease with k: F moves one way, a rounded subtraction is monotone in F, and a
// correctly rounded division by the fixed ud_a is monotone (it turns the order round for a negative ud_a, which is the way F
// moves).  No ta is a NaN: uo and ud are finite, ud_a is not 0.  Each fine skip takes the axis whose next face has the smallest
// (ta, axis), so the run is the stable merge of three sorted sequences by that key: crossing (a, k) comes before (c, j) iff (ta_a,k,
// a) < (ta_c,j, c).  Hence the run leaves the group on the axis A whose LAST face inside the group — the group clipped to the
// lattice, so that leaving the lattice is the miss it is — has the smallest (T_a, a); by then every other axis c has crossed
// exactly its faces inside the group with (ta_c,k, c) < (T_A, A), at most three.  What t the run leaves: every skip does t = ta > t ?
// ta : t, so the fold keeps t if no ta of the run exceeds it, and otherwise the FIRST ta of the run that equals the largest, T_A.
// Two binary32 numbers that compare equal have equal bits unless they are +0 and −0; so for T_A != 0 the fold's result is T_A > t ?
// T_A : t in every bit, a NaN t staying a NaN either way.  For T_A == ±0 the first of several zeros of either sign would have to be
// found (a face the ray starts on gives +0 or −0 by the sign of ud_a), and the sign of a zero t decides the sign of an infinite
// 8·value / t: the step is NOT taken then, and the fine skip below runs as it is written.  The tests `t > tEnd` between the fine
// skips only ever give the miss that the test behind the step gives: t does not decrease.  tests/test_field_handle_spec.py holds
// all this against the fine march (RM_FIELD_COARSE=0) in every bit on rays built to tie and graze, with t above and below 0.
//   Plain C++ with no device built-in, so the handle kernels of rm_field.hip and a host program
// (tests/field_handle_spec/rm_field_handle_cpu.cpp) run the very same code.  Compile with -ffp-contract=off.
#pragma once
#include "rm_field_march.h"

// 1: the march of a block handle reads the coarse level and looks the block map up for listed blocks only; 0: it looks the map up
// whenever its block changes, as rm_sdf_trace_blocks does.  The results are the same bits; profiles/field_handle.md has the
// measurement.
#ifndef RM_FIELD_COARSE
#define RM_FIELD_COARSE 1
#endif

namespace rm {
namespace fs {

// The coarse level of a block list: mask[(gz·g[1] + gy)·g[0] + gx] has bit (bx&3) | (by&3)<<2 | (bz&3)<<4 set iff an entry names
// block (bx, by, bz) of group (bx>>2, by>>2, bz>>2).  g[a] = (m_a + 3) >> 2: the groups at the high faces are ragged, and the bits
// of blocks beyond the lattice are never set and never read.
struct Coarse { const unsigned long long *mask; int g[3]; };
RM_SN_FN int groups(int m) { return (m + 3) >> 2; }
RM_SN_FN size_t group_linear(const int g[3], int bx, int by, int bz) {
  return ((size_t)(bz >> 2) * (size_t)g[1] + (size_t)(by >> 2)) * (size_t)g[0] + (size_t)(bx >> 2);
}
RM_SN_FN unsigned block_bit(int bx, int by, int bz) { return (unsigned)((bx & 3) | ((by & 3) << 2) | ((bz & 3) << 4)); }

// rm_field_trace on one ray.  Field: fm::Dense or fm::Blocks; C is read only for Blocks under RM_FIELD_COARSE.
template <bool kOcclusion, class Field>
RM_SN_FN fm::Hit march_ray(const Field &F, const Coarse &C, const fm::Frame &L, const fm::Ray &r, float iso, int maxSteps, bool noNormal) {
  using namespace fm;
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
  if (!ok || (ud[0] == 0.0f && ud[1] == 0.0f && ud[2] == 0.0f)) return h;
  float res = 1.0f;  // the penumbra factor
  h.objectId = kMiss;
  h.t = kOcclusion ? res : r.tMax;
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
  // 3. the march: a skip `continue`s without a sample; every way out below the loop's head stores res first
  bool forced = false;
  int b[3] = {0, 0, 0}, cell[3];
  float u[3], f[3], v[8];
  int kept[3] = {-1, -1, -1};  // the block whose slot `slot` is
  uint32_t slot = 0u;
#if RM_FIELD_COARSE
  int keptGroup[3] = {-1, -1, -1};  // the group whose mask `mask` is
  unsigned long long mask = 0ull;
#endif
  int samples = 0;
  // `trips` never ends the loop: a run of skips is at most mx + my + mz long and there are at most maxSteps + 1 runs, so the march
  // is over within (maxSteps + 1)·(mx + my + mz + 1) trips, below 2^31.  It is there for the loop's shape: a counter that moves on
  // every trip keeps sampling and skipping lanes of a wave in ONE loop, a trip each, as rm_sdf_trace_blocks' loop has them; without
  // it the compiler nests the sampling trips as a loop inside the loop of the skips (profiles/field_handle.md).
  int extentSum = 0;
  if constexpr (Field::kSparse) extentSum = F.blocks(0) + F.blocks(1) + F.blocks(2);
  const int trips = (maxSteps + 1) * (extentSum + 1);
  for (int trip = 0; trip < trips; trip++) {
    if (t > tEnd) break;
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
      bool listed;
#if RM_FIELD_COARSE
      if ((b[0] >> 2) != keptGroup[0] || (b[1] >> 2) != keptGroup[1] || (b[2] >> 2) != keptGroup[2]) {
        mask = C.mask[group_linear(C.g, b[0], b[1], b[2])];
        keptGroup[0] = b[0] >> 2, keptGroup[1] = b[1] >> 2, keptGroup[2] = b[2] >> 2;
      }
      listed = ((mask >> block_bit(b[0], b[1], b[2])) & 1ull) != 0ull;
      if (listed && (b[0] != kept[0] || b[1] != kept[1] || b[2] != kept[2])) {
        slot = F.slot(b);
        kept[0] = b[0], kept[1] = b[1], kept[2] = b[2];
      }
      listed = listed && slot != snb::kNoEntry;  // the two levels are built from one list: never false here
#else
      if (b[0] != kept[0] || b[1] != kept[1] || b[2] != kept[2]) {
        slot = F.slot(b);
        kept[0] = b[0], kept[1] = b[1], kept[2] = b[2];
      }
      listed = slot != snb::kNoEntry;
#endif
#if RM_FIELD_COARSE
      if (mask == 0ull) {  // the whole group is empty: the run of fine skips that leaves it, in one step (the head has the argument)
        int exitAxis = -1, n[3] = {0, 0, 0}, dir[3] = {0, 0, 0};
        float T = 0.0f;
#pragma unroll
        for (int a = 0; a < 3; a++) {  // the crossing that leaves the group, per axis; the group is clipped to the lattice
          if (ud[a] == 0.0f) continue;
          const int up = ud[a] > 0.0f ? 1 : 0;
          dir[a] = 2 * up - 1;
          n[a] = up ? imin(4 - (b[a] & 3), F.blocks(a) - b[a]) : (b[a] & 3) + 1;  // blocks left in the group, this one included
          const float face = (float)(8 * (b[a] + up + dir[a] * (n[a] - 1))), ta = (face - uo[a]) / ud[a];
          if (exitAxis < 0 || ta < T) exitAxis = a, T = ta;
        }
        if (T != 0.0f) {  // T = ±0: zeros of both signs may tie in the run, and the fine skips below keep the first of them
        bool left = false;
#pragma unroll
        for (int a = 0; a < 3; a++) {
          if (ud[a] == 0.0f) continue;
          if (a == exitAxis) {
            b[a] += dir[a] * n[a];
            left = b[a] < 0 || b[a] >= F.blocks(a);
            continue;
          }
          const int up = ud[a] > 0.0f ? 1 : 0;
          int crossed = 0;  // the faces inside the group the fine skips cross before the exit: those with (ta, a) < (T, exitAxis)
#pragma unroll
          for (int k = 0; k < 3; k++) {
            if (k >= n[a] - 1) continue;
            const float face = (float)(8 * (b[a] + up + dir[a] * k)), ta = (face - uo[a]) / ud[a];
            if (ta < T || (ta == T && a < exitAxis)) crossed++;
          }
          b[a] += dir[a] * crossed;
        }
        if (left) break;
        t = fmax2(T, t);
        forced = true;
        continue;
        }
      }
#endif
      if (!listed) {  // skip to the block's exit: rm_sdf_trace_blocks' step, free of charge
        int axis = -1, dirStep = 0;  // afterwards axis >= 0: ud is not all zeros
        float best = 0.0f;
#pragma unroll
        for (int a = 0; a < 3; a++) {
          if (ud[a] == 0.0f) continue;
          const int up = ud[a] > 0.0f ? 1 : 0;
          const float face = (float)(8 * (b[a] + up)), ta = (face - uo[a]) / ud[a];
          if (axis < 0 || ta < best) axis = a, best = ta, dirStep = 2 * up - 1;
        }
        bool left = false;
#pragma unroll
        for (int a = 0; a < 3; a++)  // b[axis] without a variable index
          if (a == axis) {
            b[a] += dirStep;
            left = b[a] < 0 || b[a] >= F.blocks(a);
          }
        if (left) break;
        t = fmax2(best, t);
        forced = true;
        continue;
      }
    }
    if (samples == maxSteps) break;
    samples++;
#pragma unroll
    for (int a = 0; a < 3; a++) {
      cell[a] = Field::kSparse ? imin(floor_int(u[a]), 8 * b[a] + 7) : imin(floor_int(u[a]), F.extent(a) - 1);
      f[a] = u[a] - (float)cell[a];
    }
    F.corners(slot, cell, b, v);
    forced = false;
    const float value = cell_value(v, f);
    if (value < iso) {  // 4. the hit
      h.objectId = F.ids ? F.id(slot, cell, b, id_corner(f)) : 0;
      if constexpr (kOcclusion) {
        h.t = res;
      } else {
        h.t = t;
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
      }
      return h;
    }
    if constexpr (kOcclusion) {  // softshadow's tracker, k = 8: a NaN q never enters
      const float q = (8.0f * value) / t;
      res = q < res ? q : res;
    }
    t = t + value;
  }
  // 5. the miss: the box or tMax left, the lattice left by a skip, the samples used up
  if constexpr (kOcclusion) h.t = res;
  return h;
}

}  // namespace fs
}  // namespace rm
