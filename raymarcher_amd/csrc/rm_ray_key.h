// rm_ray_key.h — the coherence key of rm_rays_order, ONE definition in plain C++ that the kernels (rm_order.hip) and a CPU program
// (tests/ray_order_spec/rm_ray_order_cpu.cpp) both compile, as rm_surface_nets_blocks.h is for the block-sparse meshes.
// include/raymarcher_amd.h has the definition in words.  All arithmetic is binary32, round to nearest even, denormals kept, nothing
// fused (-ffp-contract=off) and `/` correctly rounded; no library function is called, so host and device give the same bits.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define RK_HD __host__ __device__ inline
#else
#define RK_HD inline
#endif

namespace rk {

constexpr int kMaxOriginBits = 10, kMaxDirBits = 11;
constexpr int kCoords = 5;  // ox, oy, oz, u, v

RK_HD uint32_t bits_of(float x) { uint32_t u; __builtin_memcpy(&u, &x, 4); return u; }
RK_HD float float_of(uint32_t u) { float x; __builtin_memcpy(&x, &u, 4); return x; }
RK_HD bool finite(float x) { return (bits_of(x) & 0x7f800000u) != 0x7f800000u; }
RK_HD float magnitude(float x) { return float_of(bits_of(x) & 0x7fffffffu); }
RK_HD float sgn(float x) { return (bits_of(x) >> 31) != 0u ? -1.0f : 1.0f; }  // by the sign bit: −1 for −0

// The five coordinates of a ray (origin o, direction d); false for a ray that is not valid for ordering: a component that is not
// finite, or d all zeros (of either sign).  tMax and `reserved` are not looked at.
RK_HD bool coords(const float o[3], const float d[3], float c[kCoords]) {
  for (int a = 0; a < 3; a++)
    if (!finite(o[a]) || !finite(d[a])) return false;
  if (d[0] == 0.0f && d[1] == 0.0f && d[2] == 0.0f) return false;
  const float s = (magnitude(d[0]) + magnitude(d[1])) + magnitude(d[2]);  // +inf where it overflows: px = py = 0 then
  const float px = d[0] / s, py = d[1] / s;
  c[0] = o[0], c[1] = o[1], c[2] = o[2];
  if (d[2] < 0.0f) {  // the lower half of the octahedron folds outward
    c[3] = (1.0f - magnitude(py)) * sgn(px);
    c[4] = (1.0f - magnitude(px)) * sgn(py);
  } else {
    c[3] = px, c[4] = py;
  }
  return true;
}

// lo and hi of each coordinate over the valid rays: an exact minimum and maximum, so the order of the merges does not matter —
// except for WHICH of −0 and +0 becomes a bound where both occur, and that changes no key: x − lo and hi − lo have the same value
// for either zero (a difference of exactly 0 may change its sign, and every test below treats ±0 alike).
struct Bounds { float lo[kCoords], hi[kCoords]; };
RK_HD void bounds_empty(Bounds &b) {
  for (int k = 0; k < kCoords; k++) b.lo[k] = float_of(0x7f800000u), b.hi[k] = float_of(0xff800000u);  // no valid ray: hi > lo nowhere
}
RK_HD float lower(float a, float b) { return b < a ? b : a; }
RK_HD float upper(float a, float b) { return b > a ? b : a; }
RK_HD void bounds_add(Bounds &b, const float c[kCoords]) {
  for (int k = 0; k < kCoords; k++) b.lo[k] = lower(b.lo[k], c[k]), b.hi[k] = upper(b.hi[k], c[k]);
}
RK_HD void bounds_merge(Bounds &b, const Bounds &o) {
  for (int k = 0; k < kCoords; k++) b.lo[k] = lower(b.lo[k], o.lo[k]), b.hi[k] = upper(b.hi[k], o.hi[k]);
}

// x in [lo, hi] to b bits: three rounded operations, then a truncation.  t < 1 gives t·2^b < 2^b exactly (a scaling by a power of
// two); a NaN t (inf / inf) fails both comparisons and gives 0.
RK_HD uint32_t quantise(float x, float lo, float hi, int b) {
  if (!(hi > lo)) return 0u;
  const float num = x - lo, den = hi - lo;
  const float t = num / den;
  if (t >= 1.0f) return (1u << b) - 1u;
  if (t > 0.0f) return (uint32_t)(t * (float)(1u << b));
  return 0u;
}

// bit i of q to bit 3·i (q below 2^10) and to bit 2·i (q below 2^11)
RK_HD uint64_t spread3(uint32_t q) {
  uint64_t r = 0;
  for (int i = 0; i < kMaxOriginBits; i++) r |= (uint64_t)((q >> i) & 1u) << (3 * i);
  return r;
}
RK_HD uint64_t spread2(uint32_t q) {
  uint64_t r = 0;
  for (int i = 0; i < kMaxDirBits; i++) r |= (uint64_t)((q >> i) & 1u) << (2 * i);
  return r;
}

RK_HD int key_bits(int originBits, int dirBits) { return 3 * originBits + 2 * dirBits + 1; }
// above every valid key: the invalid rays end together
RK_HD uint64_t invalid_key(int originBits, int dirBits) { return 1ull << (3 * originBits + 2 * dirBits); }
// x is the lowest bit of each origin triple, u the lowest bit of each direction pair
RK_HD uint64_t valid_key(const float c[kCoords], const Bounds &b, int originBits, int dirBits) {
  uint32_t q[kCoords];
  for (int k = 0; k < kCoords; k++) q[k] = quantise(c[k], b.lo[k], b.hi[k], k < 3 ? originBits : dirBits);
  const uint64_t o = spread3(q[0]) | (spread3(q[1]) << 1) | (spread3(q[2]) << 2);
  const uint64_t d = spread2(q[3]) | (spread2(q[4]) << 1);
  return (o << (2 * dirBits)) | d;
}
RK_HD uint64_t ray_key(const float o[3], const float d[3], const Bounds &b, int originBits, int dirBits) {
  float c[kCoords];
  return coords(o, d, c) ? valid_key(c, b, originBits, dirBits) : invalid_key(originBits, dirBits);
}

}  // namespace rk
