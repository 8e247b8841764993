// rm_resolve.hip.h — the in-wave resolve of ss × ss samples on an 8×8 lane tile (lane = ly·8 + lx), shared by the supersampling
// kernels (rm_supersample.hip) and the adaptive refine kernel (rm_adaptive.hip).
#pragma once
#include "rm_device.hip.h"

namespace rm {

// The value of lane (lane ^ MASK) for the four masks of the resolve, without LDS traffic where DPP reaches: ^ 1 and ^ 2 are quad
// permutes, ^ 8 is a rotation by 8 within a row of 16 lanes, ^ 16 a ds_swizzle in bit-mask mode (and 0x1f, or 0, xor 0x10).  The
// source lane must be active (render_ss_kernel's invariant on edge lanes).
template <int MASK>
RM_DEV float xorLane(float f) {
  static_assert(MASK == 1 || MASK == 2 || MASK == 8 || MASK == 16, "lane masks of the 8×8 tile's butterfly");
  const int u = __float_as_int(f);
  if (MASK == 1) return __int_as_float(__builtin_amdgcn_update_dpp(0, u, 0xB1, 0xF, 0xF, true));   // quad_perm:[1,0,3,2]
  if (MASK == 2) return __int_as_float(__builtin_amdgcn_update_dpp(0, u, 0x4E, 0xF, 0xF, true));   // quad_perm:[2,3,0,1]
  if (MASK == 8) return __int_as_float(__builtin_amdgcn_update_dpp(0, u, 0x128, 0xF, 0xF, true));  // row_ror:8
  return __int_as_float(__builtin_amdgcn_ds_swizzle(u, 0x401F));
}
// One level of the tree on the eight channels: x pairs, S(2x, y) + S(2x + 1, y), then y pairs, a(x, 2y) + a(x, 2y + 1).
template <int LEVEL>
RM_DEV void reduceLevel(float (&v)[8]) {
#pragma unroll
  for (int k = 0; k < 8; k++) v[k] += xorLane<LEVEL>(v[k]);
#pragma unroll
  for (int k = 0; k < 8; k++) v[k] += xorLane<8 * LEVEL>(v[k]);
}

}  // namespace rm
