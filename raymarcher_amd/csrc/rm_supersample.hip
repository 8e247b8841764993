// rm_supersample.hip — the kernels of rm_render_supersampled (gfx950 only): the per-pixel raymarch of rm_kernels.hip with ss × ss
// samples per output pixel, resolved inside the wave.  The launcher (argument checks, staging, schedule) is launch_supersampled in
// rm_launcher.hip; the kernels live here so that adding them leaves the code objects of the existing kernels as they were.
#include <hip/hip_runtime.h>

#include "rm_device.hip.h"
#include "rm_internal.h"
#include "rm_resolve.hip.h"

namespace rm {

// rm_render_supersampled: ss × ss samples per output pixel (ss = 2 or 4), resolved inside the wave that rendered them.  Sample
// (x, y) is pixel (x, y) of the ss·W × ss·H frame of the same camera — the unchanged shadePixel — and a wave's tile is always 8×8
// samples, lane = ly·8 + lx, i.e. 4×4 (ss = 2) or 2×2 (ss = 4) whole output pixels: the resolve needs no memory and no second
// kernel.  The reduction is the fixed tree of the header (x pairs, then y pairs, once or twice, then · 1 / ss²) as a butterfly:
// the binary32 add is commutative, so after `v += xorLane<1>(v)` both lanes of an x pair hold the same bits, after
// `v += xorLane<8>(v)` all four lanes of a 2×2 block do, and lane ^ 2, lane ^ 16 repeat that one level up.  Production only
// (no counters, no light split), raster tile order straight from blockIdx: the launch fields of the scene block are not read.
template <int BULB, bool ENV, bool TEX, bool SEC>
__global__ __launch_bounds__(256, render_waves(BULB, ENV, TEX, SEC)) void render_ss_kernel(
    const SceneBlock *__restrict__ sb, int W, int H, int ss, float4 *__restrict__ out, float4 *__restrict__ bright) {
  sb += blockIdx.z;  // wave-uniform: the frame's own scene block
  __shared__ RmObject s_objs[BULB ? 1 : RM_MAX_OBJECTS];
  stageWorkgroup<ENV, TEX>(sb, s_objs);
  const int sW = W * ss, sH = H * ss;  // the sample frame
  int x, y;
  tilePixel8x8(x, y);
  // Edge lanes leave before the cross-lane reads below, which is safe because of this invariant: ss divides 8 and tile origins are
  // multiples of 8, so an output pixel's ss × ss lanes lie in one wave, and sW, sH are multiples of ss, so those lanes are either
  // all inside the sample frame or all past its edge.  Every lane that stays reads only lanes of its own block, all of which stay.
  if (x >= sW || y >= sH) return;
  V4 col, br;
  Counters cnt{0, 0, 0, 0, 0, 0};
  bool hit;
  shadePixel<BULB, 0, optClass(ENV, TEX, SEC) | kShareBump | kPrep>(sb, s_objs, x, y, sW, sH, col, br, cnt, hit);
  float v[8] = {col.x, col.y, col.z, col.w, br.x, br.y, br.z, br.w};
  reduceLevel<1>(v);               // lanes ^ 1, ^ 8: the 2×2 blocks of S
  if (ss == 4) reduceLevel<2>(v);  // wave-uniform; lanes ^ 2, ^ 16: the 2×2 blocks of the first level's result
  if ((x & (ss - 1)) | (y & (ss - 1))) return;  // one lane per output pixel stores
  const float scale = ss == 2 ? 0.25f : 0.0625f;
  const size_t o = ((size_t)sb->frame * (size_t)H + (size_t)(y / ss)) * (size_t)W + (size_t)(x / ss);
  out[o] = make_float4(v[0] * scale, v[1] * scale, v[2] * scale, v[3] * scale);
  if (bright) bright[o] = make_float4(v[4] * scale, v[5] * scale, v[6] * scale, v[7] * scale);
}

// The production classes (dispatch_class, rm_internal.h) and nothing more.
int launch_render_ss(const void *sbv, int bulbClass, bool env, bool tex, bool sec, dim3 grid, dim3 block, int W, int H, int ss,
                     float *d_rgba, float *d_bright, hipStream_t stream) {
  const SceneBlock *sb = static_cast<const SceneBlock *>(sbv);
  float4 *o = reinterpret_cast<float4 *>(d_rgba), *b = reinterpret_cast<float4 *>(d_bright);
  dispatch_class(bulbClass, env, tex, sec, [&](auto c) {
    using K = decltype(c);
    hipLaunchKernelGGL((render_ss_kernel<K::bulb, K::env, K::tex, K::sec>), grid, block, 0, stream, sb, W, H, ss, o, b);
  });
  HIP_OK(hipGetLastError());
  return RM_OK;
}

}  // namespace rm
