// rm_adaptive.hip — the kernels of rm_render_adaptive (gfx950 only): the contrast test over a finished 1-sample frame and the
// supersampling of the pixels it flags.  The launcher (argument checks, staging, chunks, schedule) is launch_adaptive in
// rm_launcher.hip; the kernels live here so that adding them leaves the code objects of the existing kernels as they were.
#include <hip/hip_runtime.h>

#include "rm_device.hip.h"
#include "rm_internal.h"
#include "rm_resolve.hip.h"

namespace rm {

// ---- classify: M(X, Y) of the header, one lane per pixel on 8×8 tiles, frame f0 + blockIdx.z -----------------------------------
// not (|a − b| <= thr) on r, g, b: one binary32 subtraction, a NaN difference flags
RM_DEV bool contrast(const float4 &a, const float4 &b, float thr) {
  return !(__builtin_fabsf(a.x - b.x) <= thr) || !(__builtin_fabsf(a.y - b.y) <= thr) || !(__builtin_fabsf(a.z - b.z) <= thr);
}
// Reads the pixel and its neighbours inside the frame from `rgba` (the 1-sample frames, whole batch), writes mask (if any) and
// appends the flagged pixels' indices Y·W + X to the frame's own list, list + z·W·H (z = the frame's index in the chunk): one
// ballot and one atomic add on counts[z] per wave, the wave's flagged pixels stored contiguously in lane order, so that
// neighbours in the list are neighbours in the image.  Every lane of the wave reaches the ballot; lanes past the edge vote 0.
__global__ __launch_bounds__(256) void adaptive_classify_kernel(const float4 *__restrict__ rgba, int W, int H, int f0, float thr,
                                                                uint8_t *__restrict__ mask, uint32_t *__restrict__ list,
                                                                uint32_t *__restrict__ counts) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int x = ((int)blockIdx.x * (int)(blockDim.x >> 6) + wave) * 8 + (lane & 7);
  const int y = (int)blockIdx.y * 8 + (lane >> 3);
  const bool inside = x < W && y < H;
  const size_t px = (size_t)W * (size_t)H;
  bool m = false;
  if (inside) {
    const float4 *F = rgba + (size_t)(f0 + (int)blockIdx.z) * px;
    const size_t o = (size_t)y * W + x;
    const float4 c = F[o];
    if (x > 0) m = m || contrast(c, F[o - 1], thr);
    if (x + 1 < W) m = m || contrast(c, F[o + 1], thr);
    if (y > 0) m = m || contrast(c, F[o - W], thr);
    if (y + 1 < H) m = m || contrast(c, F[o + W], thr);
    if (mask) mask[(size_t)(f0 + (int)blockIdx.z) * px + o] = m ? 1 : 0;
  }
  const uint64_t votes = __ballot(m);
  if (votes == 0ull) return;  // wave-uniform
  const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(votes >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)votes, 0u));
  uint32_t base = 0u;
  if (lane == 0) base = atomicAdd(&counts[blockIdx.z], (uint32_t)__popcll(votes));
  base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
  if (m) list[(size_t)blockIdx.z * px + base + rank] = (uint32_t)(y * W + x);  // base + rank < W·H: a pixel is listed once
}

// ---- refine: render_ss_kernel's samples and resolve for the listed pixels only -------------------------------------------------
// (the butterfly itself, xorLane / reduceLevel, is rm_resolve.hip.h: render_ss_kernel's)
// A wave is 8×8 lanes, lane = ly·8 + lx, cut into ss × ss sub-blocks as render_ss_kernel's tile is cut into output pixels: 16
// sub-blocks (ss = 2) or 4 (ss = 4), sub-block b = (ly / ss)·(8 / ss) + lx / ss.  Where render_ss_kernel takes the sub-block's
// output pixel from the tile origin, this kernel takes it from the list: wave w of frame blockIdx.z's grid serves entries
// (w + i·waves)·E + b, E = 64 / ss² entries per wave, i = 0, 1, … until the frame's count (device memory, written by the classify
// launch) is passed — the grid is fixed by the host, which never learns the count.  Lane (i, j) = (lx mod ss, ly mod ss) of the
// sub-block shades sample (ss·X + i, ss·Y + j) of the ss·W × ss·H frame, the butterfly resolves, lane (0, 0) overwrites pixel
// (X, Y).  Each frame has a list and a grid slice of its own (blockIdx.z), so the scene block stays wave-uniform.
// The lanes of a sub-block past the end of the list leave together, before the cross-lane reads: entries only grow from one
// iteration to the next, so a sub-block that leaves once has nothing left, and every lane that stays reads lanes of its own
// sub-block only (render_ss_kernel's invariant).
template <int BULB, bool ENV, bool TEX, bool SEC>
__global__ __launch_bounds__(256, render_waves(BULB, ENV, TEX, SEC)) void adaptive_refine_kernel(
    const SceneBlock *__restrict__ sb, int W, int H, int ss, const uint32_t *__restrict__ list, const uint32_t *__restrict__ counts,
    float4 *__restrict__ out, float4 *__restrict__ bright) {
  const uint32_t count = counts[blockIdx.z];
  const uint32_t E = ss == 2 ? 16u : 4u, nw = blockDim.x >> 6;
  // entries and strides fit 32 bits: count <= W·H <= INT_MAX and a grid holds at most 2^18 entries (launch_adaptive)
  if (blockIdx.x * nw * E >= count) return;  // workgroup-uniform, ahead of the barriers: nothing listed for it
  sb += blockIdx.z;  // wave-uniform: the frame's own scene block
  list += (size_t)blockIdx.z * (size_t)W * (size_t)H;
  __shared__ RmObject s_objs[BULB ? 1 : RM_MAX_OBJECTS];
  stageWorkgroup<ENV, TEX>(sb, s_objs);
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t lx = lane & 7u, ly = lane >> 3;
  const uint32_t sub = ss == 2 ? (ly >> 1) * 4u + (lx >> 1) : (ly >> 2) * 2u + (lx >> 2);
  const int si = (int)(lx & (uint32_t)(ss - 1)), sj = (int)(ly & (uint32_t)(ss - 1));
  const int sW = W * ss, sH = H * ss;  // the sample frame
  const size_t frame = (size_t)sb->frame * (size_t)H * (size_t)W;
  for (uint32_t e = (blockIdx.x * nw + wave) * E + sub; e < count; e += gridDim.x * nw * E) {
    const uint32_t p = list[e];
    const int X = (int)(p % (uint32_t)W), Y = (int)(p / (uint32_t)W);
    V4 col, br;
    Counters cnt{0, 0, 0, 0, 0, 0};
    bool hit;
    shadePixel<BULB, 0, optClass(ENV, TEX, SEC)>(sb, s_objs, X * ss + si, Y * ss + sj, sW, sH, col, br, cnt, hit);
    float v[8] = {col.x, col.y, col.z, col.w, br.x, br.y, br.z, br.w};
    reduceLevel<1>(v);               // lanes ^ 1, ^ 8: the 2×2 blocks of the samples
    if (ss == 4) reduceLevel<2>(v);  // wave-uniform; lanes ^ 2, ^ 16: the 2×2 blocks of the first level's result
    if ((si | sj) == 0) {             // one lane per listed pixel stores
      const float scale = ss == 2 ? 0.25f : 0.0625f;
      out[frame + p] = make_float4(v[0] * scale, v[1] * scale, v[2] * scale, v[3] * scale);
      if (bright) bright[frame + p] = make_float4(v[4] * scale, v[5] * scale, v[6] * scale, v[7] * scale);
    }
  }
}

int launch_adaptive_classify(const float *d_rgba, int W, int H, int f0, dim3 grid, dim3 block, float threshold, uint8_t *d_mask,
                             uint32_t *d_list, uint32_t *d_counts, hipStream_t stream) {
  hipLaunchKernelGGL(adaptive_classify_kernel, grid, block, 0, stream, reinterpret_cast<const float4 *>(d_rgba), W, H, f0, threshold,
                     d_mask, d_list, d_counts);
  HIP_OK(hipGetLastError());
  return RM_OK;
}

// The production classes (dispatch_class, rm_internal.h): render_ss_kernel's.
int launch_adaptive_refine(const void *sbv, int bulbClass, bool env, bool tex, bool sec, dim3 grid, dim3 block, int W, int H, int ss,
                           const uint32_t *d_list, const uint32_t *d_counts, float *d_rgba, float *d_bright, hipStream_t stream) {
  const SceneBlock *sb = static_cast<const SceneBlock *>(sbv);
  float4 *o = reinterpret_cast<float4 *>(d_rgba), *b = reinterpret_cast<float4 *>(d_bright);
  dispatch_class(bulbClass, env, tex, sec, [&](auto c) {
    using K = decltype(c);
    hipLaunchKernelGGL((adaptive_refine_kernel<K::bulb, K::env, K::tex, K::sec>), grid, block, 0, stream, sb, W, H, ss, d_list, d_counts, o, b);
  });
  HIP_OK(hipGetLastError());
  return RM_OK;
}

}  // namespace rm
