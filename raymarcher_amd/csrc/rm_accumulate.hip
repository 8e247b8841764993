// rm_accumulate.hip — the kernels of rm_render_accumulated (gfx950 only): the per-pixel raymarch of rm_kernels.hip over the n
// sub-frames (lens samples, shutter times) of an output frame, summed in the lane that rendered them.  The launcher (argument
// checks, staging, schedule) is launch_accumulated in rm_launcher.hip; the kernels live here so that adding them leaves the code
// objects of the existing kernels as they were.
#include <hip/hip_runtime.h>

#include "rm_device.hip.h"
#include "rm_internal.h"

namespace rm {

// rm_render_accumulated: output frame blockIdx.z is the mean of the n frames that rm_render_batch writes for the scene blocks
// sb[blockIdx.z·n] … sb[blockIdx.z·n + n − 1], added in that order (the header has the definition).  A lane keeps its pixel and
// walks the blocks: the block is wave-uniform at every iteration, so the scalar loads of shadePixel stay scalar, and the only state
// a pixel carries from one sub-frame to the next is its eight running sums — no n-sized image exists anywhere.  The object table
// is the same in every block of a call (fill_frames copies block 0), so it is staged into LDS once, from the first.
// The sums start at −0: −0 + v is v for every v, −0 and denormals included, so `acc = S_0` needs no first iteration of its own and
// the loop stays rolled around ONE copy of shadePixel (unroll(disable) also forbids peeling).  -ffp-contract=off keeps the adds
// apart from whatever produced v.  The sums live in VGPRs: the report of -Rpass-analysis=kernel-resource-usage is in DESIGN §6.9.
// The output frame is blockIdx.z; SceneBlock::frame, which counts blocks, is not read.  Production only (no counters, no light
// split), raster tile order straight from blockIdx: the launch fields of the scene block are not read either.
template <int BULB, bool ENV, bool TEX, bool SEC>
__global__ __launch_bounds__(256, render_waves(BULB, ENV, TEX, SEC)) void render_acc_kernel(
    const SceneBlock *__restrict__ sb, int W, int H, int n, float scale, float4 *__restrict__ out, float4 *__restrict__ bright) {
  sb += (size_t)blockIdx.z * (size_t)n;  // wave-uniform: the first of the frame's n scene blocks
  __shared__ RmObject s_objs[BULB ? 1 : RM_MAX_OBJECTS];
  {
    const int nd = sb->numObjects * (int)(sizeof(RmObject) / 4);
    const uint32_t *src = reinterpret_cast<const uint32_t *>(sb->objs);
    uint32_t *dst = reinterpret_cast<uint32_t *>(s_objs);
    for (int i = threadIdx.x; i < nd; i += blockDim.x) dst[i] = src[i];
  }
  if (TEX || (ENV && (sb->s.features & (RM_FEAT_NIGHTSKY_BACKGROUND | RM_FEAT_SEA)))) initUnormTable();
  __syncthreads();
  int x, y;
  tilePixel8x8(x, y);
  if (x >= W || y >= H) return;
  float acc[8] = {-0.0f, -0.0f, -0.0f, -0.0f, -0.0f, -0.0f, -0.0f, -0.0f};
#pragma clang loop unroll(disable)
  for (int j = 0; j < n; j++) {
    V4 col, br;
    Counters cnt{0, 0, 0, 0, 0, 0};
    bool hit;
    shadePixel<BULB, 0, optClass(ENV, TEX, SEC)>(sb + j, s_objs, x, y, W, H, col, br, cnt, hit);
    acc[0] += col.x; acc[1] += col.y; acc[2] += col.z; acc[3] += col.w;
    acc[4] += br.x; acc[5] += br.y; acc[6] += br.z; acc[7] += br.w;
  }
  // scale = 1.0f / (float)n from the host: 1 for n = 1, and v · 1 is v
  const size_t o = ((size_t)blockIdx.z * (size_t)H + (size_t)y) * (size_t)W + (size_t)x;
  out[o] = make_float4(acc[0] * scale, acc[1] * scale, acc[2] * scale, acc[3] * scale);
  if (bright) bright[o] = make_float4(acc[4] * scale, acc[5] * scale, acc[6] * scale, acc[7] * scale);
}

// The production classes (dispatch_class, rm_internal.h) and nothing more.
int launch_render_acc(const void *sbv, int bulbClass, bool env, bool tex, bool sec, dim3 grid, dim3 block, int W, int H, int n,
                      float *d_rgba, float *d_bright, hipStream_t stream) {
  const SceneBlock *sb = static_cast<const SceneBlock *>(sbv);
  float4 *o = reinterpret_cast<float4 *>(d_rgba), *b = reinterpret_cast<float4 *>(d_bright);
  const float scale = 1.0f / (float)n;  // one IEEE division, here on the host
  dispatch_class(bulbClass, env, tex, sec, [&](auto c) {
    using K = decltype(c);
    hipLaunchKernelGGL((render_acc_kernel<K::bulb, K::env, K::tex, K::sec>), grid, block, 0, stream, sb, W, H, n, scale, o, b);
  });
  HIP_OK(hipGetLastError());
  return RM_OK;
}

}  // namespace rm
