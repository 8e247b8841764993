// rm_animate.hip — the kernels of rm_render_animated for subFrames > 1 (gfx950 only): render_acc_kernel's loop over the n sub-frames
// of an output frame (rm_accumulate.hip), where every scene block may carry an object and a light table of its own.  The launcher
// (argument checks, per-block staging, the class of the call) is launch_animated in rm_launcher.hip; the kernels live here so that
// adding them leaves the code objects of the existing kernels as they were.  subFrames = 1 needs no kernel of its own: the
// production render_kernel classes read block blockIdx.z whole.
#include <hip/hip_runtime.h>

#include "rm_device.hip.h"
#include "rm_internal.h"

namespace rm {

// The workgroup's LDS copy of a block's object table (as render_kernel's).  Every thread of the workgroup calls it.
RM_DEV void stageObjects(RmObject *s_objs, const SceneBlock *sb) {
  const int nd = sb->numObjects * (int)(sizeof(RmObject) / 4);
  const uint32_t *src = reinterpret_cast<const uint32_t *>(sb->objs);
  uint32_t *dst = reinterpret_cast<uint32_t *>(s_objs);
  for (int i = threadIdx.x; i < nd; i += blockDim.x) dst[i] = src[i];
}

// rm_render_animated: output frame blockIdx.z is the mean of the n frames that rm_render_res writes for the scene blocks
// sb[blockIdx.z·n] … sb[blockIdx.z·n + n − 1], each with its own camera, globals, object table and light table, added in that order
// (the header has the definition).  render_acc_kernel's loop — one wave-uniform block per iteration, eight running sums that start
// at −0, unroll(disable) around ONE copy of shadePixel, -ffp-contract=off — with one difference: the LDS copy of the object table
// belongs to a block, not to the call.  It is staged from the frame's first block and again ahead of sub-frame j where the host
// found block j's table to differ from block j − 1's (restage, one bit per block of the call: a kernel argument, so the test is a
// scalar load and a scalar branch).  A restage is two barriers, one before the table that other waves may still read is overwritten
// and one after; a call whose object tables are shared (depth of field, moving lights) has no bit set and executes neither barrier
// nor copy beyond render_acc_kernel's.  Because of those barriers no thread leaves ahead of the loop: a lane outside the frame (a
// partial tile, or a whole wave of a 2- or 4-wave workgroup) stays in it masked off, and a wave without a live lane skips the shading
// on a scalar branch.  The byte→unorm table depends on the class (TEX, the union over the call's blocks) and the settings, which
// every block of a call shares, so the first block's test holds for the call.  Settings, resources, numObjects and numLights are
// the same in every block.  The output frame is blockIdx.z; SceneBlock::frame and the launch fields are not read.
template <int BULB, bool ENV, bool TEX, bool SEC>
__global__ __launch_bounds__(256, render_waves(BULB, ENV, TEX, SEC)) void render_anim_kernel(
    const SceneBlock *__restrict__ sb, RestageBits restage, int W, int H, int n, float scale, float4 *__restrict__ out,
    float4 *__restrict__ bright) {
  const int b0 = (int)blockIdx.z * n;  // wave-uniform: the first of the frame's n scene blocks
  sb += (size_t)b0;
  __shared__ RmObject s_objs[BULB ? 1 : RM_MAX_OBJECTS];
  stageObjects(s_objs, sb);
  if (TEX || (ENV && (sb->s.features & (RM_FEAT_NIGHTSKY_BACKGROUND | RM_FEAT_SEA)))) initUnormTable();
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int x = ((int)blockIdx.x * (int)(blockDim.x >> 6) + wave) * 8 + (lane & 7);
  const int y = (int)blockIdx.y * 8 + (lane >> 3);
  const bool live = x < W && y < H;
  const bool waveLive = __ballot(live) != 0ull;  // wave-uniform
  float acc[8] = {-0.0f, -0.0f, -0.0f, -0.0f, -0.0f, -0.0f, -0.0f, -0.0f};
#pragma clang loop unroll(disable)
  for (int j = 0; j < n; j++) {
    const int b = b0 + j;
    if (j > 0 && ((restage.w[b >> 5] >> (b & 31)) & 1u)) {  // wave-uniform, and the same in every wave of the workgroup
      __syncthreads();  // every wave is done with block j − 1's table
      stageObjects(s_objs, sb + j);
      __syncthreads();
    }
    if (waveLive) {
      if (live) {
        V4 col, br;
        Counters cnt{0, 0, 0, 0, 0, 0};
        bool hit;
        shadePixel<BULB, 0, optClass(ENV, TEX, SEC)>(sb + j, s_objs, x, y, W, H, col, br, cnt, hit);
        acc[0] += col.x; acc[1] += col.y; acc[2] += col.z; acc[3] += col.w;
        acc[4] += br.x; acc[5] += br.y; acc[6] += br.z; acc[7] += br.w;
      }
    }
  }
  if (!live) return;
  // scale = 1.0f / (float)n from the host: 1 for n = 1, and v · 1 is v
  const size_t o = ((size_t)blockIdx.z * (size_t)H + (size_t)y) * (size_t)W + (size_t)x;
  out[o] = make_float4(acc[0] * scale, acc[1] * scale, acc[2] * scale, acc[3] * scale);
  if (bright) bright[o] = make_float4(acc[4] * scale, acc[5] * scale, acc[6] * scale, acc[7] * scale);
}

// The production classes (dispatch_class, rm_internal.h) and nothing more.
int launch_render_anim(const void *sbv, const RestageBits &restage, int bulbClass, bool env, bool tex, bool sec, dim3 grid, dim3 block,
                       int W, int H, int n, float *d_rgba, float *d_bright, hipStream_t stream) {
  const SceneBlock *sb = static_cast<const SceneBlock *>(sbv);
  float4 *o = reinterpret_cast<float4 *>(d_rgba), *b = reinterpret_cast<float4 *>(d_bright);
  const float scale = 1.0f / (float)n;  // one IEEE division, here on the host
  dispatch_class(bulbClass, env, tex, sec, [&](auto c) {
    using K = decltype(c);
    hipLaunchKernelGGL((render_anim_kernel<K::bulb, K::env, K::tex, K::sec>), grid, block, 0, stream, sb, restage, W, H, n, scale, o, b);
  });
  HIP_OK(hipGetLastError());
  return RM_OK;
}

}  // namespace rm
