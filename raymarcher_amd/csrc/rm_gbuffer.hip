// rm_gbuffer.hip — the kernels of rm_render_gbuffer (gfx950 only): what the primary ray of every pixel HIT — surface normal, depth,
// object index and, optionally, the surface point — instead of the colour shading makes of it.  The launcher (argument checks,
// staging, the class of the call) is launch_gbuffer in rm_launcher.hip; the kernels live here so that adding them leaves the code
// objects of the existing kernels as they were.
#include <hip/hip_runtime.h>

#include "rm_device.hip.h"
#include "rm_internal.h"

namespace rm {

// rm_render_gbuffer: frame blockIdx.z of the grid reads scene block sb[blockIdx.z] and writes W·H elements of each output from
// frame·W·H (the header has the definition).  A lane is a pixel of its wave's 8×8 tile, the waves of a workgroup side by side, as in
// render_kernel's raster order.  The lane runs the head of render() (rm_device.hip.h) for shadePixel's primary ray and stops there:
// primaryRay, march<BULB, 0, kCull> to cam.initialFar, the surface point rd·d + ro in render's fused form, getNormal with the
// skip-test seeds render derives (ubP from the march's stopping rule, the taps' 0.0005 on top), bumpNormal behind the feature bit —
// the same calls with the same arguments, so the same bits as the values render hands getPhong.  The march's index is stored as it
// comes: an emissive rectangle reports its own index.  A miss stores (0, 0, 0, far), −1 and (0, 0, 0, 0).
// No material is read, so there is no LDS copy of the object table, no unorm table and no barrier, and a lane outside the frame
// leaves at once.  The launch fields of the scene block, the lights and the samplers are not read.  -ffp-contract=off, like every
// kernel here.  Stores: one float4, one dword and optionally a second float4 per lane; the eight lanes of a tile row are 128
// consecutive bytes of normalDepth.
// Register budget (second launch bound): the compiler's report per class and budget is in DESIGN §6.11.  Without shading there is
// nothing outside the march and iteration loops for a spill to land in, so the budget is the largest number of waves per SIMD at
// which the report shows no spill at all: 6 for the table walk (76 VGPRs; a bound of 8 costs 24 bytes of scratch, 5 vector and 8
// scalar registers spilled).  The bulb classes need 43 (plain) and 62 (general) registers under a bound of 6, so eight of their
// waves are resident anyway; asking for 8 only adds 6 scalar spills to the general one.  -DRM_GBUFFER*_WAVES=n overrides.
#ifndef RM_GBUFFER_WAVES
#define RM_GBUFFER_WAVES 6
#endif
#ifndef RM_GBUFFER_BULB_WAVES
#define RM_GBUFFER_BULB_WAVES 6
#endif
constexpr int gbuffer_waves(int bulb) { return bulb ? RM_GBUFFER_BULB_WAVES : RM_GBUFFER_WAVES; }

template <int BULB>
__global__ __launch_bounds__(256, gbuffer_waves(BULB)) void gbuffer_kernel(
    const SceneBlock *__restrict__ sb, int W, int H, float4 *__restrict__ normalDepth, int32_t *__restrict__ objectId,
    float4 *__restrict__ position) {
  sb += blockIdx.z;  // wave-uniform: the frame's own scene block
  int x, y;
  tilePixel8x8(x, y);
  if (x >= W || y >= H) return;
  V3 ro, rd;
  primaryRay(sb, x, y, W, H, ro, rd);
  const float far = sb->cam.initialFar;
  Counters cnt{0, 0, 0, 0, 0, 0};
  const MarchRes res = march<BULB, 0, kCull>(sb, ro, rd, far, 1.0f, cnt);  // a miss reports far, not res.d (frag:2328)
  V3 p = v3(0.0f, 0.0f, 0.0f), n = v3(0.0f, 0.0f, 0.0f);
  float depth = far;
  if (res.obj != -1) {
    depth = res.d;
    p = madd(rd, res.d, ro);
    // render()'s seeds of the skip test: an upper bound of sdScene at p, then at the normal's taps
    constexpr bool SKIP = !BULB;
    float ubP = __builtin_inff();
    if (SKIP) {
      const float lipLen = (sb->cullLip * len(rd)) * 1.0001f;
      ubP = fma(kSurfaceDist, lipLen, kSurfaceDist) * 1.001f + fma(fabs_(res.d), 1.0e-6f, 1.0e-5f);
    }
    n = getNormal<BULB, 0, optIf(SKIP, kSkip)>(sb, p, cnt, SKIP ? fma(0.0005f, sb->cullLip * 1.001f, ubP) : ubP);
    if (sb->s.features & RM_FEAT_PERLIN_BUMP) n = bumpNormal(n, p);
  }
  const size_t o = ((size_t)blockIdx.z * (size_t)H + (size_t)y) * (size_t)W + (size_t)x;
  normalDepth[o] = make_float4(n.x, n.y, n.z, depth);
  objectId[o] = res.obj;
  if (position) position[o] = make_float4(p.x, p.y, p.z, res.obj != -1 ? 1.0f : 0.0f);
}

// The three march classes (dispatch_march_class, rm_internal.h) and nothing more.
int launch_gbuffer_kernel(const void *sbv, int bulbClass, dim3 grid, dim3 block, int W, int H, float *d_normalDepth,
                          int32_t *d_objectId, float *d_position, hipStream_t stream) {
  const SceneBlock *sb = static_cast<const SceneBlock *>(sbv);
  float4 *nd = reinterpret_cast<float4 *>(d_normalDepth), *pos = reinterpret_cast<float4 *>(d_position);
  dispatch_march_class(bulbClass, [&](auto c) {
    hipLaunchKernelGGL((gbuffer_kernel<decltype(c)::bulb>), grid, block, 0, stream, sb, W, H, nd, d_objectId, pos);
  });
  HIP_OK(hipGetLastError());
  return RM_OK;
}

}  // namespace rm
