// rm_shade.hip — the kernels of rm_shade_rays (gfx950 only): the renderer's full colour for ARBITRARY rays — the rays come from
// device memory instead of from primaryRay, and everything behind the ray is the render kernels' own device code (shadeRay,
// rm_device.hip.h).  The launcher (argument checks, staging, the class of the call) is launch_shade in rm_queries.hip; the kernels
// live here so that adding them leaves the code objects of the existing kernels as they were.
#include <hip/hip_runtime.h>

#include <climits>

#include "rm_device.hip.h"
#include "rm_internal.h"

namespace rm {

// rm_shade_rays: lane i = blockIdx.x·256 + threadIdx.x is ray i of the call; every ray reads the ONE scene block sb (the header has
// the definition).  The workgroup opens as render_kernel does — the object table to LDS for the per-lane material lookups, the
// byte→unorm table under render_kernel's condition, one barrier — and only BEHIND that barrier do the lanes with i >= numRays and
// the invalid rays leave (an invalid ray after storing zeros).  They must leave before shadeRay, not inside it: the bulb classes'
// shadow pool (shadowPool) is called by every lane of the wave that renders, converged, and holds with absent lanes as it does for
// render_kernel's x >= W — its lists and ballots count the lanes that are there.  A pooled shadow ray is the same sequence of
// evaluations whichever lane marches it, with the call's ONE far (sb->cam.initialFar, wave-uniform like every far in the device
// code): the result of a ray does not depend on the rays it shares a wave with.
// A lane loads its RmRay as two float4 (origin, tMax | dir, reserved; tMax and reserved are not used) and stores its colour, and
// its bright value when asked for, as one float4 each: 2 KB of loads and 1 or 2 KB of stores per wave, contiguous.  dir is used as
// given.  COUNT = 0, SPLIT = 0: production code, no light split.  envLayers is never reached (the launcher refuses the layers) but
// the ENV instantiations compile it, so it gets a constant width.  rayPlane, the rest of cam and the launch fields are never read.
// -ffp-contract=off, like every kernel here.
// Register budget (second launch bound): render_waves of the class, the budgets of render_kernel — the device code behind the ray
// is the same and the compiler's report per instantiation stands beside render_kernel's in DESIGN §6.13.  -DRM_SHADE_*_WAVES=n
// overrides per class.
#ifndef RM_SHADE_GENERIC_WAVES
#define RM_SHADE_GENERIC_WAVES RM_GENERIC_WAVES
#endif
#ifndef RM_SHADE_GENERIC_NOSEC_WAVES
#define RM_SHADE_GENERIC_NOSEC_WAVES RM_GENERIC_NOSEC_WAVES
#endif
#ifndef RM_SHADE_BULB_WAVES
#define RM_SHADE_BULB_WAVES RM_BULB_WAVES
#endif
#ifndef RM_SHADE_BULB_NOSEC_WAVES
#define RM_SHADE_BULB_NOSEC_WAVES RM_BULB_NOSEC_WAVES
#endif
#ifndef RM_SHADE_ENV_WAVES
#define RM_SHADE_ENV_WAVES RM_ENV_WAVES
#endif
#ifndef RM_SHADE_ENV_NOSEC_WAVES
#define RM_SHADE_ENV_NOSEC_WAVES RM_ENV_NOSEC_WAVES
#endif
#ifndef RM_SHADE_TEX_WAVES
#define RM_SHADE_TEX_WAVES RM_TEX_WAVES
#endif
#ifndef RM_SHADE_TEX_NOSEC_WAVES
#define RM_SHADE_TEX_NOSEC_WAVES RM_TEX_NOSEC_WAVES
#endif
constexpr int shade_waves(int bulb, bool env, bool tex, bool sec) {  // render_waves' ladder
  if (tex) return sec ? RM_SHADE_TEX_WAVES : RM_SHADE_TEX_NOSEC_WAVES;
  if (env) return sec ? RM_SHADE_ENV_WAVES : RM_SHADE_ENV_NOSEC_WAVES;
  if (bulb) return sec ? RM_SHADE_BULB_WAVES : RM_SHADE_BULB_NOSEC_WAVES;
  return sec ? RM_SHADE_GENERIC_WAVES : RM_SHADE_GENERIC_NOSEC_WAVES;
}
constexpr int kShadeEnvWidth = 1;  // envLayers' frame width: compiled, never reached

RM_DEV bool finiteBits(float v) { return (f2u(v) & 0x7f800000u) != 0x7f800000u; }

template <int BULB, bool ENV, bool TEX, bool SEC>
__global__ __launch_bounds__(256, shade_waves(BULB, ENV, TEX, SEC)) void shade_rays_kernel(
    const SceneBlock *__restrict__ sb, const float4 *__restrict__ rays, int numRays, float4 *__restrict__ out,
    float4 *__restrict__ bright) {
  __shared__ RmObject s_objs[BULB ? 1 : RM_MAX_OBJECTS];
  stageWorkgroup<ENV, TEX>(sb, s_objs);
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= (unsigned)numRays) return;
  const float4 r0 = rays[2 * (size_t)i], r1 = rays[2 * (size_t)i + 1];
  const V3 ro = v3(r0.x, r0.y, r0.z), rd = v3(r1.x, r1.y, r1.z);
  const bool valid = finiteBits(ro.x) && finiteBits(ro.y) && finiteBits(ro.z) && finiteBits(rd.x) && finiteBits(rd.y) &&
                     finiteBits(rd.z) && (rd.x != 0.0f || rd.y != 0.0f || rd.z != 0.0f);
  if (!valid) {  // alpha 0 marks it: a valid ray's alpha is >= 1
    out[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (bright) bright[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    return;
  }
  V4 col, br = v4(0.0f, 0.0f, 0.0f, 1.0f);
  Counters cnt{0, 0, 0, 0, 0, 0};
  bool hit = false;
  shadeRay<BULB, 0, optClass(ENV, TEX, SEC)>(sb, s_objs, ro, rd, kShadeEnvWidth, col, br, cnt, hit);
  out[i] = make_float4(col.x, col.y, col.z, col.w);
  if (bright) bright[i] = make_float4(br.x, br.y, br.z, br.w);
}

// The production classes (dispatch_class, rm_internal.h) and nothing more.
int launch_shade_kernel(const void *sbv, int bulbClass, bool env, bool tex, bool sec, const void *d_rays, int numRays, float *d_rgba,
                        float *d_bright, hipStream_t stream) {
  static_assert(sizeof(RmRay) == 2 * sizeof(float4), "a ray is two float4");
  static_assert(((long long)INT_MAX + 255) / 256 <= INT_MAX, "every int numRays fits one grid of 256-lane workgroups");
  const SceneBlock *sb = static_cast<const SceneBlock *>(sbv);
  const float4 *rays = static_cast<const float4 *>(d_rays);
  float4 *o = reinterpret_cast<float4 *>(d_rgba), *b = reinterpret_cast<float4 *>(d_bright);
  const dim3 grid((unsigned)(((long long)numRays + 255) / 256)), block(256);
  dispatch_class(bulbClass, env, tex, sec, [&](auto c) {
    using K = decltype(c);
    hipLaunchKernelGGL((shade_rays_kernel<K::bulb, K::env, K::tex, K::sec>), grid, block, 0, stream, sb, rays, numRays, o, b);
  });
  HIP_OK(hipGetLastError());
  return RM_OK;
}

}  // namespace rm
