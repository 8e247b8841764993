// rm_shade_indirect.hip — the kernels of rm_shade_rays_indirect (gfx950 only): rm_shade_rays' colour with the diffuse term of a light
// grid added at the primary hit, ONE launch, one lane per ray.  The device code is rm_indirect.hip.h's shadeRayIndirect; the launcher
// (argument checks, staging, the class of the call) is launch_shade_indirect in rm_queries.hip; the kernels live here so that
// adding them leaves the code objects of the existing kernels as they were.
#include <hip/hip_runtime.h>

#include <climits>

#include "rm_indirect.hip.h"
#include "rm_internal.h"

namespace rm {

// rm_shade_rays_indirect: shade_rays_kernel's lanes, loads, stores and exits (rm_shade.hip) — lane i is ray i, the workgroup opens
// with stageWorkgroup and one barrier, and only behind it do the lanes past the end and the invalid rays leave, before the bulb
// classes' shadow pool counts the lanes that are there.  The grid comes by value in the kernel's arguments (64 bytes).  Behind the
// hit a lane gathers its cell's eight hits words, the nine float4 of every valid corner and, with depth records, four texels of
// each: up to sixteen lines of 128 bytes where the hits of a wave diverge.  There is no bright output.  -ffp-contract=off.
// Register budget (second launch bound): rm_shade.hip's rule — render_waves of the class; the compiler's report per instantiation
// stands beside shade_rays_kernel's in DESIGN §6.28.
RM_DEV bool finiteBits(float v) { return (f2u(v) & 0x7f800000u) != 0x7f800000u; }

template <int BULB, bool ENV, bool TEX, bool SEC>
__global__ __launch_bounds__(256, render_waves(BULB, ENV, TEX, SEC)) void shade_rays_indirect_kernel(
    const SceneBlock *__restrict__ sb, const float4 *__restrict__ rays, int numRays, IndirectGrid grid, float4 *__restrict__ out) {
  __shared__ RmObject s_objs[BULB ? 1 : RM_MAX_OBJECTS];
  stageWorkgroup<ENV, TEX>(sb, s_objs);
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= (unsigned)numRays) return;
  const float4 r0 = rays[2 * (size_t)i], r1 = rays[2 * (size_t)i + 1];
  const V3 ro = v3(r0.x, r0.y, r0.z), rd = v3(r1.x, r1.y, r1.z);
  const bool valid = finiteBits(ro.x) && finiteBits(ro.y) && finiteBits(ro.z) && finiteBits(rd.x) && finiteBits(rd.y) &&
                     finiteBits(rd.z) && (rd.x != 0.0f || rd.y != 0.0f || rd.z != 0.0f);
  if (!valid) {
    out[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    return;
  }
  V4 col;
  bool hit = false;
  shadeRayIndirect<BULB, optClass(ENV, TEX, SEC)>(sb, s_objs, ro, rd, grid, col, hit);
  out[i] = make_float4(col.x, col.y, col.z, col.w);
}

// The production classes (dispatch_class, rm_internal.h) and nothing more.
int launch_shade_indirect_kernel(const void *sbv, int bulbClass, bool env, bool tex, bool sec, const void *d_rays, int numRays,
                                 const IndirectGridArgs &ga, float *d_rgba, hipStream_t stream) {
  static_assert(((long long)INT_MAX + 255) / 256 <= INT_MAX, "every int numRays fits one grid of 256-lane workgroups");
  const SceneBlock *sb = static_cast<const SceneBlock *>(sbv);
  const float4 *rays = static_cast<const float4 *>(d_rays);
  float4 *o = reinterpret_cast<float4 *>(d_rgba);
  const IndirectGrid grid{static_cast<const char *>(ga.d_probes), static_cast<const char *>(ga.d_depth),
                          lg::Grid{{ga.dims[0], ga.dims[1], ga.dims[2]}, {ga.origin[0], ga.origin[1], ga.origin[2]}, {ga.step[0], ga.step[1], ga.step[2]}},
                          ga.k, ga.flags, ga.normalBias};
  const dim3 grd((unsigned)(((long long)numRays + 255) / 256)), block(256);
  dispatch_class(bulbClass, env, tex, sec, [&](auto c) {
    using K = decltype(c);
    hipLaunchKernelGGL((shade_rays_indirect_kernel<K::bulb, K::env, K::tex, K::sec>), grd, block, 0, stream, sb, rays, numRays, grid, o);
  });
  HIP_OK(hipGetLastError());
  return RM_OK;
}

}  // namespace rm
