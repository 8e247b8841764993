// rm_trace.hip — the kernels of rm_trace_rays (gfx950 only): what ARBITRARY rays hit — the rays come from device memory instead of
// from primaryRay.  Closest hit (object index, t, surface point, normal) or the renderer's own shadow march (occluder index and
// penumbra factor).  The launcher (argument checks, staging, the class of the call) is launch_trace in rm_queries.hip; the kernels
// live here so that adding them leaves the code objects of the existing kernels as they were.
#include <hip/hip_runtime.h>

#include "rm_device.hip.h"
#include "rm_internal.h"

namespace rm {

// rm_trace_rays: lane i = blockIdx.x·256 + threadIdx.x is ray i of the call; every ray reads the ONE scene block sb (the header has
// the definition).  A lane loads its RmRay as two float4 (origin, tMax | dir, reserved) and stores its RmRayHit as two float4
// (normal, t | position, objectId): 2 KB contiguous per wave each way, plain vector loads and stores.  Between them it makes
// gbuffer_kernel's device calls (rm_gbuffer.hip) with the ray in place of primaryRay's:
//   closest (MODE 0): march<BULB, 0, kCull> to the ray's tMax, the surface point rd·d + ro in render's fused form, getNormal
//     with the skip-test seeds render derives (ubP from the march's stopping rule, the taps' 0.0005 on top), bumpNormal behind the
//     feature bit.  noNormal (a kernel argument, so wave-uniform) leaves the surface point and the taps out: zeros are stored.
//   occlusion (MODE 1): march<BULB, 0, kShadow | kCull> with the default ub0 — lightTerm's shadow march.  The launcher stages
//     enableSoftShadow = 1, so the penumbra factor is always tracked, and cullR2Soft = 0: the larger ball of the soft-shadow rays is
//     derived for rays that START inside the cull ball (rm_frame.cpp, scene_cull_ball), which a caller's rays need not.
// dir is used as given: len(rd) enters the skip test's Lipschitz seeds exactly as for a unit direction, and the cull ball and box
// solve their quadratics with a = dot(rd, rd).  A lane with i >= numRays leaves at once, and so does an invalid ray after storing
// RM_RAY_INVALID: the march's __ballot / readfirstlane decisions do not depend on which lanes are live (every one of them is a
// proof about all lanes that ARE live), so the result of a ray does not depend on the rays it shares a wave with.
// No material is read: no LDS, no barrier, no light table.  rayPlane, cam, the launch fields and the samplers of the block are never
// read.  -ffp-contract=off, like every kernel here.
// Register budget (second launch bound): the compiler's report per instantiation and budget is in DESIGN §6.12; the rule is
// rm_gbuffer.hip's — the most waves per SIMD at which the report shows no spill at all.  That is 7 for the table walk (71 VGPRs in
// both modes, seven waves resident; a bound of 8 costs 16 to 32 bytes of scratch) and for the general bulb (57 / 58 VGPRs, so eight of
// its waves are resident anyway; asking for 8 only adds two scalar spills), and 8 for the plain bulb (42 / 44 VGPRs, no spill).
// -DRM_TRACE*_WAVES=n overrides.
#ifndef RM_TRACE_WAVES
#define RM_TRACE_WAVES 7
#endif
#ifndef RM_TRACE_PLAIN_BULB_WAVES
#define RM_TRACE_PLAIN_BULB_WAVES 8
#endif
constexpr int trace_waves(int bulb) { return bulb == kBulbPlain ? RM_TRACE_PLAIN_BULB_WAVES : RM_TRACE_WAVES; }
constexpr int kTraceClosest = 0, kTraceOcclusion = 1;

RM_DEV bool finiteBits(float v) { return (f2u(v) & 0x7f800000u) != 0x7f800000u; }

template <int BULB, int MODE>
__global__ __launch_bounds__(256, trace_waves(BULB)) void trace_kernel(
    const SceneBlock *__restrict__ sb, const float4 *__restrict__ rays, int numRays, int noNormal, float4 *__restrict__ hits) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= (unsigned)numRays) return;
  const float4 r0 = rays[2 * (size_t)i], r1 = rays[2 * (size_t)i + 1];
  const V3 ro = v3(r0.x, r0.y, r0.z), rd = v3(r1.x, r1.y, r1.z);
  const float tMax = r0.w;
  float4 h0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), h1 = make_float4(0.0f, 0.0f, 0.0f, u2f((uint32_t)RM_RAY_INVALID));
  const bool valid = finiteBits(ro.x) && finiteBits(ro.y) && finiteBits(ro.z) && finiteBits(rd.x) && finiteBits(rd.y) &&
                     finiteBits(rd.z) && (rd.x != 0.0f || rd.y != 0.0f || rd.z != 0.0f) && tMax >= 0.0f;  // NaN >= 0 is false
  if (!valid) {
    hits[2 * (size_t)i] = h0;
    hits[2 * (size_t)i + 1] = h1;
    return;
  }
  Counters cnt{0, 0, 0, 0, 0, 0};
  if (MODE == kTraceOcclusion) {
    const MarchRes res = march<BULB, 0, kShadow | kCull>(sb, ro, rd, tMax, 1.0f, cnt);  // softshadow(ro, rd, 0, tMax, 8)
    h0.w = res.d;
    h1.w = u2f((uint32_t)res.obj);
  } else {
    const MarchRes res = march<BULB, 0, kCull>(sb, ro, rd, tMax, 1.0f, cnt);  // a miss reports tMax, not res.d
    h0.w = tMax;
    h1.w = u2f((uint32_t)res.obj);
    if (res.obj != -1) {
      h0.w = res.d;
      if (!noNormal) {  // wave-uniform
        const V3 p = madd(rd, res.d, ro);
        // render()'s seeds of the skip test: an upper bound of sdScene at p, then at the normal's taps
        constexpr bool SKIP = !BULB;
        float ubP = __builtin_inff();
        if (SKIP) {
          const float lipLen = (sb->cullLip * len(rd)) * 1.0001f;
          ubP = fma(kSurfaceDist, lipLen, kSurfaceDist) * 1.001f + fma(fabs_(res.d), 1.0e-6f, 1.0e-5f);
        }
        V3 n = getNormal<BULB, 0, optIf(SKIP, kSkip)>(sb, p, cnt, SKIP ? fma(0.0005f, sb->cullLip * 1.001f, ubP) : ubP);
        if (sb->s.features & RM_FEAT_PERLIN_BUMP) n = bumpNormal(n, p);
        h0.x = n.x; h0.y = n.y; h0.z = n.z;
        h1.x = p.x; h1.y = p.y; h1.z = p.z;
      }
    }
  }
  hits[2 * (size_t)i] = h0;
  hits[2 * (size_t)i + 1] = h1;
}

// The three march classes (dispatch_march_class, rm_internal.h) × closest / occlusion, and nothing more.
template <int MODE>
static void launch_trace_mode(const SceneBlock *sb, int bulbClass, dim3 grid, const float4 *rays, int numRays, int noNormal,
                              float4 *hits, hipStream_t stream) {
  const dim3 block(256);
  dispatch_march_class(bulbClass, [&](auto c) {
    hipLaunchKernelGGL((trace_kernel<decltype(c)::bulb, MODE>), grid, block, 0, stream, sb, rays, numRays, noNormal, hits);
  });
}
int launch_trace_kernel(const void *sbv, int bulbClass, bool occlusion, bool noNormal, const void *d_rays, int numRays, void *d_hits,
                        hipStream_t stream) {
  static_assert(sizeof(RmRay) == 2 * sizeof(float4) && sizeof(RmRayHit) == 2 * sizeof(float4), "a ray and a hit are two float4 each");
  const SceneBlock *sb = static_cast<const SceneBlock *>(sbv);
  const float4 *rays = static_cast<const float4 *>(d_rays);
  float4 *hits = static_cast<float4 *>(d_hits);
  const dim3 grid((unsigned)(((long long)numRays + 255) / 256));
  if (occlusion) launch_trace_mode<kTraceOcclusion>(sb, bulbClass, grid, rays, numRays, 0, hits, stream);
  else launch_trace_mode<kTraceClosest>(sb, bulbClass, grid, rays, numRays, noNormal ? 1 : 0, hits, stream);
  HIP_OK(hipGetLastError());
  return RM_OK;
}

}  // namespace rm
