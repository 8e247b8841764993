// rm_layers.hip — the kernels of rm_shade_rays_layers and rm_trace_rays_layers (gfx950 only): ARBITRARY rays through the procedural
// layers — terrain, sea and clouds — as main sends its own rays through them.  The rays come from device memory; everything behind
// the ray is the render kernels' own device code (shadeRay with envLayers in rm_device.hip.h; seaMapHeight, getSeaNormal,
// raymarchTerrain and terrainNormal in rm_env.hip.h).  The launchers (argument checks, staging, the class of the call) are
// launch_shade and launch_trace in rm_queries.hip; the kernels live here so that adding them leaves the code objects
// of the existing kernels as they were.
#include <hip/hip_runtime.h>

#include <climits>

#include "rm_device.hip.h"
#include "rm_internal.h"

namespace rm {

RM_DEV bool finiteBits(float v) { return (f2u(v) & 0x7f800000u) != 0x7f800000u; }
RM_DEV bool validRay(V3 ro, V3 rd) {
  return finiteBits(ro.x) && finiteBits(ro.y) && finiteBits(ro.z) && finiteBits(rd.x) && finiteBits(rd.y) && finiteBits(rd.z) &&
         (rd.x != 0.0f || rd.y != 0.0f || rd.z != 0.0f);
}

// ---- rm_shade_rays_layers ------------------------------------------------------------------------------------------------------
// shade_rays_kernel's body (rm_shade.hip) for the calls that have a layer bit: ENV = true, BULB = 0 (bulb_class is 0 whenever an env
// feature is set), and the width of the image the rays belong to as a kernel argument, handed to shadeRay, where only seaRender's
// normal epsilon reads it (frag:2284-2310).  Lane i = blockIdx.x·256 + threadIdx.x is ray i; the workgroup opens with
// stageWorkgroup<true, TEX> and only BEHIND its barrier do the lanes with i >= numRays and the invalid rays leave.  Two float4 loads
// per ray, one float4 store per output.  far under RM_FEAT_CLOUD is shadePixel's 2000 (frag:2422-2426), not sb->cam.initialFar.
// Register budget (second launch bound): the ENV budgets of render_waves — the device code behind the ray is render_kernel<0, 0,
// true, TEX, SEC>'s, and the compiler's report per instantiation stands beside its twins' in DESIGN §6.15.
// -DRM_SHADE_LAYERS_*_WAVES=n overrides per class.
#ifndef RM_SHADE_LAYERS_ENV_WAVES
#define RM_SHADE_LAYERS_ENV_WAVES RM_ENV_WAVES
#endif
#ifndef RM_SHADE_LAYERS_ENV_NOSEC_WAVES
#define RM_SHADE_LAYERS_ENV_NOSEC_WAVES RM_ENV_NOSEC_WAVES
#endif
#ifndef RM_SHADE_LAYERS_TEX_WAVES
#define RM_SHADE_LAYERS_TEX_WAVES RM_TEX_WAVES
#endif
#ifndef RM_SHADE_LAYERS_TEX_NOSEC_WAVES
#define RM_SHADE_LAYERS_TEX_NOSEC_WAVES RM_TEX_NOSEC_WAVES
#endif
constexpr int shade_layers_waves(bool tex, bool sec) {  // render_waves' ladder for env = true
  if (tex) return sec ? RM_SHADE_LAYERS_TEX_WAVES : RM_SHADE_LAYERS_TEX_NOSEC_WAVES;
  return sec ? RM_SHADE_LAYERS_ENV_WAVES : RM_SHADE_LAYERS_ENV_NOSEC_WAVES;
}

template <bool TEX, bool SEC>
__global__ __launch_bounds__(256, shade_layers_waves(TEX, SEC)) void shade_rays_layers_kernel(
    const SceneBlock *__restrict__ sb, const float4 *__restrict__ rays, int numRays, int imageWidth, float4 *__restrict__ out,
    float4 *__restrict__ bright) {
  __shared__ RmObject s_objs[RM_MAX_OBJECTS];
  stageWorkgroup<true, TEX>(sb, s_objs);
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= (unsigned)numRays) return;
  const float4 r0 = rays[2 * (size_t)i], r1 = rays[2 * (size_t)i + 1];
  const V3 ro = v3(r0.x, r0.y, r0.z), rd = v3(r1.x, r1.y, r1.z);
  if (!validRay(ro, rd)) {  // alpha 0 marks it: a valid ray's alpha is >= 1
    out[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (bright) bright[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    return;
  }
  V4 col, br = v4(0.0f, 0.0f, 0.0f, 1.0f);
  Counters cnt{0, 0, 0, 0, 0, 0};
  bool hit = false;
  shadeRay<0, 0, kEnv | optIf(TEX, kTex) | optIf(SEC, kSec)>(sb, s_objs, ro, rd, imageWidth, col, br, cnt, hit);
  out[i] = make_float4(col.x, col.y, col.z, col.w);
  if (bright) bright[i] = make_float4(br.x, br.y, br.z, br.w);
}

int launch_shade_layers_kernel(const void *sbv, bool tex, bool sec, const void *d_rays, int numRays, int imageWidth, float *d_rgba,
                               float *d_bright, hipStream_t stream) {
  static_assert(sizeof(RmRay) == 2 * sizeof(float4), "a ray is two float4");
  static_assert(((long long)INT_MAX + 255) / 256 <= INT_MAX, "every int numRays fits one grid of 256-lane workgroups");
  const SceneBlock *sb = static_cast<const SceneBlock *>(sbv);
  const float4 *rays = static_cast<const float4 *>(d_rays);
  float4 *o = reinterpret_cast<float4 *>(d_rgba), *b = reinterpret_cast<float4 *>(d_bright);
  const dim3 grid((unsigned)(((long long)numRays + 255) / 256)), block(256);
  if (tex && sec) hipLaunchKernelGGL((shade_rays_layers_kernel<true, true>), grid, block, 0, stream, sb, rays, numRays, imageWidth, o, b);
  else if (tex) hipLaunchKernelGGL((shade_rays_layers_kernel<true, false>), grid, block, 0, stream, sb, rays, numRays, imageWidth, o, b);
  else if (sec) hipLaunchKernelGGL((shade_rays_layers_kernel<false, true>), grid, block, 0, stream, sb, rays, numRays, imageWidth, o, b);
  else hipLaunchKernelGGL((shade_rays_layers_kernel<false, false>), grid, block, 0, stream, sb, rays, numRays, imageWidth, o, b);
  HIP_OK(hipGetLastError());
  return RM_OK;
}

// ---- rm_trace_rays_layers ------------------------------------------------------------------------------------------------------
// The layer surfaces in front of d0 (the object hit's distance, or the ray's tMax), by envLayers' rules: the geometric part of
// seaRender bounded by d0 (frag:2284-2291, 2252-2282), then the geometric part of terrainRender bounded by the sea's distance
// (frag:2128-2135, 2060-2090; tmin = 15).  Terrain wins over sea, as in main (frag:2459-2475).  kind: 0 (neither), RM_HIT_SEA,
// RM_HIT_TERRAIN.  The cloud layer is a volume: it has no closest hit and is not marched.  The terrain's normal is the surface's
// own terrainNormal (frag:2106-2111), not the fbm-perturbed one its lighting builds from it; the sea's is the shader's, its epsilon
// (dot(d, d)·0.1) / imageWidth.  features and noNormal are wave-uniform.  No sampler is read: seaMap is procedural.
struct LayerSurface { int kind; float t; V3 p, n; };
RM_DEV LayerSurface layerSurface(uint32_t features, float iTime, int imageWidth, V3 ro, V3 rd, float d0, bool noNormal, Counters &cnt) {
  LayerSurface s;
  s.kind = 0; s.t = d0; s.p = v3(0.0f, 0.0f, 0.0f); s.n = v3(0.0f, 0.0f, 0.0f);
  V3 ps = v3(0.0f, 0.0f, 0.0f);
  if (features & RM_FEAT_SEA) {
    const float t = seaMapHeight(iTime, ro, rd, ps, d0);
    if (!(len(ps) == 0.0f || t == -1.0f)) { s.kind = RM_HIT_SEA; s.t = t; }
  }
  if (features & RM_FEAT_TERRAIN) {
    const float t = raymarchTerrain(ro, rd, 15.0f, s.t, cnt);
    if (t > 0.0f) { s.kind = RM_HIT_TERRAIN; s.t = t; }
  }
  if (noNormal) return s;
  if (s.kind == RM_HIT_TERRAIN) {
    s.p = madd(rd, s.t, ro);
    s.n = terrainNormal(s.p.x, s.p.z, cnt);
  } else if (s.kind == RM_HIT_SEA) {
    const V3 d = sub(ps, ro);
    s.p = ps;
    s.n = getSeaNormal(iTime, ps, (dot(d, d) * 0.1f) / (float)imageWidth);
  }
  return s;
}

// trace_kernel's closest mode (rm_trace.hip) with the layer surfaces behind its march: lane i is ray i, two float4 in, two float4
// out, no LDS, no barrier, no material, no sampler.  A lone Mandelbulb keeps its bulb march class (trace reads no material, so the
// env features do not change the class as they do for the kernels that shade).  The object's normal taps are made only where
// neither layer won: an object hit stands exactly as trace_kernel stores it, bump included, and a miss as it stores a miss.
// Register budget (second launch bound): rm_trace.hip's rule — the most waves per SIMD at which the compiler's report shows no
// spill (the rows are in DESIGN §6.15).  -DRM_TRACE_LAYERS*_WAVES=n overrides.
#ifndef RM_TRACE_LAYERS_WAVES
#define RM_TRACE_LAYERS_WAVES 7
#endif
#ifndef RM_TRACE_LAYERS_PLAIN_BULB_WAVES
#define RM_TRACE_LAYERS_PLAIN_BULB_WAVES 8
#endif
constexpr int trace_layers_waves(int bulb) { return bulb == kBulbPlain ? RM_TRACE_LAYERS_PLAIN_BULB_WAVES : RM_TRACE_LAYERS_WAVES; }

template <int BULB>
__global__ __launch_bounds__(256, trace_layers_waves(BULB)) void trace_layers_kernel(
    const SceneBlock *__restrict__ sb, const float4 *__restrict__ rays, int numRays, int imageWidth, int noNormal,
    float4 *__restrict__ hits) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= (unsigned)numRays) return;
  const float4 r0 = rays[2 * (size_t)i], r1 = rays[2 * (size_t)i + 1];
  const V3 ro = v3(r0.x, r0.y, r0.z), rd = v3(r1.x, r1.y, r1.z);
  const float tMax = r0.w;
  float4 h0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), h1 = make_float4(0.0f, 0.0f, 0.0f, u2f((uint32_t)RM_RAY_INVALID));
  if (!(validRay(ro, rd) && tMax >= 0.0f)) {  // NaN >= 0 is false
    hits[2 * (size_t)i] = h0;
    hits[2 * (size_t)i + 1] = h1;
    return;
  }
  Counters cnt{0, 0, 0, 0, 0, 0};
  const MarchRes res = march<BULB, 0, kCull>(sb, ro, rd, tMax, 1.0f, cnt);  // a miss reports tMax, not res.d
  const float d0 = res.obj != -1 ? res.d : tMax;
  const LayerSurface ls = layerSurface(sb->s.features, sb->g.iTime, imageWidth, ro, rd, d0, noNormal != 0, cnt);
  h0.w = ls.t;
  if (ls.kind != 0) {
    h1.w = u2f((uint32_t)ls.kind);
    h0.x = ls.n.x; h0.y = ls.n.y; h0.z = ls.n.z;
    h1.x = ls.p.x; h1.y = ls.p.y; h1.z = ls.p.z;
  } else {
    h1.w = u2f((uint32_t)res.obj);
    if (res.obj != -1 && !noNormal) {  // trace_kernel's lines
      const V3 p = madd(rd, res.d, ro);
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
  hits[2 * (size_t)i] = h0;
  hits[2 * (size_t)i + 1] = h1;
}

// The three march classes (dispatch_march_class, rm_internal.h), closest mode only.
int launch_trace_layers_kernel(const void *sbv, int bulbClass, bool noNormal, const void *d_rays, int numRays, int imageWidth,
                               void *d_hits, hipStream_t stream) {
  static_assert(sizeof(RmRay) == 2 * sizeof(float4) && sizeof(RmRayHit) == 2 * sizeof(float4), "a ray and a hit are two float4 each");
  const SceneBlock *sb = static_cast<const SceneBlock *>(sbv);
  const float4 *rays = static_cast<const float4 *>(d_rays);
  float4 *hits = static_cast<float4 *>(d_hits);
  const dim3 grid((unsigned)(((long long)numRays + 255) / 256)), block(256);
  const int nn = noNormal ? 1 : 0;
  dispatch_march_class(bulbClass, [&](auto c) {
    hipLaunchKernelGGL((trace_layers_kernel<decltype(c)::bulb>), grid, block, 0, stream, sb, rays, numRays, imageWidth, nn, hits);
  });
  HIP_OK(hipGetLastError());
  return RM_OK;
}

}  // namespace rm
