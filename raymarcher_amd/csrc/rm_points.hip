// rm_points.hip — the kernels of rm_shade_points (gfx950 only): what the renderer thinks of POINTS the caller already has — the
// scene's distance and object at the point, its normal, its ambient occlusion and its shaded colour — with the point optionally
// projected onto the iso-surface first.  Everything behind the point is the render kernels' own device code (rm_device.hip.h).  The
// launcher (argument checks, staging, the class of the call) is launch_points in rm_queries.hip; the kernels live here so that
// adding them leaves the code objects of the existing kernels as they were.
#include <hip/hip_runtime.h>

#include <climits>

#include "rm_device.hip.h"
#include "rm_internal.h"

namespace rm {

// rm_shade_points: lane i = blockIdx.x·256 + threadIdx.x is point i of the call; every point reads the ONE scene block sb (the
// header has the definition).  The workgroup opens as shade_rays_kernel does — stageWorkgroup, and only BEHIND its barrier do the
// lanes with i >= numPoints and the invalid points leave (an invalid point after storing its zeros) — for the same reason: the
// bulb classes' shadow pool is called by every lane of the wave that is still there, converged.
// One loop serves the projection and the final evaluation: each trip evaluates sdScene at p in the primary march's trap form
// (sdSceneImpl<BULB, 0, kTrapShader>: UB3, the trap of the last fractal evaluated) and, with an object there, getNormal(p); a trip that is a
// projection step then moves p, and the trip that stops — the steps are used up, the table is empty, q is not finite or too far from
// p0 — leaves the loop with sc and N belonging to the last accepted p, which is what steps 3 and 4 of the definition ask for.  So
// the kernel holds one copy of the evaluator and one of the normal: 1 + 4 evaluations, plus 5 per projection step.
// The table walk takes render()'s pass-over test (SKIP) for the taps, AO and shadow rays.  render seeds its bound from the march's
// stopping rule; here the value at p is known, so the seed is sc.d itself, padded for the rounding of the tap positions and of the
// values as nextMinBound pads: the bits are the same either way.
// Shading (d_rgba): render() from behind its march.  The bulb classes with hard shadows from directional lights only take the wave's
// shadow pool (renderPooled's three phases: surface, pool, light sum), every other frame getPhong.  Lanes without an object
// (objectId −1) stay for the pool with no ray to march.
// Which outputs exist is a kernel argument (null pointers): launch-uniform branches.  -ffp-contract=off, like every kernel here.
// Register budget (second launch bound): render_waves of the class without secondary rays, shade_rays_kernel's budgets — the device
// code behind the point is a subset of what is behind its ray; the compiler's report per instantiation is in DESIGN §6.17.
// -DRM_POINTS_POOL=0 builds the bulb classes with getPhong's per-lane queue instead of the pool (the measurement of DESIGN §6.17).
#ifndef RM_POINTS_POOL
#define RM_POINTS_POOL 1
#endif
RM_DEV bool finiteBits(float v) { return (f2u(v) & 0x7f800000u) != 0x7f800000u; }

struct PointsArgs {
  const float4 *points, *view;  // view may be null
  int numPoints, projectSteps;
  float iso, maxMove;
  float4 *surface;  // two per point (normal, distance | position, objectId); may be null
  float *ao;        // may be null
  float4 *rgba;     // may be null
};

template <int BULB, bool TEX>
__global__ __launch_bounds__(256, render_waves(BULB, false, TEX, false)) void shade_points_kernel(const SceneBlock *__restrict__ sb,
                                                                                                 const PointsArgs a) {
  __shared__ RmObject s_objs[BULB ? 1 : RM_MAX_OBJECTS];
  stageWorkgroup<false, TEX>(sb, s_objs);
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= (unsigned)a.numPoints) return;
  const float4 pt = a.points[i];
  V3 p = v3(pt.x, pt.y, pt.z), rd = v3(0.0f, 0.0f, 0.0f);
  bool valid = finiteBits(p.x) && finiteBits(p.y) && finiteBits(p.z);
  if (a.view) {
    const float4 vw = a.view[i];
    rd = v3(vw.x, vw.y, vw.z);
    valid = valid && finiteBits(rd.x) && finiteBits(rd.y) && finiteBits(rd.z) && (rd.x != 0.0f || rd.y != 0.0f || rd.z != 0.0f);
  }
  if (!valid) {
    if (a.surface) {
      a.surface[2 * (size_t)i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      a.surface[2 * (size_t)i + 1] = make_float4(0.0f, 0.0f, 0.0f, u2f((uint32_t)RM_RAY_INVALID));
    }
    if (a.ao) a.ao[i] = 0.0f;
    if (a.rgba) a.rgba[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    return;
  }
  Counters cnt{0, 0, 0, 0, 0, 0};
  constexpr bool SKIP = !BULB;
  const float far = sb->cam.initialFar, move2 = a.maxMove * a.maxMove;
  const V3 p0 = p;
  SceneMin sc;
  V3 N = v3(0.0f, 0.0f, 0.0f);
  float ubP = __builtin_inff();
  for (int k = 0;; k++) {
    float unused;
    sc = sdSceneImpl<BULB, 0, kTrapShader>(sb, p, cnt, __builtin_inff(), unused);
    if (sc.idx == -1) {  // no object here: whatever normal an earlier trip left is not this point's
      N = v3(0.0f, 0.0f, 0.0f);
      break;
    }
    if (SKIP) {
      const float pm = max_(max_(fabs_(p.x), fabs_(p.y)), fabs_(p.z));
      ubP = fma(fabs_(sc.d), 1.0e-4f, sc.d) + fma(pm, sb->cullLip * 1.0e-6f, 1.0e-5f);
    }
    N = getNormal<BULB, 0, optIf(SKIP, kSkip)>(sb, p, cnt, SKIP ? fma(0.0005f, sb->cullLip * 1.001f, ubP) : ubP);  // never bumped here
    if (k >= a.projectSteps) break;
    const V3 q = madd(N, -(sc.d - a.iso), p);
    if (!(finiteBits(q.x) && finiteBits(q.y) && finiteBits(q.z))) break;
    const V3 m = sub(q, p0);
    if (!(dot(m, m) <= move2)) break;
    p = q;
  }
  const bool surf = sc.idx != -1;
  if (surf && (sb->s.features & RM_FEAT_PERLIN_BUMP)) N = bumpNormalShared(N, p);
  if (a.surface) {
    a.surface[2 * (size_t)i] = make_float4(N.x, N.y, N.z, sc.d);
    a.surface[2 * (size_t)i + 1] = make_float4(p.x, p.y, p.z, u2f((uint32_t)sc.idx));
  }
  float ao = 0.0f;
  if (a.ao) {
    if (surf) ao = calcAO<BULB, 0, optIf(SKIP, kSkip)>(sb, p, N, cnt, ubP);
    a.ao[i] = ao;
  }
  if (!a.rgba) return;
  if (!a.view) rd = neg(N);  // the point seen head-on
  V4 col = v4(0.0f, 0.0f, 0.0f, 0.0f);
  if (BULB && RM_POINTS_POOL && hardDirectionalOnly(sb)) {  // wave-uniform: renderPooled's phases
    const int nl = sb->numLights;
    V3 so = v3(0.0f, 0.0f, 0.0f);
    float aoT = 1.0f, dStart = -1.0f;
    uint32_t pend = 0u, hits = 0u;
    if (surf) {
      if (sb->s.enableAmbientOcclusion) aoT = a.ao ? ao : calcAO<BULB, 0>(sb, p, N, cnt);
      so = shadowOrigin(p, N);
      bool shared = f2u(so.x) != 0x80000000u && f2u(so.y) != 0x80000000u && f2u(so.z) != 0x80000000u;
      uint32_t need = 0u;
      for (int l = 0; l < nl; l++) {
        const V3 L = preparedL(sb, l);  // lightSetup's normalize(−dir), from the host (SceneBlock::lightPrep)
        shared = shared && (fabs_(L.x) + fabs_(L.y) + fabs_(L.z) <= 2.0f);  // false for a NaN / inf direction
        if (!(dot(N, L) <= 0.005f)) need |= 1u << l;
      }
      const int maxSteps = sb->s.maxSteps;
      if (need != 0u && maxSteps > 0) {
        if (!shared) {
          pend = need;
        } else {
          const float d0 = fabs_(sdScene<BULB, 0, kTrapNone>(sb, so, cnt).d);
          if (d0 < kSurfaceDist) hits = need;
          else if (maxSteps > 1) { pend = need; dStart = d0; }
        }
      }
    }
    const uint32_t hitMask = hits | shadowPool<BULB, 0, kPrep>(sb, so, pend, dStart, far, cnt);
    if (surf) {
      const RmObject &o = s_objs[0];
      Material mat;
      mat.amb = v3(o.cAmbient[0], o.cAmbient[1], o.cAmbient[2]);
      mat.dif = getDiffuse<false>(sb, o, p);
      mat.spec = v3(o.cSpecular[0], o.cSpecular[1], o.cSpecular[2]);
      mat.shininess = o.shininess;
      const float ka = sb->g.ka, ks = sb->g.ks;
      const V3 total = v3((mat.amb.x * ka) * aoT, (mat.amb.y * ka) * aoT, (mat.amb.z * ka) * aoT);
      const V3 ph = hardLightSum<true>(sb, mat, N, v3(0.0f, 0.0f, 0.0f), normalize(neg(rd)), far, ks, hitMask, total);
      const V3 c = bulbTrapColor(sc.trap.y, sc.trap.z, sc.trap.w);
      col = v4(c.x * (ph.x * 8.0f), c.y * (ph.y * 8.0f), c.z * (ph.z * 8.0f), 1.0f);
    }
  } else if (surf) {  // render(), frag:2337-2375
    const RmObject &o = s_objs[BULB ? 0 : sc.idx];
    if (TEX && o.isEmissive) {
      col = v4(o.color[0], o.color[1], o.color[2], 1.0f);
    } else {
      Material mat;
      mat.amb = v3(o.cAmbient[0], o.cAmbient[1], o.cAmbient[2]);
      mat.dif = getDiffuse<TEX>(sb, o, p);
      mat.spec = v3(o.cSpecular[0], o.cSpecular[1], o.cSpecular[2]);
      mat.shininess = o.shininess;
      const int type = BULB ? (int)RM_MANDELBULB : o.type;
      const V3 ph = getPhong<BULB, 0, optIf(TEX, kRes) | kCull>(sb, s_objs, mat, N, p, rd, far, cnt, ubP);
      V3 c3 = ph;
      if (type == RM_MANDELBULB) {
        const V3 c = bulbTrapColor(sc.trap.y, sc.trap.z, sc.trap.w);
        c3 = v3(c.x * (ph.x * 8.0f), c.y * (ph.y * 8.0f), c.z * (ph.z * 8.0f));
      } else if (type == RM_MENGERSPONGE) {
        const V3 c = v3(fma(0.5f, cos_(fma(2.0f, sc.trap.z, 0.0f)), 0.5f), fma(0.5f, cos_(fma(2.0f, sc.trap.z, 1.0f)), 0.5f),
                        fma(0.5f, cos_(fma(2.0f, sc.trap.z, 2.0f)), 0.5f));
        c3 = mul(c, ph);
      }
      col = v4(c3.x, c3.y, c3.z, 1.0f);
    }
  }
  a.rgba[i] = make_float4(col.x, col.y, col.z, col.w);
}

// The four classes a point can have (dispatch_class with env = false, sec = false): table walk, general bulb, plain bulb, samplers.
int launch_points_kernel(const void *sbv, int bulbClass, bool tex, const float *d_points, const float *d_view, int numPoints,
                         int projectSteps, float iso, float maxMove, void *d_surface, float *d_ao, float *d_rgba,
                         hipStream_t stream) {
  static_assert(sizeof(RmSurfacePoint) == 2 * sizeof(float4), "a surface point is two float4");
  static_assert(((long long)INT_MAX + 255) / 256 <= INT_MAX, "every int numPoints fits one grid of 256-lane workgroups");
  const SceneBlock *sb = static_cast<const SceneBlock *>(sbv);
  const PointsArgs a{reinterpret_cast<const float4 *>(d_points), reinterpret_cast<const float4 *>(d_view), numPoints, projectSteps,
                     iso, maxMove, static_cast<float4 *>(d_surface), d_ao, reinterpret_cast<float4 *>(d_rgba)};
  const dim3 grid((unsigned)(((long long)numPoints + 255) / 256)), block(256);
  dispatch_class(bulbClass, false, tex, false, [&](auto c) {
    using K = decltype(c);
    hipLaunchKernelGGL((shade_points_kernel<K::bulb, K::tex>), grid, block, 0, stream, sb, a);
  });
  HIP_OK(hipGetLastError());
  return RM_OK;
}

}  // namespace rm
