// rm_light_probes_indirect.hip — the kernels of rm_light_probes_indirect (gfx950 only): rm_light_probes with every ray's colour
// replaced by rm_shade_rays_indirect's, so that a bake reads the grid of the bake before it — DDGI's further bounces — in ONE launch.
// The kernel is light_probes_kernel (rm_light_probes.hip) with shadeRayIndirect (rm_indirect.hip.h) in shadeRay's place and the grid
// in its arguments: the flattening, the leaves, the xor butterfly, the fold of the passes in LDS and the stores are its own, word
// for word.  The launcher is launch_probes_indirect in rm_queries.hip; a translation unit of its own, so that adding it leaves the
// code objects of the existing kernels — rm_light_probes.hip's among them — as they were.
#include <hip/hip_runtime.h>

#include <climits>

#include "rm_indirect.hip.h"
#include "rm_internal.h"
#include "rm_light_probes.h"

namespace rm {

static_assert(sizeof(lp::Row) == 64 && sizeof(RmProbeDir) == 64, "four float4 per table row");
static_assert(sizeof(lp::Probe) == 160 && sizeof(RmLightProbe) == 160, "ten float4 per record");
constexpr int kProbePassLevels = 4;  // log2(RM_MAX_PROBE_DIRS / 64): the pending sums above the passes of one probe
static_assert(RM_MAX_PROBE_DIRS == 64 << kProbePassLevels, "sixteen passes of 64 at the most");

// light_probes_kernel's text (rm_light_probes.hip has the account of every step): a wave holds 64 / numDirs probes, or with MULTI
// makes numDirs / 64 passes over one; the lanes that have no ray stay out of shadeRayIndirect but reach the fold; the row's
// direction is loaded ahead of the ray and its basis behind it.  The grid's gather happens inside the ray, behind its primary hit.
// Register budget: render_waves of the class, rm_light_probes.hip's rule (DESIGN §6.28 has the compiler's report).
// -ffp-contract=off.
template <int BULB, bool ENV, bool TEX, bool SEC, bool MULTI>
__global__ __launch_bounds__(256, render_waves(BULB, ENV, TEX, SEC)) void light_probes_indirect_kernel(
    const SceneBlock *__restrict__ sb, const float4 *__restrict__ positions, unsigned numProbes, const float4 *__restrict__ dirs,
    int numDirs, int numSets, IndirectGrid grid, float4 *__restrict__ out) {
  __shared__ RmObject s_objs[BULB ? 1 : RM_MAX_OBJECTS];
  __shared__ float s_pending[MULTI ? 4 : 1][MULTI ? kProbePassLevels : 1][MULTI ? lp::kWords : 1];
  stageWorkgroup<ENV, TEX>(sb, s_objs);
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const unsigned seg = MULTI ? 64u : (unsigned)numDirs, perWave = 64u / seg;
  const size_t first = ((size_t)blockIdx.x * 4u + wave) * perWave;  // the wave's first probe
  if (first >= numProbes) return;                                    // wave-uniform, behind the barrier
  const size_t i = first + lane / seg;
  const unsigned k0 = lane & (seg - 1u);
  const bool live = i < numProbes;
  const float4 *set = dirs + 4u * (size_t)((unsigned)i % (unsigned)numSets) * (size_t)numDirs;
  const int passes = MULTI ? numDirs / 64 : 1;
  float s[lp::kWords];
  int hits = 0;
  bool probeOk = false;
#pragma unroll 1
  for (int pass = 0; pass < passes; pass++) {
    const float4 *row = set + 4u * (size_t)(pass * 64 + (int)k0);
    float c[3] = {0.0f, 0.0f, 0.0f};
    bool hit = false;
    if (live) {
      const float4 q = positions[i];
      const float p[3] = {q.x, q.y, q.z};
      probeOk = lp::valid_position(p);
      if (probeOk) {
        const float4 e = row[0];
        const float d[3] = {e.x, e.y, e.z};
        if (lp::valid_direction(d)) {
          V4 col;
          shadeRayIndirect<BULB, optClass(ENV, TEX, SEC)>(sb, s_objs, v3(p[0], p[1], p[2]), v3(d[0], d[1], d[2]), grid, col, hit);
          c[0] = col.x, c[1] = col.y, c[2] = col.z;
        }
      }
    }
    float basis[lp::kBasis] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (probeOk) {
      const float4 b0 = row[1], b1 = row[2], b2 = row[3];
      basis[0] = b0.x, basis[1] = b0.y, basis[2] = b0.z, basis[3] = b0.w;
      basis[4] = b1.x, basis[5] = b1.y, basis[6] = b1.z, basis[7] = b1.w, basis[8] = b2.x;
    }
    lp::ray_leaf(basis, c, hit, s);
    int h = hit ? 1 : 0;
    for (unsigned m = 1u; m < seg; m <<= 1) {
#pragma unroll
      for (int w = 0; w < lp::kWords; w++) s[w] = s[w] + __shfl_xor(s[w], (int)m);
      h += __shfl_xor(h, (int)m);
    }
    hits += h;
    if constexpr (MULTI) {
      float(*pending)[lp::kWords] = s_pending[wave];
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      lp::fold_in_order(pass, passes, s, [&](int level, int w) { return pending[level][w]; },
                        [&](int level, int w, float v) { if (lane == 0u) pending[level][w] = v; });
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
  }
  if (!live || k0 != 0u) return;
  float4 *rec = out + 10u * i;
  if (!probeOk) {
#pragma unroll
    for (int j = 0; j < lp::kBasis; j++) rec[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    rec[9] = make_float4(__int_as_float(RM_RAY_INVALID), 0.0f, 0.0f, 0.0f);
    return;
  }
#pragma unroll
  for (int j = 0; j < lp::kBasis; j++) rec[j] = make_float4(s[4 * j], s[4 * j + 1], s[4 * j + 2], s[4 * j + 3]);
  rec[9] = make_float4(__int_as_float(hits), 0.0f, 0.0f, 0.0f);
}

// The production classes (dispatch_class, rm_internal.h), each in the one-pass form (numDirs <= 64) and in the form that loops.
int launch_probes_indirect_kernel(const void *sbv, int bulbClass, bool env, bool tex, bool sec, const float *d_positions, int numProbes,
                                  const void *d_dirs, int numDirs, int numSets, const IndirectGridArgs &ga, void *d_out,
                                  hipStream_t stream) {
  const SceneBlock *sb = static_cast<const SceneBlock *>(sbv);
  const float4 *pos = reinterpret_cast<const float4 *>(d_positions), *dirs = static_cast<const float4 *>(d_dirs);
  float4 *o = static_cast<float4 *>(d_out);
  const IndirectGrid grid{static_cast<const char *>(ga.d_probes), static_cast<const char *>(ga.d_depth),
                          lg::Grid{{ga.dims[0], ga.dims[1], ga.dims[2]}, {ga.origin[0], ga.origin[1], ga.origin[2]}, {ga.step[0], ga.step[1], ga.step[2]}},
                          ga.k, ga.flags, ga.normalBias};
  const unsigned perWave = numDirs < 64 ? 64u / (unsigned)numDirs : 1u;
  const unsigned waves = ((unsigned)numProbes + perWave - 1u) / perWave;  // at most 2^31 − 1
  const dim3 grd(waves / 4u + (waves % 4u != 0u ? 1u : 0u)), block(256);
  dispatch_class(bulbClass, env, tex, sec, [&](auto c) {
    using K = decltype(c);
    if (numDirs > 64)
      hipLaunchKernelGGL((light_probes_indirect_kernel<K::bulb, K::env, K::tex, K::sec, true>), grd, block, 0, stream, sb, pos,
                         (unsigned)numProbes, dirs, numDirs, numSets, grid, o);
    else
      hipLaunchKernelGGL((light_probes_indirect_kernel<K::bulb, K::env, K::tex, K::sec, false>), grd, block, 0, stream, sb, pos,
                         (unsigned)numProbes, dirs, numDirs, numSets, grid, o);
  });
  HIP_OK(hipGetLastError());
  return RM_OK;
}

}  // namespace rm
