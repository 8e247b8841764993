// rm_light_probes.hip — the kernels of rm_light_probes (gfx950 only): SH9 radiance probes, shaded and reduced in one launch.  The
// ray of a (probe, table row) pair is built in the kernel, everything behind it is the render kernels' own device code (shadeRay,
// rm_device.hip.h), and what comes back — a colour and the hit flag — is multiplied into the row's nine basis values and summed over
// the probe's rows by the fixed pairwise tree of rm_light_probes.h.  The launcher (argument checks, staging, the class of the call)
// is launch_probes in rm_queries.hip; the kernels live here so that adding them leaves the code objects of the existing kernels as
// they were.
#include <hip/hip_runtime.h>

#include <climits>

#include "rm_device.hip.h"
#include "rm_internal.h"
#include "rm_light_probes.h"

namespace rm {

static_assert(sizeof(lp::Row) == 64 && sizeof(RmProbeDir) == 64, "four float4 per table row");
static_assert(sizeof(lp::Probe) == 160 && sizeof(RmLightProbe) == 160, "ten float4 per record");
static_assert(lp::kMaxDirs == RM_MAX_PROBE_DIRS && RM_MAX_PROBE_DIRS == 1 << lp::kMaxLevels, "rm_light_probes.h has the header's limit");
static_assert(lp::kInvalid == RM_RAY_INVALID, "the header's code");
constexpr int kProbePassLevels = 4;  // log2(RM_MAX_PROBE_DIRS / 64): the pending sums above the passes of one probe
static_assert(RM_MAX_PROBE_DIRS == 64 << kProbePassLevels, "sixteen passes of 64 at the most");

// rm_light_probes: (probe, direction) pairs flattened over lanes as field_ambient_kernel (rm_field.hip) has them, lane % numDirs
// the row.  With numDirs <= 64 a wave holds 64 / numDirs probes, a SEGMENT of numDirs lanes each; with more (MULTI) a wave makes
// numDirs / 64 passes over one probe.  The workgroup opens as shade_rays_kernel does — stageWorkgroup, one barrier — and only BEHIND
// that barrier does a wave whose first probe is past the end leave, as a whole.  In a live wave the lanes of probes past the end,
// of probes with a non-finite position and of rows with an invalid direction must not enter shadeRay — the bulb classes' shadow
// pool counts the lanes that are there, as it does for shade_rays_kernel's absent lanes — but every lane must reach the fold: the
// call stands under `if (valid)`, nothing returns early.  A lane loads its row's direction (one float4) ahead of the ray and the
// nine basis values (three float4) behind it, so that they are not alive across shadeRay; the table, up to 256 KB, stays in global
// memory.  The fold is an xor butterfly over the 36 words of the leaf and the hit count: at level l lane j adds lane j ^ 2^l, the
// tree's s[2m] + s[2m + 1] or the same two operands the other way round, the same word, so every lane of a segment ends with the
// segment's sums.  MULTI: the 64-leaf sums of the passes join in leaf order by lp::fold_in_order, whose pending sums — 36 words on
// each of 4 levels per wave — wait in LDS, not in registers across shadeRay: lane 0 writes them, every lane reads them back
// (a broadcast), the wave's own order of LDS operations between.  Segment lane 0 stores the record as ten 16-byte stores; a probe
// with a non-finite position stores zeros and RM_RAY_INVALID.
// COUNT = 0, SPLIT = 0, far = sb->cam.initialFar, a frame width of 1 for envLayers: as shade_rays_kernel.  Register budget:
// render_waves of the class, which is shade_waves' ladder (DESIGN §6.25 has the compiler's report per instantiation).
// -ffp-contract=off.
constexpr int kProbeEnvWidth = 1;  // envLayers' frame width: compiled, never reached

template <int BULB, bool ENV, bool TEX, bool SEC, bool MULTI>
__global__ __launch_bounds__(256, render_waves(BULB, ENV, TEX, SEC)) void light_probes_kernel(
    const SceneBlock *__restrict__ sb, const float4 *__restrict__ positions, unsigned numProbes, const float4 *__restrict__ dirs,
    int numDirs, int numSets, float4 *__restrict__ out) {
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
          V4 col, br;
          Counters cnt{0, 0, 0, 0, 0, 0};
          shadeRay<BULB, 0, optClass(ENV, TEX, SEC)>(sb, s_objs, v3(p[0], p[1], p[2]), v3(d[0], d[1], d[2]), kProbeEnvWidth, col, br, cnt, hit);
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
      // every lane holds the pass's sums; the pending ones are the wave's, in LDS: lane 0 leaves them, every lane reads them back
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
int launch_probes_kernel(const void *sbv, int bulbClass, bool env, bool tex, bool sec, const float *d_positions, int numProbes,
                         const void *d_dirs, int numDirs, int numSets, void *d_out, hipStream_t stream) {
  const SceneBlock *sb = static_cast<const SceneBlock *>(sbv);
  const float4 *pos = reinterpret_cast<const float4 *>(d_positions), *dirs = static_cast<const float4 *>(d_dirs);
  float4 *o = static_cast<float4 *>(d_out);
  const unsigned perWave = numDirs < 64 ? 64u / (unsigned)numDirs : 1u;
  const unsigned waves = ((unsigned)numProbes + perWave - 1u) / perWave;  // at most 2^31 − 1
  const dim3 grid(waves / 4u + (waves % 4u != 0u ? 1u : 0u)), block(256);
  dispatch_class(bulbClass, env, tex, sec, [&](auto c) {
    using K = decltype(c);
    if (numDirs > 64)
      hipLaunchKernelGGL((light_probes_kernel<K::bulb, K::env, K::tex, K::sec, true>), grid, block, 0, stream, sb, pos, (unsigned)numProbes,
                         dirs, numDirs, numSets, o);
    else
      hipLaunchKernelGGL((light_probes_kernel<K::bulb, K::env, K::tex, K::sec, false>), grid, block, 0, stream, sb, pos, (unsigned)numProbes,
                         dirs, numDirs, numSets, o);
  });
  HIP_OK(hipGetLastError());
  return RM_OK;
}

}  // namespace rm
