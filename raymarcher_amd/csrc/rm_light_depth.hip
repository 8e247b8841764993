// rm_light_depth.hip — the kernels of rm_light_probes_depth (gfx950 only): the depth moments of light probes, marched and reduced in
// one launch.  The ray of a (probe, table row) pair is built in the kernel and marched by trace_kernel's own call (rm_trace.hip,
// march<BULB, 0, kCull>); its distance and the square of it are multiplied into the row's 64 texel weights and summed over the probe's
// rows by the fixed pairwise tree of rm_light_probes, walked serially by the lane that owns the texel (rm_light_depth.h).  The
// launcher (argument checks, staging, the class of the call) is launch_probes_depth in rm_queries.hip; the kernels live here so that
// adding them leaves the code objects of the existing kernels as they were.
#include <hip/hip_runtime.h>

#include "rm_device.hip.h"
#include "rm_internal.h"
#include "rm_light_depth.h"

namespace rm {

static_assert(sizeof(ld::Depth) == 512 && sizeof(RmProbeDepth) == 512, "64 texels of two moments");
static_assert(ld::kTexels == RM_PROBE_DEPTH_TEXELS && ld::kTexels == 64, "a texel per lane of a wave");

// rm_light_probes_depth.  TWO phases per pass, with two meanings of a lane.
//   March: light_probes_kernel's flattening (rm_light_probes.hip), lane % numDirs the row: with numDirs < 64 a wave holds
// 64 / numDirs probes, a segment of numDirs lanes each; from 64 on (MULTI) a wave makes numDirs / 64 passes over one probe — one
// pass at 64, which takes this form for its texel phase: 64 rows known to the compiler, their weights loaded ahead.  The march
// is trace_kernel's closest-hit call with tMax = maxDistance, under trace_kernel's rule for the lanes that must not enter it — a
// probe past the end, a non-finite position, an invalid direction: the march's wave-wide decisions are proofs about the lanes that
// ARE there, so the call stands under `if` and a ray's distance does not depend on the rays it shares a wave with.  No material is
// read: no object table in LDS, no workgroup barrier.  A wave whose first probe is past the end leaves as a whole.
//   Texels: the lane leaves (r, r·r) of its ray in the wave's 512 bytes of LDS — the wave's own order of LDS operations between,
// no barrier of the workgroup — and BECOMES texel x = lane.  It reads row k's weight on its texel, a coalesced 256-byte line per
// row for the wave, and the row's pair as one LDS broadcast, forms the two leaves and folds the segment's leaves in tree order by
// itself (ld::texel_sums, pending sums of six levels in registers): no shuffle.  With numDirs < 64 that runs once per probe the
// wave holds, over the complete subtree of numDirs leaves that is the probe's whole tree.  MULTI: the 64-leaf sums of the passes
// join by ld::fold_in_order, whose pending sums — two words on four levels per lane — wait in LDS at a slot per lane, not in
// registers across the march.  A record is 64 eight-byte stores of one wave, 512 contiguous bytes; a probe with a non-finite
// position stores zeros.  The weights, up to 1 MB, stay in global memory: every wave of a set reads the same lines.
// Register budget (second launch bound): rm_trace.hip's rule, the most waves per SIMD at which the compiler's report shows no
// spill; DESIGN §6.27 has the report per instantiation.  -DRM_DEPTH*_WAVES=n overrides.  -ffp-contract=off.
#ifndef RM_DEPTH_WAVES
#define RM_DEPTH_WAVES 7
#endif
#ifndef RM_DEPTH_PLAIN_BULB_WAVES
#define RM_DEPTH_PLAIN_BULB_WAVES 8
#endif
#ifndef RM_DEPTH_TABLE_MULTI_WAVES
#define RM_DEPTH_TABLE_MULTI_WAVES 6  // the table walk on whole waves per probe: at 7 the report shows spills and scratch
#endif
constexpr int depth_waves(int bulb, bool multi) {
  return bulb == kBulbPlain ? RM_DEPTH_PLAIN_BULB_WAVES : bulb == 0 && multi ? RM_DEPTH_TABLE_MULTI_WAVES : RM_DEPTH_WAVES;
}

template <int BULB, bool MULTI>
__global__ __launch_bounds__(256, depth_waves(BULB, MULTI)) void light_depth_kernel(
    const SceneBlock *__restrict__ sb, const float4 *__restrict__ positions, unsigned numProbes, const float4 *__restrict__ dirs,
    const float *__restrict__ weights, int numDirs, int numSets, float maxDistance, float2 *__restrict__ out) {
  __shared__ float2 s_ray[4][64];
  __shared__ float s_join[MULTI ? ld::kJoinLevels : 1][2][MULTI ? 256 : 1];
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const unsigned seg = MULTI ? 64u : (unsigned)numDirs, perWave = 64u / seg;
  const size_t first = ((size_t)blockIdx.x * 4u + wave) * perWave;  // the wave's first probe
  if (first >= numProbes) return;                                    // wave-uniform; the kernel has no workgroup barrier
  const size_t i = first + lane / seg;
  const unsigned k0 = lane & (seg - 1u);
  bool marches = i < numProbes;
  float p[3] = {0.0f, 0.0f, 0.0f};
  if (marches) {
    const float4 q = positions[i];
    p[0] = q.x, p[1] = q.y, p[2] = q.z;
    marches = lp::valid_position(p);
  }
  const float4 *set = dirs + 4u * (size_t)((unsigned)i % (unsigned)numSets) * (size_t)numDirs;
  const int passes = MULTI ? numDirs / 64 : 1;
  float2 *ray = s_ray[wave];
  float s[2] = {0.0f, 0.0f};
#pragma unroll 1
  for (int pass = 0; pass < passes; pass++) {
    float r = 0.0f;
    if (marches) {
      const float4 e = set[4u * (size_t)(pass * 64 + (int)k0)];
      const float d[3] = {e.x, e.y, e.z};
      if (lp::valid_direction(d)) {
        Counters cnt{0, 0, 0, 0, 0, 0};
        const MarchRes res = march<BULB, 0, kCull>(sb, v3(p[0], p[1], p[2]), v3(d[0], d[1], d[2]), maxDistance, 1.0f, cnt);
        r = res.obj != -1 ? res.d : maxDistance;  // rm_trace_rays' t: a miss reports tMax
      }
    }
    float m[2];
    ld::ray_moments(r, m);
    ray[lane] = make_float2(m[0], m[1]);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // from here on the lane is texel `lane`
    if constexpr (MULTI) {
      if (marches) {  // one probe per wave: uniform
        const float *w = weights + ((size_t)((unsigned)first % (unsigned)numSets) * (size_t)numDirs + (size_t)pass * 64u) * 64u + lane;
        ld::texel_sums_pass([&](int k) { return w[(size_t)k * 64u]; },
                            [&](int k, float v[2]) { const float2 t = ray[k]; v[0] = t.x, v[1] = t.y; }, s);
        ld::fold_in_order(pass, passes, s, [&](int level, int word) { return s_join[level][word][threadIdx.x]; },
                          [&](int level, int word, float v) { s_join[level][word][threadIdx.x] = v; });
      }
    } else {
      for (unsigned j = 0; j < perWave; j++) {
        const size_t probe = first + j;
        if (probe >= numProbes) break;
        // whether probe j marched: its segment's first lane knows, the texel lanes ask the position again (one line, uniform)
        const float4 q = positions[probe];
        const float pj[3] = {q.x, q.y, q.z};
        float2 rec = make_float2(0.0f, 0.0f);
        if (lp::valid_position(pj)) {
          const float *w = weights + (size_t)((unsigned)probe % (unsigned)numSets) * (size_t)numDirs * 64u + lane;
          const float2 *rj = ray + j * seg;
          const auto weight = [&](int k) { return w[(size_t)k * 64u]; };
          const auto pair = [&](int k, float v[2]) { const float2 t = rj[k]; v[0] = t.x, v[1] = t.y; };
          ld::texel_sums((int)seg, weight, pair, s);
          rec = make_float2(s[0], s[1]);
        }
        out[probe * 64u + lane] = rec;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // the next pass writes `ray` again
    __builtin_amdgcn_wave_barrier();
  }
  if constexpr (MULTI) out[first * 64u + lane] = marches ? make_float2(s[0], s[1]) : make_float2(0.0f, 0.0f);
}

// The three march classes (dispatch_march_class, rm_internal.h), each in the form of several probes per wave (numDirs < 64) and in
// the form of whole waves per probe, which loops over passes.
int launch_probes_depth_kernel(const void *sbv, int bulbClass, const float *d_positions, int numProbes, const void *d_dirs,
                               const float *d_weights, int numDirs, int numSets, float maxDistance, void *d_out, hipStream_t stream) {
  const SceneBlock *sb = static_cast<const SceneBlock *>(sbv);
  const float4 *pos = reinterpret_cast<const float4 *>(d_positions), *dirs = static_cast<const float4 *>(d_dirs);
  float2 *o = static_cast<float2 *>(d_out);
  const unsigned perWave = numDirs < 64 ? 64u / (unsigned)numDirs : 1u;
  const unsigned waves = ((unsigned)numProbes + perWave - 1u) / perWave;  // at most 2^31 − 1
  const dim3 grid(waves / 4u + (waves % 4u != 0u ? 1u : 0u)), block(256);
  dispatch_march_class(bulbClass, [&](auto c) {
    using K = decltype(c);
    if (numDirs >= 64)
      hipLaunchKernelGGL((light_depth_kernel<K::bulb, true>), grid, block, 0, stream, sb, pos, (unsigned)numProbes, dirs, d_weights, numDirs,
                         numSets, maxDistance, o);
    else
      hipLaunchKernelGGL((light_depth_kernel<K::bulb, false>), grid, block, 0, stream, sb, pos, (unsigned)numProbes, dirs, d_weights, numDirs,
                         numSets, maxDistance, o);
  });
  HIP_OK(hipGetLastError());
  return RM_OK;
}

}  // namespace rm
