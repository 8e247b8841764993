// rm_light_grid_visible.hip — rm_light_grid_irradiance_visible (gfx950 only): rm_light_grid_irradiance with a Chebyshev visibility
// term per corner from rm_light_probes_depth's records, ONE launch, one lane per point.  The arithmetic is rm_light_grid.h's
// grid_light_visible, the very code of the host program of tests/light_depth_spec; the kernel here only loads, calls it and stores.
// Like rm_light_grid_irradiance the entry is no render launch: it stages no scene block, records no path and no timing, touches no
// tuner or workspace state and allocates nothing.  A translation unit of its own, so that adding it leaves the code objects of the
// existing kernels — rm_light_grid.hip's among them — as they were.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "rm_internal.h"
#include "rm_lattice.h"
#include "rm_light_grid.h"

namespace rm {

static_assert(sizeof(RmProbeDepth) == 512 && RM_PROBE_DEPTH_TEXELS == lg::kDepthSide * lg::kDepthSide, "an 8×8 map of two moments");
static_assert(sizeof(RmLightProbe) == 160 && offsetof(RmLightProbe, hits) == 144, "ten float4 per probe, hits in the last");
static_assert(lg::kVisFloor == RM_LIGHT_GRID_VIS_FLOOR, "the header's floor");

// The two records of a probe where the bakes stored them: 160 and 512 bytes each, byte offsets in 64 bits.  hits is one dword, a
// coefficient one 16-byte load, a texel's two moments one 8-byte load.
struct VisibleRecords {
  const char *probes, *depths;
  __host__ __device__ int hits(size_t i) const { return *reinterpret_cast<const int32_t *>(probes + i * sizeof(RmLightProbe) + offsetof(RmLightProbe, hits)); }
  __host__ __device__ void sh(size_t i, int j, float out[4]) const {
    const float4 v = *reinterpret_cast<const float4 *>(probes + i * sizeof(RmLightProbe) + 16u * (size_t)j);
    out[0] = v.x, out[1] = v.y, out[2] = v.z, out[3] = v.w;
  }
  __host__ __device__ void depth(size_t i, int texel, float out[2]) const {
    const float2 v = *reinterpret_cast<const float2 *>(depths + i * sizeof(RmProbeDepth) + 8u * (size_t)texel);
    out[0] = v.x, out[1] = v.y;
  }
};

// One lane per point, as light_grid_kernel: on top of its loads a lane reads four texels — two pairs of neighbours, 16 contiguous
// bytes each — of every valid corner that is not at the biased point itself, 256 B more per point at the most, from up to eight
// 512-byte records.  Never a word of an invalid probe's sh or depth.  -ffp-contract=off.
__global__ __launch_bounds__(256) void light_grid_visible_kernel(VisibleRecords records, lg::Grid G, const float4 *__restrict__ points,
                                                                 const float4 *__restrict__ normals, unsigned n, unsigned flags,
                                                                 float normalBias, float4 *__restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const float4 q = points[i], m = normals[i];
  const float p[3] = {q.x, q.y, q.z}, nrm[3] = {m.x, m.y, m.z};
  const lg::GridLight r = lg::grid_light_visible(G, p, nrm, flags, normalBias, records);
  out[2 * i] = make_float4(r.e[0], r.e[1], r.e[2], r.e[3]);
  out[2 * i + 1] = make_float4(r.weight, __int_as_float(r.probes), 0.0f, 0.0f);
}

namespace {
using fchk::aligned;
using fchk::bad;

// In the header's order — rm_light_grid_irradiance's with d_depth beside d_probes and normalBias behind the step; no HIP call
// before the last.  RM_OK with *launch = false: a call of no point.
int check_light_grid_visible(const RmLightProbe *d_probes, const RmProbeDepth *d_depth, const int *dims, const float *origin,
                             const float *step, const float *d_points, const float *d_normals, int numPoints, uint32_t flags,
                             float normalBias, const RmGridLight *d_out, bool *launch) {
  *launch = false;
  if (numPoints < 0) return bad("negative numPoints");
  if (!dims || !origin || !step) return bad("null dims, origin or step");
  for (int a = 0; a < 3; a++)
    if (dims[a] < 2 || dims[a] > RM_MAX_LIGHT_GRID_DIM) return bad("grid dimension must be 2 … RM_MAX_LIGHT_GRID_DIM (1024)");
  if ((long long)dims[0] * dims[1] * dims[2] > RM_MAX_LIGHT_GRID_PROBES) return bad("more than RM_MAX_LIGHT_GRID_PROBES (2^24) probes");
  for (int a = 0; a < 3; a++)
    if (!std::isfinite(origin[a])) return bad("origin must be finite");
  for (int a = 0; a < 3; a++)
    if (!std::isfinite(step[a]) || !(step[a] > 0.0f)) return bad("step must be finite and greater than 0");
  if (!std::isfinite(normalBias)) return bad("normalBias must be finite");
  if (flags & ~RM_LIGHT_GRID_FACING) return bad("flag bits other than RM_LIGHT_GRID_FACING");
  if (numPoints == 0) return RM_OK;
  if (!d_probes || !d_depth || !d_points || !d_normals || !d_out) return bad("null d_probes, d_depth, d_points, d_normals or d_out");
  if (!aligned(d_probes, 16) || !aligned(d_depth, 16) || !aligned(d_points, 16) || !aligned(d_normals, 16) || !aligned(d_out, 16))
    return bad("d_probes, d_depth, d_points, d_normals and d_out must be 16-byte aligned");
  if (int st = require_device_pointers(
          {{"d_probes", d_probes}, {"d_depth", d_depth}, {"d_points", d_points}, {"d_normals", d_normals}, {"d_out", d_out}}))
    return st;
  *launch = true;
  return RM_OK;
}
}  // namespace

}  // namespace rm

using namespace rm;

extern "C" int rm_light_grid_irradiance_visible(const RmLightProbe *d_probes, const RmProbeDepth *d_depth, const int dims[3],
                                                const float origin[3], const float step[3], const float *d_points, const float *d_normals,
                                                int numPoints, uint32_t flags, float normalBias, RmGridLight *d_out, void *stream) {
  bool launch = false;
  if (int st = check_light_grid_visible(d_probes, d_depth, dims, origin, step, d_points, d_normals, numPoints, flags, normalBias, d_out, &launch))
    return st;
  if (!launch) return RM_OK;
  const lg::Grid G{{dims[0], dims[1], dims[2]}, {origin[0], origin[1], origin[2]}, {step[0], step[1], step[2]}};
  const dim3 grid(((unsigned)numPoints + 255u) / 256u), block(256);  // at most 2^23 workgroups
  hipLaunchKernelGGL(light_grid_visible_kernel, grid, block, 0, static_cast<hipStream_t>(stream),
                     VisibleRecords{reinterpret_cast<const char *>(d_probes), reinterpret_cast<const char *>(d_depth)}, G,
                     reinterpret_cast<const float4 *>(d_points), reinterpret_cast<const float4 *>(d_normals), (unsigned)numPoints,
                     (unsigned)flags, normalBias, reinterpret_cast<float4 *>(d_out));
  HIP_OK(hipGetLastError());
  return RM_OK;
}
