// rm_light_grid.hip — rm_light_grid_irradiance (gfx950 only): the light that a grid of rm_light_probes' SH9 records gives points with
// normals, ONE launch, one lane per point.  The arithmetic is rm_light_grid.h's grid_light, the very code of the host program of
// tests/light_grid_spec; the kernel here only loads, calls it and stores.  The entry is no render launch: like the field queries
// (rm_field.hip) it stages no scene block, records no path and no timing, touches no tuner or workspace state and allocates nothing.
// A translation unit of its own, so that adding it leaves the code objects of the existing kernels as they were.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "rm_internal.h"
#include "rm_lattice.h"
#include "rm_light_grid.h"

namespace rm {

static_assert(sizeof(lg::GridLight) == 32 && sizeof(RmGridLight) == 32, "two float4 per record");
static_assert(sizeof(RmLightProbe) == 160 && offsetof(RmLightProbe, hits) == 144, "ten float4 per probe, hits in the last");
static_assert(lg::kInvalid == RM_RAY_INVALID && lg::kFacing == RM_LIGHT_GRID_FACING, "the header's codes");
static_assert(lg::kMaxDim == RM_MAX_LIGHT_GRID_DIM && lg::kMaxProbes == RM_MAX_LIGHT_GRID_PROBES, "rm_light_grid.h has the header's limits");

// The records where rm_light_probes stored them: 160 bytes each, so the byte offset of probe 2^24 − 1 needs more than 31 bits and
// is a size_t.  hits is one dword; a coefficient is one 16-byte load.
struct ProbeRecords {
  const char *base;
  __host__ __device__ int hits(size_t i) const { return *reinterpret_cast<const int32_t *>(base + i * sizeof(RmLightProbe) + offsetof(RmLightProbe, hits)); }
  __host__ __device__ void sh(size_t i, int j, float out[4]) const {
    const float4 v = *reinterpret_cast<const float4 *>(base + i * sizeof(RmLightProbe) + 16u * (size_t)j);
    out[0] = v.x, out[1] = v.y, out[2] = v.z, out[3] = v.w;
  }
};

// One lane per point: its two 16-byte inputs, the eight hits words of its cell's corners, then the nine float4 of every corner
// that is valid — never a word of an invalid probe's sh —, four sums per corner, and the record as two 16-byte stores.  Lanes that
// are neighbours in space share a cell and with it the lines they load.  -ffp-contract=off.
__global__ __launch_bounds__(256) void light_grid_kernel(ProbeRecords probes, lg::Grid G, const float4 *__restrict__ points,
                                                         const float4 *__restrict__ normals, unsigned n, unsigned flags,
                                                         float4 *__restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const float4 q = points[i], m = normals[i];
  const float p[3] = {q.x, q.y, q.z}, nrm[3] = {m.x, m.y, m.z};
  const lg::GridLight r = lg::grid_light(G, p, nrm, flags, probes);
  out[2 * i] = make_float4(r.e[0], r.e[1], r.e[2], r.e[3]);
  out[2 * i + 1] = make_float4(r.weight, __int_as_float(r.probes), 0.0f, 0.0f);
}

namespace {
using fchk::aligned;
using fchk::bad;

// In the header's order; no HIP call before the last.  RM_OK with *launch = false: a call of no point.
int check_light_grid(const RmLightProbe *d_probes, const int *dims, const float *origin, const float *step, const float *d_points,
                     const float *d_normals, int numPoints, uint32_t flags, const RmGridLight *d_out, bool *launch) {
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
  if (flags & ~RM_LIGHT_GRID_FACING) return bad("flag bits other than RM_LIGHT_GRID_FACING");
  if (numPoints == 0) return RM_OK;
  if (!d_probes || !d_points || !d_normals || !d_out) return bad("null d_probes, d_points, d_normals or d_out");
  if (!aligned(d_probes, 16) || !aligned(d_points, 16) || !aligned(d_normals, 16) || !aligned(d_out, 16))
    return bad("d_probes, d_points, d_normals and d_out must be 16-byte aligned");
  if (int st = require_device_pointers({{"d_probes", d_probes}, {"d_points", d_points}, {"d_normals", d_normals}, {"d_out", d_out}})) return st;
  *launch = true;
  return RM_OK;
}
}  // namespace

}  // namespace rm

using namespace rm;

extern "C" int rm_light_grid_irradiance(const RmLightProbe *d_probes, const int dims[3], const float origin[3], const float step[3],
                                        const float *d_points, const float *d_normals, int numPoints, uint32_t flags, RmGridLight *d_out,
                                        void *stream) {
  bool launch = false;
  if (int st = check_light_grid(d_probes, dims, origin, step, d_points, d_normals, numPoints, flags, d_out, &launch)) return st;
  if (!launch) return RM_OK;
  const lg::Grid G{{dims[0], dims[1], dims[2]}, {origin[0], origin[1], origin[2]}, {step[0], step[1], step[2]}};
  const dim3 grid(((unsigned)numPoints + 255u) / 256u), block(256);  // at most 2^23 workgroups
  hipLaunchKernelGGL(light_grid_kernel, grid, block, 0, static_cast<hipStream_t>(stream), ProbeRecords{reinterpret_cast<const char *>(d_probes)},
                     G, reinterpret_cast<const float4 *>(d_points), reinterpret_cast<const float4 *>(d_normals), (unsigned)numPoints,
                     (unsigned)flags, reinterpret_cast<float4 *>(d_out));
  HIP_OK(hipGetLastError());
  return RM_OK;
}
