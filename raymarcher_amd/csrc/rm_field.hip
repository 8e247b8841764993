// rm_field.hip — rm_sdf_sample, rm_sdf_sample_blocks, rm_sdf_trace and rm_sdf_trace_blocks (gfx950 only): a baked lattice read back
// at arbitrary points and marched by rays.  include/raymarcher_amd.h has the definitions, rm_field_march.h the arithmetic — the
// kernels here only load a point or a ray, call it and store the record.  Everything of the four entry points is here, as
// rm_sdf_mesh_blocks is in rm_blocks.hip.  A translation unit of its own, so that adding it leaves the code objects of the existing
// kernels as they were.
//   One lane per point or ray, 256-lane workgroups, one launch per call; the block entries build the block map first
//   (enqueue_block_map, rm_blocks.hip) in the kWsBlocks workspace.  A record is two 16-byte stores.
#include <hip/hip_runtime.h>

#include <climits>
#include <mutex>
#include <string>

#include "../../include/raymarcher_amd.h"
#include "rm_field_check.h"
#include "rm_field_march.h"
#include "rm_internal.h"

namespace rm {

int enqueue_block_map(const int32_t *d_blocks, int numBlocks, int mx, int my, int mz, uint32_t *first, hipStream_t stream);  // rm_blocks.hip

template <class Field>
__global__ __launch_bounds__(256) void field_sample_kernel(const float4 *__restrict__ points, unsigned n, Field F, fm::Frame L,
                                                           float4 *__restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const float4 q = points[i];
  const float p[3] = {q.x, q.y, q.z};
  const fm::Sample s = fm::sample_point(F, L, p);
  out[2 * i] = make_float4(s.gradient[0], s.gradient[1], s.gradient[2], s.value);
  out[2 * i + 1] = make_float4(__int_as_float(s.cell[0]), __int_as_float(s.cell[1]), __int_as_float(s.cell[2]), __int_as_float(s.objectId));
}

template <class Field>
__global__ __launch_bounds__(256) void field_trace_kernel(const float4 *__restrict__ rays, unsigned n, Field F, fm::Frame L, float iso,
                                                          int maxSteps, bool noNormal, float4 *__restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const float4 a = rays[2 * i], b = rays[2 * i + 1];
  const fm::Ray r{{a.x, a.y, a.z}, a.w, {b.x, b.y, b.z}};
  const fm::Hit h = fm::march_ray(F, L, r, iso, maxSteps, noNormal);
  out[2 * i] = make_float4(h.normal[0], h.normal[1], h.normal[2], h.t);
  out[2 * i + 1] = make_float4(h.position[0], h.position[1], h.position[2], __int_as_float(h.objectId));
}

using fchk::bad;

// What the four entry points check, in the header's order (the steps rm_field_handle.hip shares are rm_field_check.h's); no HIP
// call.  A dense call has d_blocks = nullptr and numBlocks = −1.
struct FieldCall {
  const void *in;       // d_points or d_rays
  int count;
  const float *dist;
  const int32_t *ids, *blocks;
  int numBlocks;
  bool sparse, trace;
  int dims[3];          // n or m
  const float *origin, *step;
  float iso;
  int maxSteps;
  unsigned mode;
  void *out;            // d_samples or d_hits
};
// RM_OK with *launch = false: a call of no point or ray
static int check_field_call(const FieldCall &c, bool *launch) {
  *launch = false;
  if (c.count < 0) return bad(c.trace ? "negative numRays" : "negative numPoints");
  if (int st = fchk::check_field_lattice(c.sparse, c.dims, c.origin, c.step, c.numBlocks)) return st;
  if (c.trace)
    if (int st = fchk::check_field_march(c.iso, c.maxSteps, c.mode, RM_TRACE_NO_NORMAL, "mode bits other than RM_TRACE_NO_NORMAL")) return st;
  if (c.count == 0) return RM_OK;
  const char *nullText = c.trace ? "null d_rays, d_hits or d_dist" : "null d_points, d_samples or d_dist";
  if (!c.in || !c.out) return bad(nullText);
  if (int st = fchk::check_field_arrays(c.in, c.out, c.dist, c.ids, c.blocks, c.numBlocks, c.sparse, nullText,
                                        c.trace ? "misaligned d_rays or d_hits (16 bytes), d_dist, d_objectId or d_blocks (4 bytes)"
                                                : "misaligned d_points or d_samples (16 bytes), d_dist, d_objectId or d_blocks (4 bytes)"))
    return st;
  if (int st = require_device_pointers({{c.trace ? "d_rays" : "d_points", c.in}, {"d_dist", c.dist}, {"d_objectId", c.ids},
                                        {"d_blocks", c.numBlocks > 0 ? c.blocks : nullptr}, {c.trace ? "d_hits" : "d_samples", c.out}}))
    return st;
  *launch = true;
  return RM_OK;
}

template <class Field>
static int launch_field(const FieldCall &c, const Field &F, hipStream_t hs) {
  const fm::Frame L{{c.origin[0], c.origin[1], c.origin[2]}, {c.step[0], c.step[1], c.step[2]}};
  const dim3 grid(((unsigned)c.count + 255u) / 256u), block(256);  // at most 2^23 workgroups
  if (c.trace)
    hipLaunchKernelGGL(field_trace_kernel<Field>, grid, block, 0, hs, static_cast<const float4 *>(c.in), (unsigned)c.count, F, L, c.iso, c.maxSteps,
                       (c.mode & RM_TRACE_NO_NORMAL) != 0u, static_cast<float4 *>(c.out));
  else
    hipLaunchKernelGGL(field_sample_kernel<Field>, grid, block, 0, hs, static_cast<const float4 *>(c.in), (unsigned)c.count, F, L,
                       static_cast<float4 *>(c.out));
  HIP_OK(hipGetLastError());
  return RM_OK;
}

static int run_field_call(const FieldCall &c, void *stream) {
  bool launch = false;
  if (int st = check_field_call(c, &launch)) return st;
  if (!launch) return RM_OK;
  const hipStream_t hs = static_cast<hipStream_t>(stream);
  if (!c.sparse) return launch_field(c, fm::Dense{c.dist, c.ids, {c.dims[0], c.dims[1], c.dims[2]}}, hs);
  // the workspace is in use until the last launch is enqueued: the device's launcher lock keeps rm_release_workspaces away
  std::unique_lock<std::mutex> lock;
  if (int st = lock_current_device(lock)) return st;
  void *mem = nullptr;
  if (int st = stream_workspace(kWsBlocks, hs, blocks_map_workspace(c.dims[0], c.dims[1], c.dims[2]), &mem)) return st;
  uint32_t *first = static_cast<uint32_t *>(mem);
  if (c.numBlocks > 0) {
    if (int st = enqueue_block_map(c.blocks, c.numBlocks, c.dims[0], c.dims[1], c.dims[2], first, hs)) return st;
  } else {  // an empty list: no block is listed
    HIP_OK(hipMemsetAsync(first, 0xff, (size_t)c.dims[0] * (size_t)c.dims[1] * (size_t)c.dims[2] * sizeof(uint32_t), hs));
  }
  return launch_field(c, fm::Blocks{c.dist, c.ids, snb::Blocks{first, c.dims[0], c.dims[1], c.dims[2]}}, hs);
}

}  // namespace rm

using namespace rm;

extern "C" int rm_sdf_sample(const float *d_points, int numPoints, const float *d_dist, const int32_t *d_objectId, int nx, int ny, int nz,
                             const float origin[3], const float step[3], RmFieldSample *d_samples, void *stream) {
  return run_field_call(FieldCall{d_points, numPoints, d_dist, d_objectId, nullptr, -1, false, false, {nx, ny, nz}, origin, step, 0.0f, 0, 0u, d_samples},
                        stream);
}

extern "C" int rm_sdf_sample_blocks(const float *d_points, int numPoints, const float *d_dist, const int32_t *d_objectId, const int32_t *d_blocks,
                                    int numBlocks, int mx, int my, int mz, const float origin[3], const float step[3], RmFieldSample *d_samples,
                                    void *stream) {
  return run_field_call(
      FieldCall{d_points, numPoints, d_dist, d_objectId, d_blocks, numBlocks, true, false, {mx, my, mz}, origin, step, 0.0f, 0, 0u, d_samples}, stream);
}

extern "C" int rm_sdf_trace(const RmRay *d_rays, int numRays, const float *d_dist, const int32_t *d_objectId, int nx, int ny, int nz,
                            const float origin[3], const float step[3], float iso, int maxSteps, unsigned mode, RmRayHit *d_hits, void *stream) {
  return run_field_call(FieldCall{d_rays, numRays, d_dist, d_objectId, nullptr, -1, false, true, {nx, ny, nz}, origin, step, iso, maxSteps, mode, d_hits},
                        stream);
}

extern "C" int rm_sdf_trace_blocks(const RmRay *d_rays, int numRays, const float *d_dist, const int32_t *d_objectId, const int32_t *d_blocks,
                                   int numBlocks, int mx, int my, int mz, const float origin[3], const float step[3], float iso, int maxSteps,
                                   unsigned mode, RmRayHit *d_hits, void *stream) {
  return run_field_call(
      FieldCall{d_rays, numRays, d_dist, d_objectId, d_blocks, numBlocks, true, true, {mx, my, mz}, origin, step, iso, maxSteps, mode, d_hits}, stream);
}
