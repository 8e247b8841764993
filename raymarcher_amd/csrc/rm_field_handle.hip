// rm_field_handle.hip — RmField handles (gfx950 only): rm_field_create, rm_field_create_blocks, rm_field_destroy, rm_field_sample and
// rm_field_trace.  include/raymarcher_amd.h has the definitions, rm_field_march.h the sample's arithmetic and rm_field_skip.h the
// march's — the kernels here only load a point or a ray, call it and store the record.  A handle owns what is derived from a block
// list, the block map and the coarse level, in device memory of its own (plain hipMalloc, not the kWsBlocks workspace), built once
// at create.  A translation unit of its own, so that adding it leaves the code objects of the existing kernels as they were.
//   One lane per point or ray, 256-lane workgroups, one launch per call.  A record is two 16-byte stores.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/raymarcher_amd.h"
#include "rm_field_check.h"
#include "rm_field_skip.h"
#include "rm_internal.h"

struct RmField {
  uint32_t magic;  // kMagic while the handle lives: best effort against a stale or garbage pointer
  int device;      // the device current at create
  bool sparse;
  const float *dist;   // borrowed
  const int32_t *ids;  // borrowed, may be null
  int dims[3];         // n or m
  rm::fm::Frame frame;
  uint32_t *first;             // owned: the block map, sparse only
  unsigned long long *coarse;  // owned: the coarse level, sparse only
};

namespace rm {

int enqueue_block_map(const int32_t *d_blocks, int numBlocks, int mx, int my, int mz, uint32_t *first, hipStream_t stream);  // rm_blocks.hip

static_assert(RM_FIELD_PENUMBRA_K == 8.0f, "rm_field_skip.h has the 8 written out");
constexpr uint32_t kMagic = 0x524d4644u;  // "RMFD"

// The coarse level of a list: an entry inside the lattice sets its block's bit, a repeat sets it again.  `mask` is zeroed before.
__global__ __launch_bounds__(256) void field_coarse_kernel(const int32_t *__restrict__ list, unsigned numBlocks, int mx, int my, int mz,
                                                           unsigned long long *__restrict__ mask) {
  const unsigned n = blockIdx.x * 256u + threadIdx.x;
  if (n >= numBlocks) return;
  const int bi = list[4 * (size_t)n], bj = list[4 * (size_t)n + 1], bk = list[4 * (size_t)n + 2];
  if (!snb::in_range(snb::Blocks{nullptr, mx, my, mz}, bi, bj, bk)) return;
  const int g[3] = {fs::groups(mx), fs::groups(my), fs::groups(mz)};
  atomicOr(&mask[fs::group_linear(g, bi, bj, bk)], 1ull << fs::block_bit(bi, bj, bk));
}

template <class Field>
__global__ __launch_bounds__(256) void handle_sample_kernel(const float4 *__restrict__ points, unsigned n, Field F, fm::Frame L,
                                                            float4 *__restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const float4 q = points[i];
  const float p[3] = {q.x, q.y, q.z};
  const fm::Sample s = fm::sample_point(F, L, p);
  out[2 * i] = make_float4(s.gradient[0], s.gradient[1], s.gradient[2], s.value);
  out[2 * i + 1] = make_float4(__int_as_float(s.cell[0]), __int_as_float(s.cell[1]), __int_as_float(s.cell[2]), __int_as_float(s.objectId));
}

template <bool OCCLUSION, class Field>
__global__ __launch_bounds__(256) void handle_trace_kernel(const float4 *__restrict__ rays, unsigned n, Field F, fs::Coarse C, fm::Frame L,
                                                           float iso, int maxSteps, bool noNormal, float4 *__restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const float4 a = rays[2 * i], b = rays[2 * i + 1];
  const fm::Ray r{{a.x, a.y, a.z}, a.w, {b.x, b.y, b.z}};
  const fm::Hit h = fs::march_ray<OCCLUSION>(F, C, L, r, iso, maxSteps, noNormal);
  out[2 * i] = make_float4(h.normal[0], h.normal[1], h.normal[2], h.t);
  out[2 * i + 1] = make_float4(h.position[0], h.position[1], h.position[2], __int_as_float(h.objectId));
}

using fchk::aligned;
using fchk::bad;

// frees what a create has allocated unless the handle took it over
struct Owned {
  uint32_t *first = nullptr;
  unsigned long long *coarse = nullptr;
  ~Owned() {
    if (first) (void)hipFree(first);
    if (coarse) (void)hipFree(coarse);
  }
};

// What both creates check, in the header's order (the steps rm_field.hip shares are rm_field_check.h's); all but the last before
// any HIP call.  Dense: blocks = nullptr, numBlocks = −1.
static int check_create(const float *dist, const int32_t *ids, const int32_t *blocks, int numBlocks, bool sparse, const int dims[3],
                        const float *origin, const float *step, RmField **field) {
  if (int st = fchk::check_field_lattice(sparse, dims, origin, step, numBlocks)) return st;
  if (!field) return bad("null field");
  if (int st = fchk::check_field_arrays(nullptr, nullptr, dist, ids, blocks, numBlocks, sparse, "null d_dist",
                                        "misaligned d_dist, d_objectId or d_blocks (4 bytes)"))
    return st;
  return require_device_pointers({{"d_dist", dist}, {"d_objectId", ids}, {"d_blocks", numBlocks > 0 ? blocks : nullptr}});
}

static int create_field(const float *dist, const int32_t *ids, const int32_t *blocks, int numBlocks, bool sparse, const int dims[3],
                        const float *origin, const float *step, hipStream_t hs, RmField **field) {
  if (int st = check_create(dist, ids, blocks, numBlocks, sparse, dims, origin, step, field)) return st;
  int device = 0;
  HIP_OK(hipGetDevice(&device));
  Owned mem;
  if (sparse) {
    const size_t numMap = (size_t)dims[0] * (size_t)dims[1] * (size_t)dims[2];
    const size_t numGroups = (size_t)fs::groups(dims[0]) * (size_t)fs::groups(dims[1]) * (size_t)fs::groups(dims[2]);
    HIP_OK(hipMalloc(reinterpret_cast<void **>(&mem.first), numMap * sizeof(uint32_t)));
    HIP_OK(hipMalloc(reinterpret_cast<void **>(&mem.coarse), numGroups * sizeof(unsigned long long)));
    HIP_OK(hipMemsetAsync(mem.coarse, 0, numGroups * sizeof(unsigned long long), hs));
    if (numBlocks > 0) {
      if (int st = enqueue_block_map(blocks, numBlocks, dims[0], dims[1], dims[2], mem.first, hs)) return st;
      hipLaunchKernelGGL(field_coarse_kernel, dim3(((unsigned)numBlocks + 255u) / 256u), dim3(256), 0, hs, blocks, (unsigned)numBlocks, dims[0],
                         dims[1], dims[2], mem.coarse);
      HIP_OK(hipGetLastError());
    } else {  // an empty list: no block is listed
      HIP_OK(hipMemsetAsync(mem.first, 0xff, numMap * sizeof(uint32_t), hs));
    }
    HIP_OK(hipStreamSynchronize(hs));  // the list is consumed, and the handle is usable on any stream
  }
  RmField *f = new RmField{kMagic, device, sparse, dist, ids, {dims[0], dims[1], dims[2]},
                           fm::Frame{{origin[0], origin[1], origin[2]}, {step[0], step[1], step[2]}}, mem.first, mem.coarse};
  mem.first = nullptr, mem.coarse = nullptr;
  *field = f;
  return RM_OK;
}

// What both queries check, in the header's order.  RM_OK with *launch = false: a call of no point or ray.
static int check_query(const RmField *f, const void *in, int count, bool trace, float iso, int maxSteps, unsigned mode, void *out, bool *launch) {
  *launch = false;
  if (!f || !aligned(f, alignof(RmField)) || f->magic != kMagic) return bad("null or stale RmField handle");
  if (count < 0) return bad(trace ? "negative numRays" : "negative numPoints");
  if (trace)
    if (int st = fchk::check_field_march(iso, maxSteps, mode, RM_TRACE_NO_NORMAL | RM_TRACE_OCCLUSION,
                                         "mode bits other than RM_TRACE_NO_NORMAL and RM_TRACE_OCCLUSION"))
      return st;
  if (count == 0) return RM_OK;
  if (!in || !out) return bad(trace ? "null d_rays or d_hits" : "null d_points or d_samples");
  if (!aligned(in, 16) || !aligned(out, 16)) return bad(trace ? "misaligned d_rays or d_hits (16 bytes)" : "misaligned d_points or d_samples (16 bytes)");
  int device = -1;
  HIP_OK(hipGetDevice(&device));
  if (device != f->device) return bad("the RmField handle belongs to another device than the current one");
  if (int st = require_device_pointers({{trace ? "d_rays" : "d_points", in}, {trace ? "d_hits" : "d_samples", out}})) return st;
  *launch = true;
  return RM_OK;
}

template <class Field>
static void launch_query(const RmField *f, const Field &F, const void *in, int count, bool trace, float iso, int maxSteps, unsigned mode, void *out,
                         hipStream_t hs) {
  const dim3 grid(((unsigned)count + 255u) / 256u), block(256);  // at most 2^23 workgroups
  const fs::Coarse C{f->coarse, {fs::groups(f->dims[0]), fs::groups(f->dims[1]), fs::groups(f->dims[2])}};
  const float4 *src = static_cast<const float4 *>(in);
  float4 *dst = static_cast<float4 *>(out);
  if (!trace)
    hipLaunchKernelGGL(handle_sample_kernel<Field>, grid, block, 0, hs, src, (unsigned)count, F, f->frame, dst);
  else if (mode & RM_TRACE_OCCLUSION)
    hipLaunchKernelGGL((handle_trace_kernel<true, Field>), grid, block, 0, hs, src, (unsigned)count, F, C, f->frame, iso, maxSteps, false, dst);
  else
    hipLaunchKernelGGL((handle_trace_kernel<false, Field>), grid, block, 0, hs, src, (unsigned)count, F, C, f->frame, iso, maxSteps,
                       (mode & RM_TRACE_NO_NORMAL) != 0u, dst);
}

static int run_query(const RmField *f, const void *in, int count, bool trace, float iso, int maxSteps, unsigned mode, void *out, void *stream) {
  bool launch = false;
  if (int st = check_query(f, in, count, trace, iso, maxSteps, mode, out, &launch)) return st;
  if (!launch) return RM_OK;
  const hipStream_t hs = static_cast<hipStream_t>(stream);
  if (f->sparse)
    launch_query(f, fm::Blocks{f->dist, f->ids, snb::Blocks{f->first, f->dims[0], f->dims[1], f->dims[2]}}, in, count, trace, iso, maxSteps, mode,
                 out, hs);
  else
    launch_query(f, fm::Dense{f->dist, f->ids, {f->dims[0], f->dims[1], f->dims[2]}}, in, count, trace, iso, maxSteps, mode, out, hs);
  HIP_OK(hipGetLastError());
  return RM_OK;
}

}  // namespace rm

using namespace rm;

extern "C" int rm_field_create(const float *d_dist, const int32_t *d_objectId, int nx, int ny, int nz, const float origin[3], const float step[3],
                               RmField **field) {
  if (field) *field = nullptr;
  const int dims[3] = {nx, ny, nz};
  return create_field(d_dist, d_objectId, nullptr, -1, false, dims, origin, step, nullptr, field);
}

extern "C" int rm_field_create_blocks(const float *d_dist, const int32_t *d_objectId, const int32_t *d_blocks, int numBlocks, int mx, int my, int mz,
                                      const float origin[3], const float step[3], void *stream, RmField **field) {
  if (field) *field = nullptr;
  const int dims[3] = {mx, my, mz};
  return create_field(d_dist, d_objectId, d_blocks, numBlocks, true, dims, origin, step, static_cast<hipStream_t>(stream), field);
}

extern "C" void rm_field_destroy(RmField *field) {
  if (!field || field->magic != kMagic) return;
  field->magic = 0u;
  if (field->first) (void)hipFree(field->first);
  if (field->coarse) (void)hipFree(field->coarse);
  delete field;
}

extern "C" int rm_field_sample(const RmField *field, const float *d_points, int numPoints, RmFieldSample *d_samples, void *stream) {
  return run_query(field, d_points, numPoints, false, 0.0f, 0, 0u, d_samples, stream);
}

extern "C" int rm_field_trace(const RmField *field, const RmRay *d_rays, int numRays, float iso, int maxSteps, unsigned mode, RmRayHit *d_hits,
                              void *stream) {
  return run_query(field, d_rays, numRays, true, iso, maxSteps, mode, d_hits, stream);
}
