// rm_field.hip — a baked lattice read back at arbitrary points and marched by rays (gfx950 only): rm_sdf_sample, rm_sdf_sample_blocks,
// rm_sdf_trace and rm_sdf_trace_blocks, which take the lattice with every call, and the RmField handles — rm_field_create,
// rm_field_create_blocks, rm_field_destroy, rm_field_sample and rm_field_trace.  include/raymarcher_amd.h has the definitions,
// rm_field_march.h the sample's arithmetic and the calls' march, rm_field_skip.h the handles' march — the kernels here only load a
// point or a ray, call it and store the record.  rm_lattice.h has the checks the two groups share.
//   One lane per point or ray, 256-lane workgroups, one launch per call.  A record is two 16-byte stores.  A block call builds the
// block map first (enqueue_block_map, rm_blocks.hip) in the kWsBlocks workspace; a handle owns what is derived from a block list,
// the block map and the coarse level, in device memory of its own (plain hipMalloc), built once at create.
#include <hip/hip_runtime.h>

#include <mutex>
#include <string>

#include "rm_field_skip.h"
#include "rm_lattice.h"

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

static_assert(sizeof(fm::Sample) == 32 && sizeof(RmFieldSample) == 32 && sizeof(fm::Hit) == 32 && sizeof(RmRayHit) == 32, "two float4 per record");
static_assert(fm::kInvalid == RM_RAY_INVALID && fm::kOutside == RM_FIELD_OUTSIDE && fm::kUnlisted == RM_FIELD_UNLISTED, "the header's codes");
static_assert(RM_FIELD_PENUMBRA_K == 8.0f, "rm_field_skip.h has the 8 written out");
constexpr uint32_t kMagic = 0x524d4644u;  // "RMFD"

// ---- the kernels ------------------------------------------------------------------------------------------------------------------
#define RF_DEV __device__ __forceinline__

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

RF_DEV fm::Ray load_ray(const float4 *__restrict__ ray) {
  const float4 a = ray[0], b = ray[1];
  return fm::Ray{{a.x, a.y, a.z}, a.w, {b.x, b.y, b.z}};
}
// A hit as the two words a kernel stores at out[2·i] and out[2·i + 1].  The stores stay in the kernels, and load_ray takes the ray's
// address, not the array and i: in these forms the six march kernels compile to the instruction streams they had with the load and
// the record written out in each (profiles/lattice_units.md).
struct Record { float4 lo, hi; };
RF_DEV Record hit_record(const fm::Hit &h) {
  return Record{make_float4(h.normal[0], h.normal[1], h.normal[2], h.t),
                make_float4(h.position[0], h.position[1], h.position[2], __int_as_float(h.objectId))};
}

// rm_sdf_trace and rm_sdf_trace_blocks
template <class Field>
__global__ __launch_bounds__(256) void field_trace_kernel(const float4 *__restrict__ rays, unsigned n, Field F, fm::Frame L, float iso,
                                                          int maxSteps, bool noNormal, float4 *__restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const fm::Ray r = load_ray(rays + 2 * i);
  const fm::Hit h = fm::march_ray(F, L, r, iso, maxSteps, noNormal);
  const Record rec = hit_record(h);
  out[2 * i] = rec.lo;
  out[2 * i + 1] = rec.hi;
}
// rm_field_trace: the march that skips by the coarse level, and the occlusion mode
template <bool OCCLUSION, class Field>
__global__ __launch_bounds__(256) void handle_trace_kernel(const float4 *__restrict__ rays, unsigned n, Field F, fs::Coarse C, fm::Frame L,
                                                           float iso, int maxSteps, bool noNormal, float4 *__restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const fm::Ray r = load_ray(rays + 2 * i);
  const fm::Hit h = fs::march_ray<OCCLUSION>(F, C, L, r, iso, maxSteps, noNormal);
  const Record rec = hit_record(h);
  out[2 * i] = rec.lo;
  out[2 * i + 1] = rec.hi;
}

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

using fchk::aligned;
using fchk::bad;

// one workgroup per 256 points or rays: at most 2^23 workgroups
static dim3 record_grid(int count) { return dim3(((unsigned)count + 255u) / 256u); }

// ---- the calls that take the lattice ----------------------------------------------------------------------------------------------
// What the four entry points check, in the header's order; no HIP call.  A dense call has d_blocks = nullptr and numBlocks = −1.
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
  const dim3 grid = record_grid(c.count), block(256);
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
  Carve ws(mem);
  uint32_t *first = take_block_map(ws, c.dims[0], c.dims[1], c.dims[2]);
  if (int st = enqueue_block_map(c.blocks, c.numBlocks, c.dims[0], c.dims[1], c.dims[2], first, hs)) return st;
  return launch_field(c, fm::Blocks{c.dist, c.ids, snb::Blocks{first, c.dims[0], c.dims[1], c.dims[2]}}, hs);
}

// ---- the handles --------------------------------------------------------------------------------------------------------------------
// frees what a create has allocated unless the handle took it over
struct Owned {
  uint32_t *first = nullptr;
  unsigned long long *coarse = nullptr;
  ~Owned() {
    if (first) (void)hipFree(first);
    if (coarse) (void)hipFree(coarse);
  }
};

// What both creates check, in the header's order; all but the last before any HIP call.  Dense: blocks = nullptr, numBlocks = −1.
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
    const size_t numGroups = (size_t)fs::groups(dims[0]) * (size_t)fs::groups(dims[1]) * (size_t)fs::groups(dims[2]);
    HIP_OK(hipMalloc(reinterpret_cast<void **>(&mem.first), (size_t)dims[0] * (size_t)dims[1] * (size_t)dims[2] * sizeof(uint32_t)));
    HIP_OK(hipMalloc(reinterpret_cast<void **>(&mem.coarse), numGroups * sizeof(unsigned long long)));
    HIP_OK(hipMemsetAsync(mem.coarse, 0, numGroups * sizeof(unsigned long long), hs));
    if (int st = enqueue_block_map(blocks, numBlocks, dims[0], dims[1], dims[2], mem.first, hs)) return st;
    if (numBlocks > 0) {
      hipLaunchKernelGGL(field_coarse_kernel, record_grid(numBlocks), dim3(256), 0, hs, blocks, (unsigned)numBlocks, dims[0], dims[1], dims[2],
                         mem.coarse);
      HIP_OK(hipGetLastError());
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
  const dim3 grid = record_grid(count), block(256);
  const fs::Coarse C{f->coarse, {fs::groups(f->dims[0]), fs::groups(f->dims[1]), fs::groups(f->dims[2])}};
  const float4 *src = static_cast<const float4 *>(in);
  float4 *dst = static_cast<float4 *>(out);
  if (!trace)
    hipLaunchKernelGGL(field_sample_kernel<Field>, grid, block, 0, hs, src, (unsigned)count, F, f->frame, dst);
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
