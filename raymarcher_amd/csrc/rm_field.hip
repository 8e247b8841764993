// rm_field.hip — a baked lattice read back at arbitrary points and marched by rays (gfx950 only): rm_sdf_sample, rm_sdf_sample_blocks,
// rm_sdf_trace and rm_sdf_trace_blocks, which take the lattice with every call, and the RmField handles — rm_field_create,
// rm_field_create_blocks, rm_field_destroy, rm_field_sample, rm_field_trace and rm_field_ambient (with the host's
// rm_hemisphere_directions).  include/raymarcher_amd.h has the definitions, rm_field_march.h the sample's arithmetic and the calls'
// march, rm_field_skip.h the handles' march, rm_field_ambient.h a point's normal, frame, rays and leaves — the kernels here only
// load a point or a ray, call it and store the record; the ambient kernel also folds a point's leaves across lanes.  rm_lattice.h has
// the checks the two groups share.
//   One lane per point or ray, 256-lane workgroups, one launch per call.  A record is two 16-byte stores.  A block call builds the
// block map first (enqueue_block_map, rm_blocks.hip) in the kWsBlocks workspace; a handle owns what is derived from a block list,
// the block map and the coarse level, in device memory of its own (plain hipMalloc), built once at create.
#include <hip/hip_runtime.h>

#include <mutex>
#include <string>

#include "rm_field_ambient.h"
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
static_assert(sizeof(fa::Ambient) == 32 && sizeof(RmAmbient) == 32, "two float4 per record");
static_assert(fa::kMaxDirs == RM_MAX_AMBIENT_DIRS && RM_MAX_AMBIENT_DIRS == 1 << fa::kMaxLevels, "rm_field_ambient.h has the header's limit");
static_assert(RM_MAX_AMBIENT_TABLE * sizeof(float4) == 16384, "the table a workgroup stages: 16 KB of LDS");
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

// rm_field_ambient: (point, direction) pairs flattened over lanes, lane % numDirs the direction.  With numDirs <= 64 a wave holds
// 64 / numDirs points, a SEGMENT of numDirs lanes each, and folds every segment's leaves by log2(numDirs) xor levels: at level l
// lane j adds lane j ^ 2^l, which for the lanes with that bit clear is the tree's s[2j] + s[2j + 1] and for the others the same
// two operands the other way round, the same word (rm_field_ambient.h), so every lane of a segment ends with the sums and lane 0
// of it stores.  128 and 256 directions are 2 or 4 passes of 64 by one wave on one point, whose sums fold by the same tree.  The
// table (at most 16 KB) is staged into LDS once per workgroup.  Every lane of a segment works its point's normal and frame out
// for itself: the same loads and operations in all of them, at the cost of one lane's.  A wave whose first point is past the end
// leaves as a whole, before the shuffles; in the last live wave the segments past the end march nothing, carry zeros through the
// shuffles and store nothing.
//   MULTI: more than 64 directions.  The one-pass kernel has no loop around its march, and so nothing of the point but its normal,
// the ray's direction and its weight alive across it: 69 to 71 VGPRs on a block handle where one kernel that loops for every
// numDirs has 91 to 94, 7 waves per SIMD instead of 5 (profiles/field_ambient.md has what that is worth).
template <bool SOFT, bool MULTI, class Field>
__global__ __launch_bounds__(256) void field_ambient_kernel(const float4 *__restrict__ points, const float4 *__restrict__ normals, unsigned n,
                                                            const float4 *__restrict__ dirs, int numDirs, int numSets, Field F, fs::Coarse C,
                                                            fm::Frame L, float bias, float maxDistance, float iso, int maxSteps,
                                                            float4 *__restrict__ out) {
  __shared__ float4 table[RM_MAX_AMBIENT_TABLE];
  for (int j = (int)threadIdx.x; j < numSets * numDirs; j += 256) table[j] = dirs[j];
  __syncthreads();
  const unsigned lane = threadIdx.x & 63u, seg = numDirs < 64 ? (unsigned)numDirs : 64u, perWave = 64u / seg;
  const size_t first = ((size_t)blockIdx.x * 4u + (threadIdx.x >> 6)) * perWave;  // the wave's first point
  if (first >= n) return;                                                          // wave-uniform
  const size_t i = first + lane / seg;
  const unsigned k0 = lane & (seg - 1u);
  const bool live = i < n;
  const float4 *set = table + (size_t)((unsigned)i % (unsigned)numSets) * (size_t)numDirs;
  const int passes = MULTI ? numDirs / 64 : 1;  // 1, 2 or 4
  // acc0 and acc1 are the tree's pending left operands above the passes: S0, then S0 + S1 — (S0 + S1) + (S2 + S3) in the end.
  float nrm[3] = {0.0f, 0.0f, 0.0f}, s[4] = {0.0f, 0.0f, 0.0f, 0.0f}, acc0[4] = {0.0f, 0.0f, 0.0f, 0.0f}, acc1[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  int code = 0, hits = 0;
#pragma unroll 1
  for (int pass = 0; pass < passes; pass++) {
    int hit = 0;
#pragma unroll
    for (int c = 0; c < 4; c++) s[c] = 0.0f;
    if (live) {
      const float4 q = points[i];
      const float p[3] = {q.x, q.y, q.z};
      if (normals) {
        const float4 g = normals[i];
        const float given[3] = {g.x, g.y, g.z};
        code = fa::point_normal(F, L, p, given, nrm);
      } else {
        code = fa::point_normal(F, L, p, nullptr, nrm);
      }
      if (code == 0) {
        float T[3], B[3];
        fa::tangent_frame(nrm, T, B);
        const float4 e4 = set[pass * 64 + (int)k0];
        const float e[4] = {e4.x, e4.y, e4.z, e4.w};
        hit = fa::ray_leaf<SOFT>(F, C, L, p, nrm, T, B, e, bias, maxDistance, iso, maxSteps, s) ? 1 : 0;
      }
    }
    for (unsigned m = 1u; m < seg; m <<= 1) {
#pragma unroll
      for (int c = 0; c < 4; c++) s[c] = s[c] + __shfl_xor(s[c], (int)m);
      hit += __shfl_xor(hit, (int)m);
    }
    hits += hit;
#pragma unroll
    for (int c = 0; c < 4; c++) {
      if (pass & 1) {
        s[c] = acc0[c] + s[c];
        if (pass & 2) s[c] = acc1[c] + s[c];
        else acc1[c] = s[c];
      } else {
        acc0[c] = s[c];
      }
    }
  }
  if (!live || k0 != 0u) return;
  const bool refused = code != 0;
  out[2 * i] = make_float4(s[0], s[1], s[2], s[3]);
  out[2 * i + 1] = make_float4(refused ? 0.0f : nrm[0], refused ? 0.0f : nrm[1], refused ? 0.0f : nrm[2], __int_as_float(refused ? code : hits));
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

// ---- rm_field_ambient ---------------------------------------------------------------------------------------------------------------
static bool ambient_dirs_ok(int numDirs) { return numDirs >= 1 && numDirs <= RM_MAX_AMBIENT_DIRS && (numDirs & (numDirs - 1)) == 0; }
// What rm_field_ambient and rm_hemisphere_directions refuse about the table's shape; no HIP call.
static int check_ambient_table(int numDirs, int numSets) {
  if (!ambient_dirs_ok(numDirs)) return bad("numDirs must be a power of two, 1 … RM_MAX_AMBIENT_DIRS (256)");
  if (numSets < 1 || (long long)numSets * numDirs > RM_MAX_AMBIENT_TABLE) return bad("numSets must be at least 1 and numSets * numDirs at most RM_MAX_AMBIENT_TABLE (1024)");
  return RM_OK;
}

struct AmbientCall {
  const float *points, *normals;
  int numPoints;
  const float *dirs;
  int numDirs, numSets;
  float bias, maxDistance, iso;
  int maxSteps;
  unsigned mode;
  RmAmbient *out;
};
// In the header's order.  RM_OK with *launch = false: a call of no point.
static int check_ambient(const RmField *f, const AmbientCall &c, bool *launch) {
  *launch = false;
  if (!f || !aligned(f, alignof(RmField)) || f->magic != kMagic) return bad("null or stale RmField handle");
  if (c.numPoints < 0) return bad("negative numPoints");
  if (int st = check_ambient_table(c.numDirs, c.numSets)) return st;
  if (!std::isfinite(c.bias)) return bad("bias must be finite");
  if (!std::isfinite(c.maxDistance) || c.maxDistance < 0.0f) return bad("maxDistance must be finite and not negative");
  if (int st = fchk::check_field_march(c.iso, c.maxSteps, c.mode, RM_AMBIENT_HARD, "mode bits other than RM_AMBIENT_HARD")) return st;
  if (c.numPoints == 0) return RM_OK;
  if (!c.points || !c.dirs || !c.out) return bad("null d_points, d_dirs or d_out");
  if (!aligned(c.points, 16) || !aligned(c.normals, 16) || !aligned(c.dirs, 16) || !aligned(c.out, 16))
    return bad("misaligned d_points, d_normals, d_dirs or d_out (16 bytes)");
  int device = -1;
  HIP_OK(hipGetDevice(&device));
  if (device != f->device) return bad("the RmField handle belongs to another device than the current one");
  if (int st = require_device_pointers({{"d_points", c.points}, {"d_normals", c.normals}, {"d_dirs", c.dirs}, {"d_out", c.out}})) return st;
  *launch = true;
  return RM_OK;
}

template <class Field>
static void launch_ambient(const RmField *f, const Field &F, const AmbientCall &c, hipStream_t hs) {
  const unsigned perWave = c.numDirs < 64 ? 64u / (unsigned)c.numDirs : 1u;
  const unsigned waves = ((unsigned)c.numPoints + perWave - 1u) / perWave;  // at most 2^31 − 1
  const dim3 grid(waves / 4u + (waves % 4u != 0u ? 1u : 0u)), block(256);
  const fs::Coarse C{f->coarse, {fs::groups(f->dims[0]), fs::groups(f->dims[1]), fs::groups(f->dims[2])}};
  const float4 *pts = reinterpret_cast<const float4 *>(c.points), *nrm = reinterpret_cast<const float4 *>(c.normals);
  const float4 *dirs = reinterpret_cast<const float4 *>(c.dirs);
  float4 *dst = reinterpret_cast<float4 *>(c.out);
  const bool hard = (c.mode & RM_AMBIENT_HARD) != 0u, multi = c.numDirs > 64;
  auto kernel = hard ? (multi ? field_ambient_kernel<false, true, Field> : field_ambient_kernel<false, false, Field>)
                     : (multi ? field_ambient_kernel<true, true, Field> : field_ambient_kernel<true, false, Field>);
  hipLaunchKernelGGL(kernel, grid, block, 0, hs, pts, nrm, (unsigned)c.numPoints, dirs, c.numDirs, c.numSets, F, C, f->frame, c.bias, c.maxDistance,
                     c.iso, c.maxSteps, dst);
}

static int run_ambient(const RmField *f, const AmbientCall &c, void *stream) {
  bool launch = false;
  if (int st = check_ambient(f, c, &launch)) return st;
  if (!launch) return RM_OK;
  const hipStream_t hs = static_cast<hipStream_t>(stream);
  if (f->sparse)
    launch_ambient(f, fm::Blocks{f->dist, f->ids, snb::Blocks{f->first, f->dims[0], f->dims[1], f->dims[2]}}, c, hs);
  else
    launch_ambient(f, fm::Dense{f->dist, f->ids, {f->dims[0], f->dims[1], f->dims[2]}}, c, hs);
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

extern "C" int rm_hemisphere_directions(int numDirs, int numSets, float *out4) {
  if (int st = check_ambient_table(numDirs, numSets)) return st;
  if (!out4) return bad("null out4");
  const double K = (double)numDirs, twoPi = 6.283185307179586476925286766559;
  for (int s = 0; s < numSets; s++)
    for (int k = 0; k < numDirs; k++) {
      const double u = ((double)k + 0.5) / K, r = std::sqrt(u), z = std::sqrt(1.0 - u);
      const double turn = (double)k * 0.6180339887498949 + (double)s * 0.7548776662466927, phi = twoPi * (turn - std::floor(turn));
      float *e = out4 + 4 * ((size_t)s * (size_t)numDirs + (size_t)k);
      e[0] = (float)(r * std::cos(phi)), e[1] = (float)(r * std::sin(phi)), e[2] = (float)z, e[3] = (float)(1.0 / K);
    }
  return RM_OK;
}

extern "C" int rm_field_ambient(const RmField *field, const float *d_points, const float *d_normals, int numPoints, const float *d_dirs, int numDirs,
                                int numSets, float bias, float maxDistance, float iso, int maxSteps, unsigned mode, RmAmbient *d_out, void *stream) {
  return run_ambient(field, AmbientCall{d_points, d_normals, numPoints, d_dirs, numDirs, numSets, bias, maxDistance, iso, maxSteps, mode, d_out}, stream);
}
