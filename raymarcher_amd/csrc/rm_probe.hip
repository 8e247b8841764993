// rm_probe.hip — the test-only device probes: the scene evaluator's production instantiations (rm_probe_sdscene_variant), the
// plain evaluator (rm_probe_sdscene), the rm_math built-ins (rm_probe_math), the bump gradient's four noise samples (rm_probe_bump),
// the shadow pool's cull of a hand-out (rm_probe_pool_cull) and the 2^32-input checker of the cheap exact forms (rm_debug_check_math).
//
// Kept out of rm_kernels.hip so that the production translation unit's compile time and code stay as they are.  The variant kernels
// below call the very template functions the render kernels call (sdSceneImpl, sdSceneOne in rm_device.hip.h) with the same
// template arguments; the entry point (rm_queries.hip) validates the request and stages the production SceneBlock, then hands it
// to launch_sdscene_variant.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <string>

#include "rm_device.hip.h"
#include "rm_internal.h"

namespace rm {

__global__ void probe_math_kernel(int fn, const float *x, const float *y, const float *z, float *out, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float a = x[i], b = y ? y[i] : 0.0f, c = z ? z[i] : 0.0f, r = 0.0f;
  switch (fn) {
    case RM_FN_SIN: r = sin_(a); break;
    case RM_FN_COS: r = cos_(a); break;
    case RM_FN_ACOS: r = acos_(a); break;
    case RM_FN_ATAN2: r = atan2_(a, b); break;
    case RM_FN_LOG2: r = log2_(a); break;
    case RM_FN_EXP2: r = exp2_(a); break;
    case RM_FN_POW: r = pow_(a, b); break;
    case RM_FN_SQRT: r = sqrt_(a); break;
    case RM_FN_DIV: r = a / b; break;
    case RM_FN_PNOISE3: r = pnoise(v3(a, b, c)); break;
    case RM_FN_ASIN: r = asin_(a); break;
    case RM_FN_Q16: r = __half2float(__float2half_rn(a)); break;
    case RM_FN_SQRT_FAST: r = sqrt_fast_(a); break;
    case RM_FN_DIVR: r = divr_(a, b); break;
    case RM_FN_RCP: r = rcp_(a); break;
    case RM_FN_SMOOTHSTEP: r = smoothstep_(a, b, c); break;
    case RM_FN_MIN: r = min_(a, b); break;
    case RM_FN_MAX: r = max_(a, b); break;
    case RM_FN_FRACT: r = fract_(a); break;
    case RM_FN_MEDIAN_ABS: r = __builtin_amdgcn_fmed3f(fabs_(a), fabs_(b), fabs_(c)); break;
  }
  out[i] = r;
}

__global__ void probe_sdscene_kernel(const SceneBlock *__restrict__ sb, const float *pts, float *out, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Counters cnt{0, 0, 0, 0, 0, 0};
  SceneMin m = sdScene<0, 0, kTrapShader>(sb, v3(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]), cnt);
  out[4 * i] = m.d;
  out[4 * i + 1] = (float)m.idx;
  out[4 * i + 2] = m.trap.y;
  out[4 * i + 3] = m.trap.z;
}

// bumpGradient, the function behind bumpNormalShared, on the lanes the caller chose: point i on lane i % 64 of wave i / 64 (one
// 64-lane workgroup per wave, lanes past n leave before the call), so its per-sample ballots see exactly those 64 points.
__global__ void __launch_bounds__(64) probe_bump_kernel(const float *pts, float *out, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  float nv, g[3];
  bumpGradient(v3(pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2]), nv, g);
  float *o = out + 4 * (size_t)i;
  o[0] = nv;
  o[1] = g[0];
  o[2] = g[1];
  o[3] = g[2];
}

// The shadow pool's hand-out (shadowPool's PREP form) for shadow origin i and light `light`, beside the forms it replaces: the
// end and `own` of bulbCullEndPrepared from the block's prepared constants, then those of bulbCullEnd with the direction
// normalised on the device, then that direction.  Point i on lane i % 64 of wave i / 64, lanes past n leave first: the plain
// form's fallback for a non-finite origin is a choice of the wave and sees exactly those 64 origins.
template <int BULB>
__global__ void __launch_bounds__(64) probe_pool_cull_kernel(const SceneBlock *__restrict__ sb, int light, float far, const float *pts,
                                                             float *out, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const V3 o = v3(pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2]);
  const LightPrep &q = sb->lightPrep[light];
  const BulbCull cu = bulbCullSetup(sb);
  bool ownP, ownF;
  const float endP = bulbCullEndPrepared<BULB == kBulbPlain>(sb, cu, o, v3(q.pd[0], q.pd[1], q.pd[2]), q.a, far, ownP);
  const RmLight &li = sb->lights[light];
  const V3 L = normalize(v3(-li.dir[0], -li.dir[1], -li.dir[2]));
  const float endF = bulbCullEnd(sb, o, L, far, ownF);
  float *w = out + 8 * (size_t)i;
  w[0] = endP; w[1] = ownP ? 1.0f : 0.0f;
  w[2] = endF; w[3] = ownF ? 1.0f : 0.0f;
  w[4] = L.x; w[5] = L.y; w[6] = L.z; w[7] = 0.0f;
}

namespace {

// One lane per point, one 64-lane workgroup per wave: point i runs on lane i % 64 of wave i / 64, so every wave-uniform
// choice of the evaluator (__ballot) sees exactly the 64 points the caller put there.  Lanes past n leave at once, as finished
// rays do in the march loops: a partial last wave evaluates with its remaining lanes only.
template <int BULB, int COUNT, int TRAP, bool SKIP, bool TRACK, bool ONE>
__global__ void __launch_bounds__(64) probe_variant_kernel(const SceneBlock *__restrict__ sb, const float *pts, const float *ubs,
                                                           float *out, int n, int one) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  Counters cnt{0, 0, 0, 0, 0, 0};
  const V3 p = v3(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]);
  float second = __builtin_inff();
  SceneMin m;
  constexpr unsigned O = optTrap(TRAP) | optIf(SKIP, kSkip) | optIf(TRACK, kTrack);
  if (ONE) m = sdSceneOne<COUNT>(sb, one, p, cnt);
  else m = sdSceneImpl<BULB, COUNT, O>(sb, p, cnt, ubs ? ubs[i] : __builtin_inff(), second);
  float *o = out + 8 * (size_t)i;
  o[0] = m.d;
  o[1] = (float)m.idx;
  o[2] = m.trap.x;
  o[3] = m.trap.y;
  o[4] = m.trap.z;
  o[5] = m.trap.w;
  o[6] = second;
  o[7] = (float)cnt.shapes;
}

using Launch = void (*)(const SceneBlock *, const float *, const float *, float *, int, int, hipStream_t);
template <int BULB, int COUNT, int TRAP, bool SKIP, bool TRACK, bool ONE = false>
void launch(const SceneBlock *sb, const float *pts, const float *ubs, float *out, int n, int one, hipStream_t stream) {
  hipLaunchKernelGGL((probe_variant_kernel<BULB, COUNT, TRAP, SKIP, TRACK, ONE>), dim3((unsigned)((n + 63) / 64)), dim3(64), 0,
                     stream, sb, pts, ubs, out, n, one);
}

// Every combination a production kernel instantiates, found at the call sites: march (sdSceneImpl<BULB, COUNT, the trap unless
// kShadow | kSkip | kTrack> with the last two for SKIP = CULL && !BULB && COUNT != 1, and sdSceneOne<COUNT> on its fast path), getNormal
// and calcAO (sdScene<…, kTrapNone | kSkip>, same SKIP), the hard-shadow pools and the refraction march (no SKIP), the wavefront march (table walk, COUNT 0, TRAP 2
// or 0, SKIP either); the plain bulb form only in the production (COUNT 0) kernels.
struct Variant { int bulbClass, count, trap, skip, track, one; Launch fn; };
const Variant kVariants[] = {
    // table walk
    {0, 0, 0, 0, 0, 0, launch<0, 0, 0, false, false>}, {0, 0, 0, 1, 0, 0, launch<0, 0, 0, true, false>},
    {0, 0, 0, 1, 1, 0, launch<0, 0, 0, true, true>},   {0, 1, 0, 0, 0, 0, launch<0, 1, 0, false, false>},
    {0, 2, 0, 0, 0, 0, launch<0, 2, 0, false, false>}, {0, 2, 0, 1, 0, 0, launch<0, 2, 0, true, false>},
    {0, 2, 0, 1, 1, 0, launch<0, 2, 0, true, true>},
    {0, 0, 1, 0, 0, 0, launch<0, 0, 1, false, false>}, {0, 0, 1, 1, 1, 0, launch<0, 0, 1, true, true>},
    {0, 1, 1, 0, 0, 0, launch<0, 1, 1, false, false>}, {0, 2, 1, 0, 0, 0, launch<0, 2, 1, false, false>},
    {0, 2, 1, 1, 1, 0, launch<0, 2, 1, true, true>},
    {0, 0, 2, 0, 0, 0, launch<0, 0, 2, false, false>}, {0, 0, 2, 1, 0, 0, launch<0, 0, 2, true, false>},
    // the single-Mandelbulb class
    {kBulbGeneral, 0, 0, 0, 0, 0, launch<kBulbGeneral, 0, 0, false, false>},
    {kBulbGeneral, 0, 1, 0, 0, 0, launch<kBulbGeneral, 0, 1, false, false>},
    {kBulbGeneral, 1, 0, 0, 0, 0, launch<kBulbGeneral, 1, 0, false, false>},
    {kBulbGeneral, 1, 1, 0, 0, 0, launch<kBulbGeneral, 1, 1, false, false>},
    {kBulbGeneral, 2, 0, 0, 0, 0, launch<kBulbGeneral, 2, 0, false, false>},
    {kBulbGeneral, 2, 1, 0, 0, 0, launch<kBulbGeneral, 2, 1, false, false>},
    {kBulbPlain, 0, 0, 0, 0, 0, launch<kBulbPlain, 0, 0, false, false>},
    {kBulbPlain, 0, 1, 0, 0, 0, launch<kBulbPlain, 0, 1, false, false>},
    // the march's single-object fast path, in place of the SKIP + TRACK walks above (TRAP plays no part in it)
    {0, 0, 0, 1, 1, 1, launch<0, 0, 0, true, true, true>}, {0, 0, 1, 1, 1, 1, launch<0, 0, 0, true, true, true>},
    {0, 2, 0, 1, 1, 1, launch<0, 2, 0, true, true, true>}, {0, 2, 1, 1, 1, 1, launch<0, 2, 0, true, true, true>},
};

const Variant *find_variant(int bulbClass, int count, int trap, int skip, int track, bool one) {
  for (const Variant &v : kVariants)
    if (v.bulbClass == bulbClass && v.count == count && v.trap == trap && v.skip == skip && v.track == track && v.one == (int)one)
      return &v;
  return nullptr;
}

}  // namespace

bool sdscene_variant_exists(int bulbClass, int count, int trap, int skip, int track, bool one) {
  return find_variant(bulbClass, count, trap, skip, track, one) != nullptr;
}

int launch_sdscene_variant(const void *sb, int bulbClass, int count, int trap, int skip, int track, int one, const float *d_pts,
                           const float *d_ub, float *d_out, int n, hipStream_t stream) {
  const Variant *v = find_variant(bulbClass, count, trap, skip, track, one >= 0);
  if (!v) { set_error("not an instantiated sdScene variant"); return RM_ERR_INVALID_ARGUMENT; }
  v->fn(static_cast<const SceneBlock *>(sb), d_pts, d_ub, d_out, n, one, stream);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { set_error(std::string("probe_variant_kernel: ") + hipGetErrorString(e)); return RM_ERR_DEVICE; }
  return RM_OK;
}

int launch_probe_math(int fn, const float *d_x, const float *d_y, const float *d_z, float *d_out, int n, hipStream_t stream) {
  hipLaunchKernelGGL(probe_math_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, fn, d_x, d_y, d_z, d_out, n);
  HIP_OK(hipGetLastError());
  return RM_OK;
}
int launch_probe_sdscene(const void *sb, const float *d_pts, float *d_out, int n, hipStream_t stream) {
  hipLaunchKernelGGL(probe_sdscene_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, static_cast<const SceneBlock *>(sb), d_pts, d_out, n);
  HIP_OK(hipGetLastError());
  return RM_OK;
}
int launch_probe_pool_cull(const void *sb, int bulbClass, int light, float far, const float *d_pts, float *d_out, int n, hipStream_t stream) {
  const SceneBlock *b = static_cast<const SceneBlock *>(sb);
  const dim3 grid((unsigned)((n + 63) / 64)), block(64);
  if (bulbClass == kBulbPlain) hipLaunchKernelGGL(probe_pool_cull_kernel<kBulbPlain>, grid, block, 0, stream, b, light, far, d_pts, d_out, n);
  else hipLaunchKernelGGL(probe_pool_cull_kernel<kBulbGeneral>, grid, block, 0, stream, b, light, far, d_pts, d_out, n);
  HIP_OK(hipGetLastError());
  return RM_OK;
}
int launch_probe_bump(const float *d_pts, float *d_out, int n, hipStream_t stream) {
  hipLaunchKernelGGL(probe_bump_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, d_pts, d_out, n);
  HIP_OK(hipGetLastError());
  return RM_OK;
}

}  // namespace rm

using namespace rm;

// The cheap exact forms against the IEEE operations for EVERY binary32 input (NaN = NaN): out[0] = inputs where rcp_(y) !=
// 1.0f / y, out[1] = inputs of the fast range 2^-126 <= |y| < 2^126 where the bare v_rcp_f32 + Newton form differs, out[2] =
// inputs where sqrt_fast_(x) != sqrtf(x), out[3] = inputs of sqrt_noscale_'s domain (±0, |x| >= 2^-96, ±inf, NaN)
// where it differs from sqrtf(x), out[4] = inputs where fract_(x) (v_fract_f32) != x − floor(x) kept below 1.  All must be 0.
extern "C" __global__ void check_math_kernel(unsigned long long *out) {
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
  unsigned long long bad = 0, badFast = 0, badSqrt = 0, badNoscale = 0, badFract = 0;
  for (uint64_t u = tid; u < (1ull << 32); u += stride) {
    const float y = u2f((uint32_t)u), ref = 1.0f / y, got = rcp_(y);
    if (f2u(got) != f2u(ref) && !(got != got && ref != ref)) bad++;
    const float ay = fabs_(y);
    if (ay >= 1.17549435e-38f && ay < 8.50705917e37f) {
      const float r = __builtin_amdgcn_rcpf(y), f = rm::fma(rm::fma(-y, r, 1.0f), r, r);
      if (f2u(f) != f2u(ref)) badFast++;
    }
    const float fd = y - __builtin_floorf(y), fref = (fd >= 1.0f) ? 0.99999994f : fd, fg = fract_(y);
    if (f2u(fg) != f2u(fref) && !(fg != fg && fref != fref)) badFract++;
    const float sref = sqrt_(y), sf = sqrt_fast_(y);
    if (f2u(sf) != f2u(sref) && !(sf != sf && sref != sref)) badSqrt++;
    if (!(ay > 0.0f && ay < 1.262177448e-29f)) {
      const float sn = sqrt_noscale_(y);
      if (f2u(sn) != f2u(sref) && !(sn != sn && sref != sref)) badNoscale++;

    }
  }
  if (bad) atomicAdd(&out[0], bad);
  if (badFast) atomicAdd(&out[1], badFast);
  if (badSqrt) atomicAdd(&out[2], badSqrt);
  if (badNoscale) atomicAdd(&out[3], badNoscale);
  if (badFract) atomicAdd(&out[4], badFract);
}

void rm::launch_check_math(unsigned long long *d_out5) { check_math_kernel<<<4096, 256>>>(d_out5); }
