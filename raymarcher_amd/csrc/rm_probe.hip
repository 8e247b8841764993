// rm_probe.hip — test-only device probe of the scene evaluator's production instantiations (rm_probe_sdscene_variant).
//
// Kept out of rm_kernels.hip so that the production translation unit's compile time and code stay as they are.  The kernels
// below call the very template functions the render kernels call (sdSceneImpl, sdSceneOne in rm_device.hip.h) with the same
// template arguments; the launcher (rm_kernels.hip) validates the request and stages the production SceneBlock, then hands it
// to launch_sdscene_variant.
#include <hip/hip_runtime.h>

#include <string>

#include "rm_device.hip.h"
#include "rm_internal.h"

namespace rm {
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
  if (ONE) m = sdSceneOne<COUNT>(sb, one, p, cnt);
  else m = sdSceneImpl<BULB, COUNT, TRAP, SKIP, TRACK>(sb, p, cnt, ubs ? ubs[i] : __builtin_inff(), second);
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

// Every combination a production kernel instantiates, found at the call sites: march (sdSceneImpl<BULB, COUNT, !SHADOW, SKIP,
// SKIP> with SKIP = CULL && !BULB && COUNT != 1, and sdSceneOne<COUNT> on its fast path), getNormal and calcAO (sdScene<…, 0,
// SKIP>, same SKIP), the hard-shadow pools and the refraction march (no SKIP), the wavefront march (table walk, COUNT 0, TRAP 2
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

}  // namespace rm
