// rm_indirect.hip.h — the device code of rm_shade_rays_indirect and rm_light_probes_indirect (gfx950 only): shadeRay with the
// diffuse term of a light grid added at the primary hit (include/raymarcher_amd.h has the definition).  render() and shadePixel()
// (rm_device.hip.h) hand out neither the hit's diffuse colour nor the march's orbit trap, and a new option on them would touch every
// kernel that instantiates them; so this header COMPOSES their parts — march, renderPooled, getNormal, getDiffuse, getPhong,
// render() itself for the secondary rays — in render()'s and shadePixel()'s own order with the very template arguments shadeRay
// gives them, and rm_device.hip.h stays as it is: the code object of every other translation unit is byte-identical.
// The colour is shade_rays_kernel's in every word because every operation behind a ray is one of those functions' and none is
// fused (-ffp-contract=off).
//   Where the term is computed.  Behind getPhong (behind renderPooled in the pooled bulb classes): the hit point and the bumped normal
// are alive there anyway — render() hands them on in Hit — and so are the material's diffuse colour (getPhong reads it) and the
// trap (the palette reads it), so the grid lookup adds no word to what is alive across the shadow marches.  From there three words
// and a flag, the finished term, wait across the secondary rays for the one addition; the lookup's inputs (p, n, dif, trap: thirteen
// words) do not.
//   The grid is read through rm_light_grid.h's grid_light / grid_light_visible, the code of rm_light_grid_irradiance and of its
// _visible form; the arithmetic behind it is rm_indirect.h's.  The layers are refused by the launchers, so envLayers is not
// compiled: the ENV classes here are the sky backgrounds alone.
#pragma once
#include "rm_device.hip.h"
#include "rm_indirect.h"
#include "rm_light_grid.h"

namespace rm {

// The grid of a call, by value in the kernel's arguments: the two kinds of records where the bakes stored them (depths null: the
// plain lookup), the box, k = strength · RM_INV_PI, the lookup's flags and bias.  The loaders are rm_light_grid.hip's and
// rm_light_grid_visible.hip's: hits one dword, a coefficient one 16-byte load, a texel's moments one 8-byte load, 64-bit offsets.
struct IndirectGrid {
  const char *probes, *depths;
  lg::Grid G;
  float k;
  unsigned flags;
  float normalBias;
  __host__ __device__ int hits(size_t i) const { return *reinterpret_cast<const int32_t *>(probes + i * 160u + 144u); }
  __host__ __device__ void sh(size_t i, int j, float out[4]) const {
    const float4 v = *reinterpret_cast<const float4 *>(probes + i * 160u + 16u * (size_t)j);
    out[0] = v.x, out[1] = v.y, out[2] = v.z, out[3] = v.w;
  }
  __host__ __device__ void depth(size_t i, int texel, float out[2]) const {
    const float2 v = *reinterpret_cast<const float2 *>(depths + i * 512u + 8u * (size_t)texel);
    out[0] = v.x, out[1] = v.y;
  }
};
static_assert(sizeof(RmLightProbe) == 160 && offsetof(RmLightProbe, hits) == 144 && sizeof(RmProbeDepth) == 512, "the loaders' offsets");

// The finished term of a ray: on = false where the definition has none, and then nothing is added.
struct IndirectTerm { float ind[3]; bool on; };

// The term at the hit (p, n) of an object of `type` with the diffuse colour dif and the primary march's trap.
RM_DEV void gridTerm(const IndirectGrid &grid, int type, V3 p, V3 n, V3 dif, V4 trap, IndirectTerm &t) {
  const float pp[3] = {p.x, p.y, p.z}, nn[3] = {n.x, n.y, n.z};
  const lg::GridLight r = grid.depths ? lg::grid_light_visible(grid.G, pp, nn, grid.flags, grid.normalBias, grid)  // wave-uniform
                                      : lg::grid_light(grid.G, pp, nn, grid.flags, grid);
  if (r.probes <= 0) return;
  const float d[3] = {dif.x, dif.y, dif.z};
  float x[3], c[3] = {0.0f, 0.0f, 0.0f};
  ind::diffuse_term(d, r.e, grid.k, x);
  int palette = ind::kPlain;
  if (type == RM_MANDELBULB) {  // render()'s palettes (frag:2354-2365)
    const V3 cc = bulbTrapColor(trap.y, trap.z, trap.w);
    c[0] = cc.x, c[1] = cc.y, c[2] = cc.z;
    palette = ind::kBulb;
  } else if (type == RM_MENGERSPONGE) {
    c[0] = fma(0.5f, cos_(fma(2.0f, trap.z, 0.0f)), 0.5f);
    c[1] = fma(0.5f, cos_(fma(2.0f, trap.z, 1.0f)), 0.5f);
    c[2] = fma(0.5f, cos_(fma(2.0f, trap.z, 2.0f)), 0.5f);
    palette = ind::kSponge;
  }
  ind::apply_palette(palette, c, x, t.ind);
  t.on = true;
}

// render() for the primary ray of shadeRay — COUNT = 0, no light split, side = 1 — statement for statement, with the term formed
// behind getPhong / renderPooled.  O: render()'s kTex | kCull | kPool | kShareBump | kPrep.
template <int BULB, unsigned O>
RM_DEV RenderOut renderIndirect(const SceneBlock *sb, const RmObject *objs, V3 ro, V3 rd, Hit &info, float maxT, V3 bg, Counters &cnt,
                                const IndirectGrid &grid, IndirectTerm &term) {
  static_assert(optOnly(O, kTex | kCull | kPool | kShareBump | kPrep), "renderIndirect: an option it does not take");
  constexpr bool TEX = (O & kTex) != 0, CULLS = (O & kCull) != 0, POOL = (O & kPool) != 0, PREP = (O & kPrep) != 0;
  RenderOut out;
  info.obj = -1;
  term.on = false;
  const MarchRes res = march<BULB, 0, (O & kCull) | optIf(POOL && kBulbScalarLoop<BULB, PREP>, kScalar)>(sb, ro, rd, maxT, 1.0f, cnt);
  if (POOL && hardDirectionalOnly(sb)) {
    out = renderPooled<BULB, 0, O & (kShareBump | kPrep)>(sb, objs, ro, rd, res, info, maxT, bg, cnt);
    // the pool's classes have no textures and no emissive object; info holds the hit's p and N
    if (res.obj != -1) gridTerm(grid, RM_MANDELBULB, info.p, info.n, getDiffuse<false>(sb, objs[0], info.p), res.trap, term);
    return out;
  }
  if (res.obj == -1) {
    out.col = (TEX && sb->s.enableSkyBox) ? sampleCube(sb->skybox, rd) : bg;
    out.isEnv = 1;
    out.d = maxT;
    return out;
  }
  out.isEnv = 0;
  out.d = res.d;
  V3 p = madd(rd, res.d, ro);
  constexpr bool SKIP = CULLS && !BULB;
  float ubP = __builtin_inff();
  if (SKIP) {
    const float lipLen = (sb->cullLip * len(rd)) * 1.0001f;
    ubP = fma(kSurfaceDist, lipLen, kSurfaceDist) * 1.001f + fma(fabs_(res.d), 1.0e-6f, 1.0e-5f);
  }
  V3 pn = getNormal<BULB, 0, optIf(SKIP, kSkip)>(sb, p, cnt, SKIP ? fma(0.0005f, sb->cullLip * 1.001f, ubP) : ubP);
  if (sb->s.features & RM_FEAT_PERLIN_BUMP) pn = bumpNormal(pn, p);
  const RmObject &o = objs[BULB ? 0 : res.obj];
  if (TEX && o.isEmissive) {  // no term; info.obj stays -1
    out.col = v3(o.color[0], o.color[1], o.color[2]);
    return out;
  }
  Material mat;
  mat.amb = v3(o.cAmbient[0], o.cAmbient[1], o.cAmbient[2]);
  mat.dif = getDiffuse<TEX>(sb, o, p);
  mat.spec = v3(o.cSpecular[0], o.cSpecular[1], o.cSpecular[2]);
  mat.shininess = o.shininess;
  const int type = BULB ? (int)RM_MANDELBULB : o.type;
  V3 ph = getPhong<BULB, 0, optIf(TEX, kRes) | (O & kCull)>(sb, objs, mat, pn, p, rd, maxT, cnt, ubP, LightSplit{-1, nullptr, 0});
  V3 col = ph;
  if (type == RM_MANDELBULB) {
    V3 c = bulbTrapColor(res.trap.y, res.trap.z, res.trap.w);
    col = v3(c.x * (ph.x * 8.0f), c.y * (ph.y * 8.0f), c.z * (ph.z * 8.0f));
  } else if (type == RM_MENGERSPONGE) {
    V3 c = v3(fma(0.5f, cos_(fma(2.0f, res.trap.z, 0.0f)), 0.5f), fma(0.5f, cos_(fma(2.0f, res.trap.z, 1.0f)), 0.5f),
              fma(0.5f, cos_(fma(2.0f, res.trap.z, 2.0f)), 0.5f));
    col = mul(c, ph);
  }
  gridTerm(grid, type, p, pn, mat.dif, res.trap, term);
  info.p = p; info.n = pn; info.rd = rd; info.obj = res.obj;
  out.col = col;
  return out;
}

// shadeRay (shadePixel's ray part with kRay | kShareBump | kPrep, COUNT = 0, no split, no layers) for the ray (ro, rd), with
// the term of `grid` added to the finished colour: fragColor.rgb + ind, one addition per channel, where the ray has a term.
// O: shadeRay's class bits, optClass(ENV, TEX, SEC).
template <int BULB, unsigned O>
RM_DEV void shadeRayIndirect(const SceneBlock *sb, const RmObject *objs, V3 ro, V3 rd, const IndirectGrid &grid, V4 &fragColor,
                             bool &hitFlag) {
  static_assert(optOnly(O, kEnv | kTex | kSec), "shadeRayIndirect: an option it does not take");
  constexpr bool ENV = (O & kEnv) != 0, TEX = (O & kTex) != 0, SEC = (O & kSec) != 0;
  Counters cnt{0, 0, 0, 0, 0, 0};
  hitFlag = false;
  const V3 bg = ENV ? backgroundColor(sb, rd) : backgroundColor(sb);
  const float far = sb->cam.initialFar;  // the launchers refuse RM_FEAT_CLOUD
  Hit info;
  IndirectTerm term;
  constexpr bool POOL = BULB && !ENV && !TEX;
  RenderOut ri = renderIndirect<BULB, (O & kTex) | kShareBump | kPrep | optIf(!ENV, kCull) | optIf(POOL, kPool)>(sb, objs, ro, rd, info, far,
                                                                                                              bg, cnt, grid, term);
  if (ri.isEnv) {
    fragColor = v4(ri.col.x, ri.col.y, ri.col.z, 1.0f);
    return;
  }
  hitFlag = true;
  V4 phong = v4(ri.col.x, ri.col.y, ri.col.z, 1.0f);
  V4 refl = v4(0.0f, 0.0f, 0.0f, 0.0f), refr = v4(0.0f, 0.0f, 0.0f, 0.0f);
  const Hit oi = info;
  const bool noObj = TEX && info.obj < 0;
  const RmObject &o = objs[(BULB || noObj) ? 0 : info.obj];
  const V3 cRefl = noObj ? v3(0.0f, 0.0f, 0.0f) : v3(o.cReflective[0], o.cReflective[1], o.cReflective[2]);
  const V3 cRefr = noObj ? v3(0.0f, 0.0f, 0.0f) : v3(o.cTransparent[0], o.cTransparent[1], o.cTransparent[2]);
  const float ior = o.ior;
  if (SEC && sb->s.enableReflection && len(cRefl) != 0.0f) {
    V3 fil = v3(1.0f, 1.0f, 1.0f);
    const int nb = sb->s.numReflection;
    for (int i = 0; i < nb; i++) {
      V3 r = reflect(info.rd, info.n);
      V3 sro = v3(fma(r.x * kSurfaceDist, 3.0f, info.p.x), fma(r.y * kSurfaceDist, 3.0f, info.p.y),
                  fma(r.z * kSurfaceDist, 3.0f, info.p.z));
      fil = mul(fil, cRefl);
      RenderOut res = render<BULB, 0, (O & kTex) | optIf(!ENV, kCull)>(sb, objs, sro, r, info, 1.0f, far, bg, cnt);
      refl.x += (sb->g.ks * fil.x) * res.col.x;
      refl.y += (sb->g.ks * fil.y) * res.col.y;
      refl.z += (sb->g.ks * fil.z) * res.col.z;
      refl.w += 1.0f;
      if (res.isEnv) break;
    }
  }
  if (SEC && sb->s.enableRefraction && len(cRefr) != 0.0f) {
    V3 rdIn = refract(oi.rd, oi.n, 1.0f / ior);
    V3 pEnter = v3(fma(-(oi.n.x * kSurfaceDist), 3.0f, oi.p.x), fma(-(oi.n.y * kSurfaceDist), 3.0f, oi.p.y),
                   fma(-(oi.n.z * kSurfaceDist), 3.0f, oi.p.z));
    float dIn = march<BULB, 0>(sb, pEnter, rdIn, far, -1.0f, cnt).d;
    V3 pExit = madd(rdIn, dIn, pEnter);
    V3 nExit = neg(getNormal<BULB, 0>(sb, pExit, cnt));
    V3 rdOut = refract(rdIn, nExit, ior);
    if (len(rdOut) != 0.0f) {
      V3 sro = v3(fma(-(nExit.x * kSurfaceDist), 5.0f, pExit.x), fma(-(nExit.y * kSurfaceDist), 5.0f, pExit.y),
                  fma(-(nExit.z * kSurfaceDist), 5.0f, pExit.z));
      RenderOut res = render<BULB, 0, (O & kTex) | optIf(!ENV, kCull)>(sb, objs, sro, rdOut, info, 1.0f, far, bg, cnt);
      refr.x += (sb->g.kt * cRefr.x) * res.col.x;
      refr.y += (sb->g.kt * cRefr.y) * res.col.y;
      refr.z += (sb->g.kt * cRefr.z) * res.col.z;
      refr.w += 1.0f;
    }
  }
  fragColor = v4((phong.x + refl.x) + refr.x, (phong.y + refl.y) + refr.y, (phong.z + refl.z) + refr.z, (phong.w + refl.w) + refr.w);
  if (term.on) {
    fragColor.x = fragColor.x + term.ind[0];
    fragColor.y = fragColor.y + term.ind[1];
    fragColor.z = fragColor.z + term.ind[2];
  }
}

}  // namespace rm
