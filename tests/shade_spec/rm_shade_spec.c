/*
 * tests/shade_spec/rm_shade_spec.c — TEST INFRASTRUCTURE.  The specification of rm_shade_rays (include/raymarcher_amd.h), restated
 * with the oracle's OWN static functions.  Nothing under oracle/ changes for this: the file includes the oracle's source, as
 * tests/trace_spec/rm_trace_spec.c does, and restates the oracle's shadePixel from the background colour on (rm_oracle.c: frag:2405-
 * 2419, 2443, 2459-2465, 2481-2574) for a given (ro, rd, far) — getSky, getMoonColor, render, raymarch, getNormal, reflect3,
 * refract3 and brightOf are the oracle's.  The layers (terrain, cloud, sea) are refused by the entry point, so their branches are
 * absent.  tests/test_shade_spec.py pins these lines: on the primary rays of a camera they must equal rmo_render_res in every bit.
 * Built on demand by tests/shade_helpers.py with oracle/Makefile's flags (-ffp-contract=off matters) into _build/.
 */
#include "../../oracle/rm_oracle.c"

static int spec_finite(float v) { return v == v && v - v == 0.0f; }

static void spec_shade_ray(Ctx *c, v3 ro, v3 rd, float far, float *outColor, float *outBright) {
  v4 fragColor, bright = V4(0.0f, 0.0f, 0.0f, 1.0f);
  /* frag:2405-2419 (later #ifdefs override earlier ones) */
  v3 bgCol = V3(0.0f, 0.0f, 0.0f);
  if (c->s.features & RM_FEAT_SKY_BACKGROUND) bgCol = getSky(rd);
  if (c->s.features & RM_FEAT_NIGHTSKY_BACKGROUND) bgCol = getMoonColor(c, rd);
  if (c->s.features & RM_FEAT_WHITE_BACKGROUND) bgCol = V3(1.0f, 1.0f, 1.0f);
  if (c->s.features & RM_FEAT_DARK_BACKGROUND) bgCol = V3(0.0f, 0.0f, 0.0f);

  IntersectionInfo info, oi;
  RenderInfo ri = render(c, ro, rd, &info, OUTSIDE, far, bgCol); /* frag:2443 */
  if (ri.isEnv) {                                                /* frag:2459-2465 */
    fragColor = ri.fragColor;
    goto done;
  }
  {
    v4 phong = ri.fragColor;
    v4 refl = V4(0, 0, 0, 0), refr = V4(0, 0, 0, 0);
    oi = info; /* frag:2481 */
    /* UB5, as the oracle decides it: an emissive hit leaves info.intersectObj = -1; objects[-1] reads as zeros */
    static const RmObject kZeroObject;
    const RmObject *obj = info.intersectObj >= 0 ? &c->objs[info.intersectObj] : &kZeroObject;
    v3 cRefl = V3(obj->cReflective[0], obj->cReflective[1], obj->cReflective[2]);
    v3 cRefr = V3(obj->cTransparent[0], obj->cTransparent[1], obj->cTransparent[2]);
    if (c->s.enableReflection && len3(cRefl) != 0.0f) { /* frag:2491-2524 */
      v3 fil = V3(1.0f, 1.0f, 1.0f);
      for (int i = 0; i < c->s.numReflection; i++) {
        v3 r = reflect3(info.rd, info.n);
        v3 sro = V3(rm_fma(r.x * SURFACE_DIST, 3.0f, info.p.x), rm_fma(r.y * SURFACE_DIST, 3.0f, info.p.y),
                    rm_fma(r.z * SURFACE_DIST, 3.0f, info.p.z));
        fil = v3_mul(fil, cRefl);
        RenderInfo res = render(c, sro, r, &info, OUTSIDE, far, bgCol);
        refl.x += (c->g.ks * fil.x) * res.fragColor.x;
        refl.y += (c->g.ks * fil.y) * res.fragColor.y;
        refl.z += (c->g.ks * fil.z) * res.fragColor.z;
        refl.w += 1.0f;
        if (res.isEnv) break;
      }
    }
    if (c->s.enableRefraction && len3(cRefr) != 0.0f) { /* frag:2526-2570 */
      const RmObject *o2 = &c->objs[oi.intersectObj];
      float ior = o2->ior;
      v3 ct = V3(o2->cTransparent[0], o2->cTransparent[1], o2->cTransparent[2]);
      v3 rdIn = refract3(oi.rd, oi.n, 1.0f / ior);
      v3 pEnter = V3(rm_fma(-(oi.n.x * SURFACE_DIST), 3.0f, oi.p.x), rm_fma(-(oi.n.y * SURFACE_DIST), 3.0f, oi.p.y),
                     rm_fma(-(oi.n.z * SURFACE_DIST), 3.0f, oi.p.z));
      float dIn = raymarch(c, pEnter, rdIn, far, INSIDE).d;
      v3 pExit = v3_madd(rdIn, dIn, pEnter);
      v3 nExit = v3_neg(getNormal(c, pExit));
      v3 rdOut = refract3(rdIn, nExit, ior);
      if (len3(rdOut) != 0.0f) {
        v3 sro = V3(rm_fma(-(nExit.x * SURFACE_DIST), 5.0f, pExit.x), rm_fma(-(nExit.y * SURFACE_DIST), 5.0f, pExit.y),
                    rm_fma(-(nExit.z * SURFACE_DIST), 5.0f, pExit.z));
        RenderInfo res = render(c, sro, rdOut, &info, OUTSIDE, far, bgCol);
        refr.x += (c->g.kt * ct.x) * res.fragColor.x;
        refr.y += (c->g.kt * ct.y) * res.fragColor.y;
        refr.z += (c->g.kt * ct.z) * res.fragColor.z;
        refr.w += 1.0f;
      }
    }
    /* frag:2572-2574 */
    fragColor = V4((phong.x + refl.x) + refr.x, (phong.y + refl.y) + refr.y, (phong.z + refl.z) + refr.z,
                   (phong.w + refl.w) + refr.w);
    bright = brightOf(V3(fragColor.x, fragColor.y, fragColor.z));
  }
done:
  outColor[0] = fragColor.x; outColor[1] = fragColor.y; outColor[2] = fragColor.z; outColor[3] = fragColor.w;
  if (outBright) { outBright[0] = bright.x; outBright[1] = bright.y; outBright[2] = bright.z; outBright[3] = bright.w; }
}

/* rays: n × 8 floats (origin.xyz, unread, dir.xyz, unread); rgba, bright (may be NULL): n × 4 floats.  No camera: `far` is the
 * call's.  The caller passes a call the entry point accepts (no layers, no 2-D mode, samplers where they are read). */
int rmo_spec_shade(const RmObject *objs, int numObjects, const RmLight *lights, int numLights, const RmGlobals *g, const RmSettings *s,
                   const RmResources *resIn, const float *rays, int n, float far, float *rgba, float *bright) {
  if (!g || !s || (numObjects > 0 && !objs) || (numLights > 0 && !lights) || numObjects < 0 || numObjects > RM_MAX_OBJECTS ||
      numLights < 0 || numLights > RM_MAX_LIGHTS || n < 0 || (n > 0 && (!rays || !rgba)) || !(far >= 0.0f) || far - far != 0.0f)
    return RM_ERR_INVALID_ARGUMENT;
  if ((s->features & (RM_FEAT_TERRAIN | RM_FEAT_CLOUD | RM_FEAT_SEA)) || g->isTwoD) return RM_ERR_UNSUPPORTED;
  RmResources none;
  memset(&none, 0, sizeof none);
  const RmResources *res = resIn ? resIn : &none;
  RmCamera cam;
  memset(&cam, 0, sizeof cam);
  cam.initialFar = far;
#pragma omp parallel for schedule(dynamic, 16)
  for (int i = 0; i < n; i++) {
    Ctx c;
    memset(&c, 0, sizeof c);
    c.cam = &cam; c.objs = objs; c.numObjects = numObjects; c.lights = lights; c.numLights = numLights;
    c.g = *g; c.s = *s; c.tex = res->textures; c.numTex = res->numTextures; c.res = res; c.W = 1;
    const float *r = rays + 8 * (size_t)i;
    float *col = rgba + 4 * (size_t)i, *br = bright ? bright + 4 * (size_t)i : NULL;
    const v3 ro = V3(r[0], r[1], r[2]), rd = V3(r[4], r[5], r[6]);
    const int valid = spec_finite(ro.x) && spec_finite(ro.y) && spec_finite(ro.z) && spec_finite(rd.x) && spec_finite(rd.y) &&
                      spec_finite(rd.z) && (rd.x != 0.0f || rd.y != 0.0f || rd.z != 0.0f);
    if (!valid) {
      for (int k = 0; k < 4; k++) { col[k] = 0.0f; if (br) br[k] = 0.0f; }
      continue;
    }
    spec_shade_ray(&c, ro, rd, far, col, br);
  }
  return RM_OK;
}
