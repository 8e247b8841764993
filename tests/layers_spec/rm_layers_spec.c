/*
 * tests/layers_spec/rm_layers_spec.c — TEST INFRASTRUCTURE.  The specification of rm_shade_rays_layers and rm_trace_rays_layers
 * (include/raymarcher_amd.h), restated with the oracle's OWN static functions.  Nothing under oracle/ changes for this: the file
 * includes the oracle's source, as tests/shade_spec/rm_shade_spec.c does.
 * rmo_spec_shade_layers is the oracle's shadePixel from the background colour on (rm_oracle.c: frag:2405-2426, 2443-2475,
 * 2481-2574) for a given (ro, rd, far, imageWidth): render, envLayers, reflect3, refract3, raymarch, getNormal and brightOf are the
 * oracle's, and c->W = imageWidth is what its seaRender divides the normal's epsilon by.  tests/test_layers_spec.py pins these
 * lines: on the primary rays of a camera with imageWidth = W they must equal rmo_render_res in every bit.
 * rmo_spec_trace_layers does not restate the two layer marches: whether the sea and the terrain are hit, and where along the ray,
 * are the return value and dOut of the oracle's own seaRender and terrainRender; only position and normal are written out here,
 * with the oracle's seaMapHeight, getSeaNormal, v3_madd and terrainNormal.
 * Built on demand by tests/layers_helpers.py with oracle/Makefile's flags (-ffp-contract=off matters) into _build/.
 */
#include "../../oracle/rm_oracle.c"

#define SPEC_TRACE_NO_NORMAL 1u
#define SPEC_TRACE_OCCLUSION 2u
#define SPEC_RAY_INVALID (-2)
#define SPEC_HIT_SEA (-3)
#define SPEC_HIT_TERRAIN (-4)
#define SPEC_LAYER_BITS (RM_FEAT_TERRAIN | RM_FEAT_CLOUD | RM_FEAT_SEA)

static int spec_finite(float v) { return v == v && v - v == 0.0f; }
static int spec_valid(v3 ro, v3 rd) {
  return spec_finite(ro.x) && spec_finite(ro.y) && spec_finite(ro.z) && spec_finite(rd.x) && spec_finite(rd.y) && spec_finite(rd.z) &&
         (rd.x != 0.0f || rd.y != 0.0f || rd.z != 0.0f);
}

static void spec_shade_layers_ray(Ctx *c, v3 ro, v3 rd, float *outColor, float *outBright) {
  v4 fragColor, bright = V4(0.0f, 0.0f, 0.0f, 1.0f);
  /* frag:2405-2419 (later #ifdefs override earlier ones) */
  v3 bgCol = V3(0.0f, 0.0f, 0.0f);
  if (c->s.features & RM_FEAT_SKY_BACKGROUND) bgCol = getSky(rd);
  if (c->s.features & RM_FEAT_NIGHTSKY_BACKGROUND) bgCol = getMoonColor(c, rd);
  if (c->s.features & RM_FEAT_WHITE_BACKGROUND) bgCol = V3(1.0f, 1.0f, 1.0f);
  if (c->s.features & RM_FEAT_DARK_BACKGROUND) bgCol = V3(0.0f, 0.0f, 0.0f);
  const int env = (c->s.features & SPEC_LAYER_BITS) != 0;
  float far = (c->s.features & RM_FEAT_CLOUD) ? 2000.0f : c->cam->initialFar; /* frag:2422-2426 */

  IntersectionInfo info, oi;
  RenderInfo ri = render(c, ro, rd, &info, OUTSIDE, far, bgCol); /* frag:2443 */
  int terrainHit = 0, cloudHit = 0, seaHit = 0;
  v3 tcol = bgCol, ccol = bgCol, scol = bgCol;
  if (env) envLayers(c, ro, rd, ri.d, bgCol, &terrainHit, &cloudHit, &seaHit, &tcol, &ccol, &scol); /* frag:2444-2456 */
  if (ri.isEnv && !cloudHit && !terrainHit && !seaHit) { /* frag:2459-2465 */
    fragColor = ri.fragColor;
    goto done;
  } else if (cloudHit) { /* frag:2466-2468 */
    fragColor = V4(ccol.x, ccol.y, ccol.z, 1.0f);
    bright = brightOf(ccol);
    goto done;
  } else if (terrainHit) { /* frag:2469-2471 */
    fragColor = V4(tcol.x, tcol.y, tcol.z, 1.0f);
    bright = brightOf(tcol);
    goto done;
  } else if (seaHit) { /* frag:2472-2474 */
    fragColor = V4(scol.x, scol.y, scol.z, 1.0f);
    bright = brightOf(scol);
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
        if (env) { /* frag:2506-2518: terrain and cloud end the loop, the sea does not */
          int th, ch, sh; v3 tc, cc, sc;
          envLayers(c, sro, r, res.d, bgCol, &th, &ch, &sh, &tc, &cc, &sc);
          if (sh) res.fragColor = V4(sc.x, sc.y, sc.z, 1.0f);
          if (th) { res.fragColor = V4(tc.x, tc.y, tc.z, 1.0f); res.isEnv = 1; }
          if (ch) { res.fragColor = V4(cc.x, cc.y, cc.z, 1.0f); res.isEnv = 1; }
        }
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
        if (env) { /* frag:2555-2567 */
          int th, ch, sh; v3 tc, cc, sc;
          envLayers(c, sro, rdOut, res.d, bgCol, &th, &ch, &sh, &tc, &cc, &sc);
          if (sh) res.fragColor = V4(sc.x, sc.y, sc.z, 1.0f);
          if (th) res.fragColor = V4(tc.x, tc.y, tc.z, 1.0f);
          if (ch) res.fragColor = V4(cc.x, cc.y, cc.z, 1.0f);
        }
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
 * call's and imageWidth stands for the frame's W.  The caller passes a call the entry point accepts (no 2-D mode, samplers where
 * they are read). */
int rmo_spec_shade_layers(const RmObject *objs, int numObjects, const RmLight *lights, int numLights, const RmGlobals *g,
                          const RmSettings *s, const RmResources *resIn, const float *rays, int n, float far, int imageWidth,
                          float *rgba, float *bright) {
  if (!g || !s || (numObjects > 0 && !objs) || (numLights > 0 && !lights) || numObjects < 0 || numObjects > RM_MAX_OBJECTS ||
      numLights < 0 || numLights > RM_MAX_LIGHTS || n < 0 || (n > 0 && (!rays || !rgba)) || !(far >= 0.0f) || far - far != 0.0f ||
      imageWidth < 1)
    return RM_ERR_INVALID_ARGUMENT;
  if (g->isTwoD) return RM_ERR_UNSUPPORTED;
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
    c.g = *g; c.s = *s; c.tex = res->textures; c.numTex = res->numTextures; c.res = res; c.W = imageWidth;
    const float *r = rays + 8 * (size_t)i;
    float *col = rgba + 4 * (size_t)i, *br = bright ? bright + 4 * (size_t)i : NULL;
    const v3 ro = V3(r[0], r[1], r[2]), rd = V3(r[4], r[5], r[6]);
    if (!spec_valid(ro, rd)) {
      for (int k = 0; k < 4; k++) { col[k] = 0.0f; if (br) br[k] = 0.0f; }
      continue;
    }
    spec_shade_layers_ray(&c, ro, rd, col, br);
  }
  return RM_OK;
}

/* rays: n × 8 floats (origin.xyz, tMax, dir.xyz, unused); hits: n × 8 words (normal.xyz, t, position.xyz, objectId as int32).
 * mode: 0 closest, 1 closest without normals, 2 occlusion (only without a layer bit).  The oracle's seaRender also shades the sea,
 * which reads the noise sampler; its hit flag and distance do not, so a one-texel sampler of this file stands in. */
int rmo_spec_trace_layers(const RmObject *objs, int numObjects, const RmGlobals *g, const RmSettings *s, const float *rays, int n,
                          int imageWidth, unsigned mode, float *hits) {
  if (!g || !s || (numObjects > 0 && !objs) || numObjects < 0 || numObjects > RM_MAX_OBJECTS || n < 0 || (n > 0 && (!rays || !hits)) ||
      mode > 2u || imageWidth < 1)
    return RM_ERR_INVALID_ARGUMENT;
  if (mode == SPEC_TRACE_OCCLUSION && (s->features & SPEC_LAYER_BITS)) return RM_ERR_UNSUPPORTED;
  static const uint8_t texel[4] = {0, 0, 0, 0};
  RmResources stand;
  memset(&stand, 0, sizeof stand);
  stand.noise.pixels = texel; stand.noise.width = 1; stand.noise.height = 1;
  RmCamera cam;
  memset(&cam, 0, sizeof cam);
#pragma omp parallel for schedule(dynamic, 16)
  for (int i = 0; i < n; i++) {
    Ctx c;
    memset(&c, 0, sizeof c);
    c.cam = &cam; c.objs = objs; c.numObjects = numObjects; c.lights = NULL; c.numLights = 0;
    c.g = *g; c.s = *s; c.tex = NULL; c.numTex = 0; c.res = &stand; c.W = imageWidth;
    const float *r = rays + 8 * (size_t)i;
    float *h = hits + 8 * (size_t)i;
    const v3 ro = V3(r[0], r[1], r[2]), rd = V3(r[4], r[5], r[6]);
    const float tMax = r[3];
    v3 nrm = V3(0.0f, 0.0f, 0.0f), p = V3(0.0f, 0.0f, 0.0f);
    float t = 0.0f;
    int32_t id = SPEC_RAY_INVALID;
    const int valid = spec_valid(ro, rd) && tMax >= 0.0f;
    if (valid && mode == SPEC_TRACE_OCCLUSION) {
      RayMarchRes sh = softshadow(&c, ro, rd, 0.0f, tMax, 8.0f);
      id = sh.intersectObj;
      t = sh.d;
    } else if (valid) {
      RayMarchRes res = raymarch(&c, ro, rd, tMax, OUTSIDE);
      const float d0 = res.intersectObj != -1 ? res.d : tMax;
      const v3 bg = V3(0.0f, 0.0f, 0.0f);
      v3 col;
      float d1 = d0, d2 = d0;
      int seaHit = 0, terrainHit = 0;
      if (c.s.features & RM_FEAT_SEA) seaHit = seaRender(&c, ro, rd, d0, bg, &col, &d1);
      d2 = d1;
      if (c.s.features & RM_FEAT_TERRAIN) terrainHit = terrainRender(&c, ro, rd, d1, bg, &col, &d2);
      if (terrainHit) {
        id = SPEC_HIT_TERRAIN;
        t = d2;
        if (mode != SPEC_TRACE_NO_NORMAL) {
          p = v3_madd(rd, d2, ro);
          nrm = terrainNormal(p.x, p.z);
        }
      } else if (seaHit) {
        id = SPEC_HIT_SEA;
        t = d1;
        if (mode != SPEC_TRACE_NO_NORMAL) {
          seaMapHeight(&c, ro, rd, &p, d0);
          v3 d = v3_sub(p, ro);
          nrm = getSeaNormal(&c, p, (dot3(d, d) * 0.1f) / (float)imageWidth);
        }
      } else { /* rm_trace_rays' closest hit or miss */
        id = res.intersectObj;
        t = tMax;
        if (res.intersectObj != -1) {
          t = res.d;
          if (mode != SPEC_TRACE_NO_NORMAL) {
            p = v3_madd(rd, res.d, ro);
            nrm = getNormal(&c, p);
            if (c.s.features & RM_FEAT_PERLIN_BUMP) nrm = bumpNormal(nrm, p, 10.0f, 2.0f);
          }
        }
      }
    }
    h[0] = nrm.x; h[1] = nrm.y; h[2] = nrm.z; h[3] = t;
    h[4] = p.x; h[5] = p.y; h[6] = p.z;
    memcpy(&h[7], &id, 4);
  }
  return RM_OK;
}
