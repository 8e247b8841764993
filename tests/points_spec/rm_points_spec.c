/*
 * tests/points_spec/rm_points_spec.c — TEST INFRASTRUCTURE.  The specification of rm_shade_points (include/raymarcher_amd.h), restated
 * with the oracle's OWN static functions.  Nothing under oracle/ changes for this: the file includes the oracle's source, as
 * tests/shade_spec/rm_shade_spec.c does.  sdScene, getNormal, bumpNormal, calcAO, getPhong, v3_madd, dot3 and the palette lines of
 * render (rm_oracle.c: frag:2337-2375) are the oracle's; what is written here is the order the header gives them: validity,
 * projection, the evaluation at the point, the normal, AO, render from behind its march.  tests/test_points_spec.py ties it to what
 * is already pinned: at the hit points of a camera's rays it must give the shade spec's colour and the trace spec's normal.
 * Built on demand by helpers.load_spec with oracle/Makefile's flags (-ffp-contract=off matters) into _build/.
 */
#include "../../oracle/rm_oracle.c"

static int spec_finite(float v) { return v == v && v - v == 0.0f; }

/* surface: 8 floats (normal, distance | position, objectId bits), ao: 1 float, rgba: 4 floats; each may be NULL */
static void spec_shade_point(Ctx *c, v3 p, const v3 *view, float far, float iso, float maxMove, int projectSteps, float *surface,
                             float *ao, float *rgba) {
  const v3 p0 = p;
  const float move2 = maxMove * maxMove;
  for (int k = 0; k < projectSteps; k++) { /* step 2 */
    SceneMin sc = sdScene(c, p);
    if (sc.minObjIdx == -1) break;
    float e = sc.minD - iso;
    v3 N = getNormal(c, p);
    v3 q = v3_madd(N, -e, p);
    if (!(spec_finite(q.x) && spec_finite(q.y) && spec_finite(q.z))) break;
    v3 m = v3_sub(q, p0);
    if (!(dot3(m, m) <= move2)) break;
    p = q;
  }
  SceneMin sc = sdScene(c, p); /* step 3 */
  v3 N = V3(0.0f, 0.0f, 0.0f);
  float aoV = 0.0f;
  v4 col = V4(0.0f, 0.0f, 0.0f, 0.0f);
  if (sc.minObjIdx != -1) {
    N = getNormal(c, p); /* step 4 */
    if (c->s.features & RM_FEAT_PERLIN_BUMP) N = bumpNormal(N, p, 10.0f, 2.0f);
    if (ao) aoV = calcAO(c, p, N); /* step 5 */
    if (rgba) {                    /* step 6: render() from behind its march, rm_oracle.c's lines */
      const v3 rd = view ? *view : v3_neg(N);
      const RmObject *obj = &c->objs[sc.minObjIdx];
      v3 cc;
      if (obj->isEmissive) {
        cc = V3(obj->color[0], obj->color[1], obj->color[2]);
      } else if (obj->type == RM_MANDELBULB) {
        cc = V3(0.2f, 0.2f, 0.2f);
        cc = mix3(cc, V3(0.10f, 0.20f, 0.30f), rm_clamp(sc.trap.y, 0.0f, 1.0f));
        cc = mix3(cc, V3(0.02f, 0.10f, 0.30f), rm_clamp(sc.trap.z * sc.trap.z, 0.0f, 1.0f));
        cc = mix3(cc, V3(0.30f, 0.10f, 0.02f), rm_clamp(rm_pow(sc.trap.w, 6.0f), 0.0f, 1.0f));
        cc = v3_scale(cc, 0.5f);
        v3 ph = getPhong(c, N, sc.minObjIdx, p, rd, far);
        cc = V3(cc.x * (ph.x * 8.0f), cc.y * (ph.y * 8.0f), cc.z * (ph.z * 8.0f));
      } else if (obj->type == RM_MENGERSPONGE) {
        cc = V3(rm_fma(0.5f, rm_cos(rm_fma(2.0f, sc.trap.z, 0.0f)), 0.5f), rm_fma(0.5f, rm_cos(rm_fma(2.0f, sc.trap.z, 1.0f)), 0.5f),
                rm_fma(0.5f, rm_cos(rm_fma(2.0f, sc.trap.z, 2.0f)), 0.5f));
        cc = v3_mul(cc, getPhong(c, N, sc.minObjIdx, p, rd, far));
      } else {
        cc = getPhong(c, N, sc.minObjIdx, p, rd, far);
      }
      col = V4(cc.x, cc.y, cc.z, 1.0f);
    }
  }
  if (surface) {
    surface[0] = N.x; surface[1] = N.y; surface[2] = N.z; surface[3] = sc.minD;
    surface[4] = p.x; surface[5] = p.y; surface[6] = p.z;
    memcpy(&surface[7], &sc.minObjIdx, 4);
  }
  if (ao) *ao = aoV;
  if (rgba) { rgba[0] = col.x; rgba[1] = col.y; rgba[2] = col.z; rgba[3] = col.w; }
}

/* points, view (may be NULL): n × 4 floats (w unread); surface: n × 8 floats, ao: n floats, rgba: n × 4 floats, each may be NULL.
 * The caller passes a call the entry point accepts (no layers, no 2-D mode, samplers where they are read). */
int rmo_spec_points(const RmObject *objs, int numObjects, const RmLight *lights, int numLights, const RmGlobals *g, const RmSettings *s,
                    const RmResources *resIn, const float *points, const float *view, int n, float far, float iso, float maxMove,
                    int projectSteps, float *surface, float *ao, float *rgba) {
  if (!g || !s || (numObjects > 0 && !objs) || (numLights > 0 && !lights) || numObjects < 0 || numObjects > RM_MAX_OBJECTS ||
      numLights < 0 || numLights > RM_MAX_LIGHTS || n < 0 || (n > 0 && !points) || !(far >= 0.0f) || far - far != 0.0f ||
      !spec_finite(iso) || !(maxMove >= 0.0f) || projectSteps < 0 || projectSteps > RM_MAX_PROJECT_STEPS || (!surface && !ao && !rgba))
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
    const float *pt = points + 4 * (size_t)i, *vw = view ? view + 4 * (size_t)i : NULL;
    float *sf = surface ? surface + 8 * (size_t)i : NULL, *a = ao ? ao + i : NULL, *col = rgba ? rgba + 4 * (size_t)i : NULL;
    const v3 p = V3(pt[0], pt[1], pt[2]);
    v3 rd = V3(0.0f, 0.0f, 0.0f);
    int valid = spec_finite(p.x) && spec_finite(p.y) && spec_finite(p.z);
    if (vw) {
      rd = V3(vw[0], vw[1], vw[2]);
      valid = valid && spec_finite(rd.x) && spec_finite(rd.y) && spec_finite(rd.z) && (rd.x != 0.0f || rd.y != 0.0f || rd.z != 0.0f);
    }
    if (!valid) {
      if (sf) {
        const int32_t bad = RM_RAY_INVALID;
        for (int k = 0; k < 7; k++) sf[k] = 0.0f;
        memcpy(&sf[7], &bad, 4);
      }
      if (a) *a = 0.0f;
      if (col) for (int k = 0; k < 4; k++) col[k] = 0.0f;
      continue;
    }
    spec_shade_point(&c, p, vw ? &rd : NULL, far, iso, maxMove, projectSteps, sf, a, col);
  }
  return RM_OK;
}
