/*
 * tests/gbuffer_spec/rm_gbuffer_spec.c — TEST INFRASTRUCTURE.  The specification of rm_render_gbuffer (include/raymarcher_amd.h):
 * the RayMarchRes / IntersectionInfo of main's first render() call, restated with the oracle's OWN static functions.  The oracle
 * (oracle/rm_oracle.c) exposes hits only through colour, and nothing under oracle/ changes for this: the file includes the
 * oracle's source, as oracle/rm_oracle_f64.c does, and adds one function that calls rayPlanes, interpolateVarying, normalize3,
 * raymarch, getNormal, bumpNormal and v3_madd exactly as shadePixel and render call them (frag:2388-2392, 2443, 2318-2337).
 * Built on demand by tests/gbuffer_helpers.py with oracle/Makefile's flags (-ffp-contract=off matters) into _build/.
 */
#include "../../oracle/rm_oracle.c"

/* normalDepth: W·H·4 floats (n.x, n.y, n.z, depth); objectId: W·H int32; position: W·H·4 floats (p.x, p.y, p.z, hit ? 1 : 0) or
 * NULL.  Row 0 at the bottom.  Reads cam, the object table, g and s (maxSteps, the fractal bounds, RM_FEAT_PERLIN_BUMP); no
 * lights, no resources.  The caller passes a frame the entry point accepts (no layers, no 2-D mode, no CUSTOM object). */
int rmo_spec_gbuffer(const RmCamera *cam, const RmObject *objs, int numObjects, const RmGlobals *g, const RmSettings *s, int W,
                     int H, float *normalDepth, int32_t *objectId, float *position) {
  if (!cam || !g || !s || (numObjects > 0 && !objs) || numObjects < 0 || numObjects > RM_MAX_OBJECTS || W <= 0 || H <= 0 ||
      !normalDepth || !objectId)
    return RM_ERR_INVALID_ARGUMENT;
  RmResources none;
  memset(&none, 0, sizeof none);
  Ctx c;
  memset(&c, 0, sizeof c);
  c.cam = cam; c.objs = objs; c.numObjects = numObjects; c.lights = NULL; c.numLights = 0;
  c.g = *g; c.s = *s; c.tex = NULL; c.numTex = 0; c.res = &none; c.W = W;
  rayPlanes(cam->invProjView, c.rayPlane);
  const float far = cam->initialFar;
  for (int py = 0; py < H; py++)
    for (int px = 0; px < W; px++) {
      /* shadePixel: the pixel centre in the full-screen quad, the varyings, frag:2388-2392 */
      const float tx = ((float)px + 0.5f) / (float)W, ty = ((float)py + 0.5f) / (float)H;
      const int upper = (tx + ty) > 1.0f;
      const float I = upper ? 1.0f - tx : tx, J = upper ? 1.0f - ty : ty;
      v4 nearClip = interpolateVarying(c.rayPlane[upper][0], I, J);
      v4 farClip = interpolateVarying(c.rayPlane[upper][1], I, J);
      v3 ro = V3(nearClip.x / nearClip.w, nearClip.y / nearClip.w, nearClip.z / nearClip.w);
      v3 farC = V3(farClip.x / farClip.w, farClip.y / farClip.w, farClip.z / farClip.w);
      v3 rd = normalize3(v3_sub(farC, ro));
      /* render: frag:2318-2337 */
      RayMarchRes res = raymarch(&c, ro, rd, far, OUTSIDE);
      const size_t o = (size_t)py * (size_t)W + (size_t)px;
      v3 n = V3(0.0f, 0.0f, 0.0f), p = V3(0.0f, 0.0f, 0.0f);
      float depth = far; /* RenderInfo.d of a miss (frag:2328) */
      if (res.intersectObj != -1) {
        depth = res.d;
        p = v3_madd(rd, res.d, ro);
        n = getNormal(&c, p);
        if (c.s.features & RM_FEAT_PERLIN_BUMP) n = bumpNormal(n, p, 10.0f, 2.0f);
      }
      normalDepth[4 * o + 0] = n.x; normalDepth[4 * o + 1] = n.y; normalDepth[4 * o + 2] = n.z; normalDepth[4 * o + 3] = depth;
      objectId[o] = res.intersectObj;
      if (position) {
        position[4 * o + 0] = p.x; position[4 * o + 1] = p.y; position[4 * o + 2] = p.z;
        position[4 * o + 3] = (res.intersectObj != -1) ? 1.0f : 0.0f;
      }
    }
  return RM_OK;
}
