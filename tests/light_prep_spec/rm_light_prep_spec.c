/*
 * tests/light_prep_spec/rm_light_prep_spec.c — TEST INFRASTRUCTURE.  The specification of the per-light constants the launcher
 * stages for the bulb kernels' shadow pool (rm_debug_light_prep, include/raymarcher_amd.h), restated with the oracle's OWN static
 * functions: L is the oracle's normalize3 of the negated direction, as its getPhong takes it for a directional light; pd and a are
 * the products of the cull (rm_device.hip.h, bulbCullEnd) written with the oracle's rm_fma and dot3.  Nothing under oracle/ changes
 * for this: the file includes the oracle's source, as tests/trace_spec/rm_trace_spec.c does.
 * Built on demand by tests/helpers.py (load_spec) with oracle/Makefile's flags (-ffp-contract=off matters) into _build/.
 */
#include "../../oracle/rm_oracle.c"

/* out: 8 floats per light { L xyz, pd xyz, a, 0 }; zeros for a light that is not directional. */
int rmo_spec_light_prep(const RmObject *objs, int numObjects, const RmLight *lights, int numLights, float *out) {
  if ((numObjects > 0 && !objs) || (numLights > 0 && !lights) || !out || numObjects < 0 || numLights < 0) return RM_ERR_INVALID_ARGUMENT;
  for (int i = 0; i < numLights; i++) {
    float *o = out + 8 * (size_t)i;
    for (int k = 0; k < 8; k++) o[k] = 0.0f;
    if (lights[i].type != RM_LIGHT_DIRECTIONAL) continue;
    const v3 L = normalize3(V3(-lights[i].dir[0], -lights[i].dir[1], -lights[i].dir[2]));
    o[0] = L.x; o[1] = L.y; o[2] = L.z;
    if (numObjects < 1) continue;
    const float *M = objs[0].invModel;
    const v3 pd = V3(rm_fma(M[8], L.z, rm_fma(M[4], L.y, M[0] * L.x)), rm_fma(M[9], L.z, rm_fma(M[5], L.y, M[1] * L.x)),
                     rm_fma(M[10], L.z, rm_fma(M[6], L.y, M[2] * L.x)));
    o[3] = pd.x; o[4] = pd.y; o[5] = pd.z;
    o[6] = dot3(pd, pd);
  }
  return RM_OK;
}
