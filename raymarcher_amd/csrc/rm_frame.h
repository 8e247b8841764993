// rm_frame.h — the host-only scene prep (rm_frame.cpp): argument checks of a scene, the derived fields of its SceneBlocks and
// the class of kernels a frame takes.  No HIP.
#pragma once
#include <climits>
#include <cstddef>

#include "rm_scene_block.h"

namespace rm {

// A knob for A/B runs: see rm_frame.cpp.
int env_int(const char *name, int def, int lo = INT_MIN, int hi = INT_MAX);

// RM_OK, or the status of the first check the scene fails with its text in rm_last_error.
int validate_scene(const RmCamera *cam, const RmObject *objs, int numObjects, const RmLight *lights, int numLights,
                   const RmGlobals *g, const RmSettings *s, const RmResources &res);
// The same for a bare object table whose pointers and count are checked (rm_render_gbuffer, rm_trace_rays): the capacity, the
// loop bounds of the march and the types.
int check_object_table(const RmObject *objs, int numObjects, const RmSettings *s);
double sigma_max3(const double m[3][3]);
void scene_cull_ball(SceneBlock *h);
void ray_planes(SceneBlock *h);
void scene_eval_records(SceneBlock *h);
void scene_light_prep(SceneBlock *h);
int bulb_plain(const RmObject *objs, int numObjects, const RmGlobals *g);
void fill_frames(SceneBlock *h, int n, const RmCamera *cams, const RmGlobals *globals, int numGlobals, const RmObject *objs,
                 int numObjects, const RmLight *lights, int numLights, const RmSettings *s, const RmResources &res);
void fill_frames_animated(SceneBlock *h, int n, const RmCamera *cams, const RmGlobals *globals, int numGlobals, const RmObject *objs,
                          int numObjects, int numObjectTables, const RmLight *lights, int numLights, int numLightTables,
                          const RmSettings *s, const RmResources &res, RestageBits *restage);

bool skip_applies(const RmObject *objs, int numObjects);
bool all_primitives(const RmObject *objs, int numObjects);
bool wavefront_pays(const RmObject *objs, int numObjects, int bounces, size_t pixels, bool tileShard);

// What decides which kernels a frame takes.
struct FrameClass {
  bool bulb, twoD, envFeatures, textured, secondary;
  bool wfOk, wfSkip;  // the wavefront pipeline covers this frame; its kernels take the table walk's pass-over test
  int wfBounces;      // its reflection generations
};
FrameClass classify_frame(const RmObject *objs, int numObjects, const RmLight *lights, int numLights, const RmGlobals *g,
                          const RmSettings *s, int count);
int bulb_class(const FrameClass &fc, bool plainBulb);
int table_bulb_class(const RmObject *objs, int numObjects, bool plainBulb);

unsigned long long picture_key(const RmCamera *cam, const RmObject *objs, int numObjects, const RmLight *lights, int numLights,
                               const RmGlobals *g, const RmSettings *s, const RowMap &map);
int row_range(int H, int rowBegin, int rowEnd, RowMap *map, int *nRows);

}  // namespace rm
