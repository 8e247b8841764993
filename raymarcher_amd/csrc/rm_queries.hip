// rm_queries.hip — the query entry points of the C ABI (gfx950 only): rays, points and lattices against ONE scene, and the test-only
// probes.  Each checks its arguments, stages one scene block and launches one kernel of another unit through the launcher's
// stage_block_launch (rm_launch.h), which also records the path and the timing: nothing here reads or writes a tuner, the tile
// order or the wavefront state, and nothing here sees the launcher's slots, rings or device state.  Host code only: the kernels
// and the functions that launch them are in rm_trace.hip, rm_shade.hip, rm_shade_indirect.hip, rm_light_probes.hip, rm_light_probes_indirect.hip, rm_light_depth.hip, rm_layers.hip, rm_points.hip,
// rm_volume.hip, rm_blocks.hip and rm_probe.hip (declared in rm_internal.h, the lattice family's in rm_lattice.h), the scene prep that needs no GPU in rm_frame.cpp.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>
#include <vector>

#include "rm_internal.h"
#include "rm_frame.h"
#include "rm_lattice.h"
#include "rm_launch.h"

namespace rm {
namespace {

// ---- rays from memory: closest hits and occlusion (rm_trace_rays) -----------------------------------------------------------------
// rm_trace_rays (the header has the definition): the caller's rays against ONE object table.  Its checks run in check_gbuffer's
// order, every one but the last ahead of the first HIP call: numRays (negative; zero is RM_OK; every int fits one grid of
// 256-lane workgroups), the scene pointers, the mode bits, the layers and the 2-D mode a ray is not defined through, the
// table's limits and types, the arrays (null, alignment of the float4 accesses), then whether they are device memory.
// Staging is stage_block_launch: one block, filled with a zeroed camera, no lights and no resources — the evaluation records, the
// cull ball and box with cullLip and cullOneOk, bulbPlain.  rayPlane and cam are staged (zeros) and never read.  The occlusion mode
// stages two fields of its own: s.enableSoftShadow = 1, so that march<…, kShadow> tracks the penumbra factor whatever the caller's
// settings say, and cullR2Soft = 0 (occlusion_fields, the call's afterFill).  scene_cull_ball derives that larger ball for shadow
// rays that start on a surface, inside the cull ball, where t <= ρ + R; a caller's ray may start anywhere, so with it a far origin
// would settle the factor too early.  Without it a soft march ends at tMax, as the reference's does.  (The hard bounds — ball, box,
// the bulb's own ball — argue about points, not origins, and hold for any ray.)
// Then ONE launch of trace_kernel (rm_trace.hip), path 12: no tuner, tile-order or workspace state is read or changed.
// rm_trace_rays_layers is the same call with TraceCall.layers set: imageWidth is checked behind the mode bits, the refusal of the
// layers holds only for the occlusion mode, the launch is trace_layers_kernel (rm_layers.hip) when TERRAIN or SEA is set, path 15.
struct TraceCall {
  const RmRay *d_rays; int numRays;
  const RmObject *objs; int numObjects; const RmGlobals *g; const RmSettings *s;
  unsigned mode; RmRayHit *d_hits; hipStream_t stream;
  bool layers = false; int imageWidth = 1;  // rm_trace_rays_layers: the layers are traced, not refused
};
int check_trace(const TraceCall &c) {
  if (c.numRays < 0) { set_error("negative numRays"); return RM_ERR_INVALID_ARGUMENT; }
  if (c.numRays == 0) return RM_OK;
  static_assert(((long long)INT_MAX + 255) / 256 <= INT_MAX, "every int numRays fits one grid of 256-lane workgroups");
  if (!c.g || !c.s || (c.numObjects > 0 && !c.objs) || c.numObjects < 0) {
    set_error("null scene pointer or negative count");
    return RM_ERR_INVALID_ARGUMENT;
  }
  if (c.mode & ~(RM_TRACE_NO_NORMAL | RM_TRACE_OCCLUSION)) { set_error("unknown mode bits"); return RM_ERR_INVALID_ARGUMENT; }
  if ((c.mode & RM_TRACE_NO_NORMAL) && (c.mode & RM_TRACE_OCCLUSION)) {
    set_error("RM_TRACE_NO_NORMAL is a flag on RM_TRACE_CLOSEST: occlusion stores no normal anyway");
    return RM_ERR_INVALID_ARGUMENT;
  }
  int st = RM_OK;
  if (!c.layers) st = refuse_layers(c.s, "rm_trace_rays traces the object table: rays through TERRAIN / CLOUD / SEA are not defined");
  else if ((st = check_image_width(c.imageWidth)) == RM_OK && (c.mode & RM_TRACE_OCCLUSION))
    st = refuse_layers(c.s, "RM_TRACE_OCCLUSION is the objects' shadow march: it does not see TERRAIN / CLOUD / SEA");
  if (st != RM_OK || (st = refuse_two_d(c.g, "the 2-D mode (isTwoD) marches no ray")) != RM_OK) return st;
  if ((st = check_object_table(c.objs, c.numObjects, c.s)) != RM_OK) return st;
  if (!c.d_rays || !c.d_hits) { set_error("null d_rays or d_hits"); return RM_ERR_INVALID_ARGUMENT; }
  if (((uintptr_t)c.d_rays | (uintptr_t)c.d_hits) & 15u) { set_error("d_rays and d_hits must be 16-byte aligned"); return RM_ERR_INVALID_ARGUMENT; }
  return require_device_pointers({{"d_rays", c.d_rays}, {"d_hits", c.d_hits}});
}
void occlusion_fields(SceneBlock *h) { h->cullR2Soft = 0.0f; }
int launch_trace(const TraceCall &c) {
  int st = check_trace(c);
  if (st != RM_OK || c.numRays == 0) return st;
  const bool occlusion = (c.mode & RM_TRACE_OCCLUSION) != 0;
  const int bulbClass = table_bulb_class(c.objs, c.numObjects, bulb_plain(c.objs, c.numObjects, c.g) != 0);
  RmSettings s = *c.s;
  if (occlusion) s.enableSoftShadow = 1;
  BlockCall b{c.objs, c.numObjects, c.g, &s, c.stream, c.layers ? 15 : 12};
  if (occlusion) b.afterFill = occlusion_fields;
  // the layers' kernel only where a layer has a surface: without one (CLOUD alone is a volume) rm_trace_rays' own kernels run
  const bool noNormal = (c.mode & RM_TRACE_NO_NORMAL) != 0;
  return stage_block_launch(b, [&](const SceneBlock *sb, const SceneBlock *, void *) {
    if (c.layers && (c.s->features & (RM_FEAT_TERRAIN | RM_FEAT_SEA)))
      return launch_trace_layers_kernel(sb, bulbClass, noNormal, c.d_rays, c.numRays, c.imageWidth, c.d_hits, c.stream);
    return launch_trace_kernel(sb, bulbClass, occlusion, noNormal, c.d_rays, c.numRays, c.d_hits, c.stream);
  });
}

// ---- rays from memory: the full colour (rm_shade_rays) ----------------------------------------------------------------------------
// rm_shade_rays (the header has the definition): the shader's whole main for the caller's rays against ONE scene.  ShadeCall stands
// beside TraceCall; its checks run in check_trace's order, every one but the last ahead of the first HIP call: numRays (negative;
// zero is RM_OK), the scene pointers and counts, far, the layers and the 2-D mode a ray is not defined through, then what
// validate_scene checks of a frame — the limits, the loop bounds, the samplers a feature, an object or a light reads, the types,
// with rm_render_res's statuses and texts — the arrays (null, alignment of the float4 accesses), and whether they, and the
// resources' pixels, are device memory.
// Staging is stage_block_launch: one block, filled with the caller's lights and resources and a camera that is zeros but for
// initialFar = far — the one far every device function reads, wave-uniform (a per-ray far would change which lane of the shadow
// pool ends a pooled ray where).  rayPlane and the rest of cam are staged and never read.  The class is the frame's
// (classify_frame, bulb_class with the plain form where bulb_plain finds it).  Then ONE launch of shade_rays_kernel
// (rm_shade.hip), path 13: no wavefront pipeline, no light split, no tuner, tile-order or workspace state is read or changed.
// rm_shade_rays_layers is the same call with ShadeCall.layers set: imageWidth is checked in place of the refusal of the layers, the
// launch is shade_rays_layers_kernel (rm_layers.hip) when a layer bit is set, path 14.
struct ShadeCall {
  const RmRay *d_rays; int numRays; float far;
  const RmObject *objs; int numObjects; const RmLight *lights; int numLights;
  const RmGlobals *g; const RmSettings *s; const RmResources &res;
  float *d_rgba, *d_bright; hipStream_t stream;
  bool layers = false; int imageWidth = 1;  // rm_shade_rays_layers: the layers are shaded, not refused
};
int check_shade_args(const ShadeCall &c, const RmCamera &cam) {  // every check ahead of the first HIP call
  if (c.numRays < 0) { set_error("negative numRays"); return RM_ERR_INVALID_ARGUMENT; }
  if (c.numRays == 0) return RM_OK;
  if (!c.g || !c.s || (c.numObjects > 0 && !c.objs) || (c.numLights > 0 && !c.lights) || c.numObjects < 0 || c.numLights < 0) {
    set_error("null scene pointer or negative count");
    return RM_ERR_INVALID_ARGUMENT;
  }
  if (!(c.far >= 0.0f) || c.far == __builtin_inff()) { set_error("far must be finite and not negative"); return RM_ERR_INVALID_ARGUMENT; }
  int st = RM_OK;
  if (c.layers) st = check_image_width(c.imageWidth);
  else st = refuse_layers(c.s, "rm_shade_rays shades rays against the object table: rays through TERRAIN / CLOUD / SEA are not defined");
  if (st != RM_OK || (st = refuse_two_d(c.g, "the 2-D mode (isTwoD) marches no ray")) != RM_OK) return st;
  if ((st = validate_scene(&cam, c.objs, c.numObjects, c.lights, c.numLights, c.g, c.s, c.res)) != RM_OK) return st;
  if (!c.d_rays || !c.d_rgba) { set_error("null d_rays or d_rgba"); return RM_ERR_INVALID_ARGUMENT; }
  if (((uintptr_t)c.d_rays | (uintptr_t)c.d_rgba | (uintptr_t)c.d_bright) & 15u) {
    set_error("d_rays, d_rgba and d_bright must be 16-byte aligned");
    return RM_ERR_INVALID_ARGUMENT;
  }
  return RM_OK;
}
int check_shade_device(const ShadeCall &c) {
  if (int st = require_device_pointers({{"d_rays", c.d_rays}})) return st;
  return check_device_pointers(c.res, c.d_rgba, c.d_bright);
}
int check_shade(const ShadeCall &c, const RmCamera &cam) {
  const int st = check_shade_args(c, cam);
  return (st != RM_OK || c.numRays == 0) ? st : check_shade_device(c);
}
int launch_shade(const ShadeCall &c) {
  RmCamera cam{};
  cam.initialFar = c.far;
  int st = check_shade(c, cam);
  if (st != RM_OK || c.numRays == 0) return st;
  const FrameClass fc = classify_frame(c.objs, c.numObjects, c.lights, c.numLights, c.g, c.s, 0);
  const int bulbClass = bulb_class(fc, bulb_plain(c.objs, c.numObjects, c.g) != 0);
  BlockCall b{c.objs, c.numObjects, c.g, c.s, c.stream, c.layers ? 14 : 13};
  b.cam = &cam; b.lights = c.lights; b.numLights = c.numLights; b.res = &c.res;
  // the layers' kernel only with a layer bit (then fc.envFeatures is set and bulbClass is 0): without one, rm_shade_rays' twelve classes
  return stage_block_launch(b, [&](const SceneBlock *sb, const SceneBlock *, void *) {
    if (c.layers && (c.s->features & (RM_FEAT_TERRAIN | RM_FEAT_CLOUD | RM_FEAT_SEA)))
      return launch_shade_layers_kernel(sb, fc.textured, fc.secondary, c.d_rays, c.numRays, c.imageWidth, c.d_rgba, c.d_bright, c.stream);
    return launch_shade_kernel(sb, bulbClass, fc.envFeatures, fc.textured, fc.secondary, c.d_rays, c.numRays, c.d_rgba, c.d_bright, c.stream);
  });
}

// ---- light probes: rays from a position and a table row, shaded and summed (rm_light_probes) -------------------------------------
// rm_light_probes (the header has the definition): rm_shade_rays for the rays of numProbes positions times the numDirs rows of a
// direction table, each colour and hit flag multiplied into its row's nine basis values and summed per probe inside the kernel.
// ProbesCall stands beside ShadeCall; its checks run in check_shade's order with its words where they overlap, every one but the
// last ahead of the first HIP call: numProbes (negative), the table's shape (numDirs, then numSets), numProbes == 0 (RM_OK), the
// rays of the call beyond INT_MAX, the scene pointers and counts, far, the layers and the 2-D mode, validate_scene, the arrays
// (null, alignment of the float4 accesses), and whether they, and the resources' pixels, are device memory.
// Staging is launch_shade's: stage_block_launch, one block, the caller's lights and resources and a camera that is zeros but for
// initialFar = far; the class is the frame's.  Then ONE launch of light_probes_kernel (rm_light_probes.hip), path 21: no tuner,
// tile-order or workspace state is read or changed and nothing is allocated.
struct ProbesCall {
  const float *d_positions; int numProbes; const RmProbeDir *d_dirs; int numDirs, numSets; float far;
  const RmObject *objs; int numObjects; const RmLight *lights; int numLights;
  const RmGlobals *g; const RmSettings *s; const RmResources &res;
  RmLightProbe *d_out; hipStream_t stream;
};
// What rm_light_probes and rm_sphere_directions refuse about the table's shape; no HIP call.
int check_probe_table(int numDirs, int numSets) {
  if (numDirs < 1 || numDirs > RM_MAX_PROBE_DIRS || (numDirs & (numDirs - 1)) != 0) {
    set_error("numDirs must be a power of two, 1 … RM_MAX_PROBE_DIRS (1024)");
    return RM_ERR_INVALID_ARGUMENT;
  }
  if (numSets < 1 || (long long)numSets * numDirs > RM_MAX_PROBE_TABLE) {
    set_error("numSets must be at least 1 and numSets * numDirs at most RM_MAX_PROBE_TABLE (4096)");
    return RM_ERR_INVALID_ARGUMENT;
  }
  return RM_OK;
}
int check_probes_args(const ProbesCall &c, const RmCamera &cam) {  // every check ahead of the first HIP call
  if (c.numProbes < 0) { set_error("negative numProbes"); return RM_ERR_INVALID_ARGUMENT; }
  int st = check_probe_table(c.numDirs, c.numSets);
  if (st != RM_OK || c.numProbes == 0) return st;
  if ((long long)c.numProbes * c.numDirs > INT_MAX) { set_error("numProbes * numDirs exceeds INT_MAX rays"); return RM_ERR_INVALID_ARGUMENT; }
  if (!c.g || !c.s || (c.numObjects > 0 && !c.objs) || (c.numLights > 0 && !c.lights) || c.numObjects < 0 || c.numLights < 0) {
    set_error("null scene pointer or negative count");
    return RM_ERR_INVALID_ARGUMENT;
  }
  if (!(c.far >= 0.0f) || c.far == __builtin_inff()) { set_error("far must be finite and not negative"); return RM_ERR_INVALID_ARGUMENT; }
  st = refuse_layers(c.s, "rm_light_probes shades rays against the object table: rays through TERRAIN / CLOUD / SEA are not defined");
  if (st != RM_OK || (st = refuse_two_d(c.g, "the 2-D mode (isTwoD) marches no ray")) != RM_OK) return st;
  if ((st = validate_scene(&cam, c.objs, c.numObjects, c.lights, c.numLights, c.g, c.s, c.res)) != RM_OK) return st;
  if (!c.d_positions || !c.d_dirs || !c.d_out) { set_error("null d_positions, d_dirs or d_out"); return RM_ERR_INVALID_ARGUMENT; }
  if (((uintptr_t)c.d_positions | (uintptr_t)c.d_dirs | (uintptr_t)c.d_out) & 15u) {
    set_error("d_positions, d_dirs and d_out must be 16-byte aligned");
    return RM_ERR_INVALID_ARGUMENT;
  }
  return RM_OK;
}
int check_probes_device(const ProbesCall &c) {
  if (int st = require_device_pointers({{"d_positions", c.d_positions}, {"d_dirs", c.d_dirs}, {"d_out", c.d_out}})) return st;
  return check_device_pointers(c.res, nullptr, nullptr);
}
int check_probes(const ProbesCall &c, const RmCamera &cam) {
  const int st = check_probes_args(c, cam);
  return (st != RM_OK || c.numProbes == 0) ? st : check_probes_device(c);
}
int launch_probes(const ProbesCall &c) {
  RmCamera cam{};
  cam.initialFar = c.far;
  int st = check_probes(c, cam);
  if (st != RM_OK || c.numProbes == 0) return st;
  const FrameClass fc = classify_frame(c.objs, c.numObjects, c.lights, c.numLights, c.g, c.s, 0);
  const int bulbClass = bulb_class(fc, bulb_plain(c.objs, c.numObjects, c.g) != 0);
  BlockCall b{c.objs, c.numObjects, c.g, c.s, c.stream, 21};
  b.cam = &cam; b.lights = c.lights; b.numLights = c.numLights; b.res = &c.res;
  return stage_block_launch(b, [&](const SceneBlock *sb, const SceneBlock *, void *) {
    return launch_probes_kernel(sb, bulbClass, fc.envFeatures, fc.textured, fc.secondary, c.d_positions, c.numProbes, c.d_dirs, c.numDirs,
                                c.numSets, c.d_out, c.stream);
  });
}

// ---- the grid's diffuse term at the hit of a shaded ray (rm_shade_rays_indirect, rm_light_probes_indirect) -------------------------
// Both (the header has the definition) are launch_shade / launch_probes with a light grid in the kernel's arguments and no bright
// output.  The checks: check_shade_args / check_probes_args (the call's own, all ahead of the first HIP call; a call of no ray or
// no probe is RM_OK there), then check_grid_ref — rm_light_grid_irradiance_visible's order with d_depth == NULL allowed, then the
// strength —, for the bake the overlap of d_out with the grid's probe records, and last the device-memory checks of the call and
// of the grid.  Staging and class are launch_shade's; ONE launch of shade_rays_indirect_kernel (rm_shade_indirect.hip), path 23, or
// of light_probes_indirect_kernel (rm_light_probes_indirect.hip), path 24.
int check_grid_ref(const RmLightGridRef *gr) {
  using fchk::bad;
  if (!gr) return bad("null grid");
  for (int a = 0; a < 3; a++)
    if (gr->dims[a] < 2 || gr->dims[a] > RM_MAX_LIGHT_GRID_DIM) return bad("grid dimension must be 2 … RM_MAX_LIGHT_GRID_DIM (1024)");
  if ((long long)gr->dims[0] * gr->dims[1] * gr->dims[2] > RM_MAX_LIGHT_GRID_PROBES) return bad("more than RM_MAX_LIGHT_GRID_PROBES (2^24) probes");
  for (int a = 0; a < 3; a++)
    if (!std::isfinite(gr->origin[a])) return bad("origin must be finite");
  for (int a = 0; a < 3; a++)
    if (!std::isfinite(gr->step[a]) || !(gr->step[a] > 0.0f)) return bad("step must be finite and greater than 0");
  if (!std::isfinite(gr->normalBias)) return bad("normalBias must be finite");
  if (gr->flags & ~RM_LIGHT_GRID_FACING) return bad("flag bits other than RM_LIGHT_GRID_FACING");
  if (!gr->d_probes) return bad("null d_probes in the grid");
  if (((uintptr_t)gr->d_probes | (uintptr_t)gr->d_depth) & 15u) return bad("the grid's d_probes and d_depth must be 16-byte aligned");
  if (!std::isfinite(gr->strength)) return bad("strength must be finite");
  return RM_OK;
}
int check_grid_device(const RmLightGridRef &gr) { return require_device_pointers({{"grid.d_probes", gr.d_probes}, {"grid.d_depth", gr.d_depth}}); }
// The checked grid as the kernels take it; k = strength · RM_INV_PI, the ONE multiplication of the definition.
IndirectGridArgs grid_args(const RmLightGridRef &gr) {
  IndirectGridArgs a{gr.d_probes, gr.d_depth, {gr.dims[0], gr.dims[1], gr.dims[2]}, {gr.origin[0], gr.origin[1], gr.origin[2]},
                     {gr.step[0], gr.step[1], gr.step[2]}, 0.0f, gr.flags, gr.normalBias};
  volatile float k = gr.strength * RM_INV_PI;  // volatile: rounded to binary32 here, whatever the host's evaluation method
  a.k = k;
  return a;
}
int launch_shade_indirect(const ShadeCall &c, const RmLightGridRef *gridRef) {
  RmCamera cam{};
  cam.initialFar = c.far;
  int st = check_shade_args(c, cam);
  if (st != RM_OK || c.numRays == 0) return st;
  if ((st = check_grid_ref(gridRef)) != RM_OK) return st;
  const RmLightGridRef gr = *gridRef;  // the caller's struct is read once
  if ((st = check_shade_device(c)) != RM_OK || (st = check_grid_device(gr)) != RM_OK) return st;
  const IndirectGridArgs ga = grid_args(gr);
  const FrameClass fc = classify_frame(c.objs, c.numObjects, c.lights, c.numLights, c.g, c.s, 0);
  const int bulbClass = bulb_class(fc, bulb_plain(c.objs, c.numObjects, c.g) != 0);
  BlockCall b{c.objs, c.numObjects, c.g, c.s, c.stream, 23};
  b.cam = &cam; b.lights = c.lights; b.numLights = c.numLights; b.res = &c.res;
  return stage_block_launch(b, [&](const SceneBlock *sb, const SceneBlock *, void *) {
    return launch_shade_indirect_kernel(sb, bulbClass, fc.envFeatures, fc.textured, fc.secondary, c.d_rays, c.numRays, ga, c.d_rgba, c.stream);
  });
}
int launch_probes_indirect(const ProbesCall &c, const RmLightGridRef *gridRef) {
  RmCamera cam{};
  cam.initialFar = c.far;
  int st = check_probes_args(c, cam);
  if (st != RM_OK || c.numProbes == 0) return st;
  if ((st = check_grid_ref(gridRef)) != RM_OK) return st;
  const RmLightGridRef gr = *gridRef;
  const uintptr_t o0 = (uintptr_t)c.d_out, o1 = o0 + (uintptr_t)c.numProbes * sizeof(RmLightProbe);
  const uintptr_t g0 = (uintptr_t)gr.d_probes, g1 = g0 + (uintptr_t)gr.dims[0] * gr.dims[1] * gr.dims[2] * sizeof(RmLightProbe);
  if (o0 < g1 && g0 < o1) {
    set_error("d_out overlaps the grid's probe records: a bake must not read the grid it writes");
    return RM_ERR_INVALID_ARGUMENT;
  }
  if ((st = check_probes_device(c)) != RM_OK || (st = check_grid_device(gr)) != RM_OK) return st;
  const IndirectGridArgs ga = grid_args(gr);
  const FrameClass fc = classify_frame(c.objs, c.numObjects, c.lights, c.numLights, c.g, c.s, 0);
  const int bulbClass = bulb_class(fc, bulb_plain(c.objs, c.numObjects, c.g) != 0);
  BlockCall b{c.objs, c.numObjects, c.g, c.s, c.stream, 24};
  b.cam = &cam; b.lights = c.lights; b.numLights = c.numLights; b.res = &c.res;
  return stage_block_launch(b, [&](const SceneBlock *sb, const SceneBlock *, void *) {
    return launch_probes_indirect_kernel(sb, bulbClass, fc.envFeatures, fc.textured, fc.secondary, c.d_positions, c.numProbes, c.d_dirs,
                                         c.numDirs, c.numSets, ga, c.d_out, c.stream);
  });
}

// ---- probe depth: rays from a position and a table row, marched and summed into 64 texels (rm_light_probes_depth) ------------------
// rm_light_probes_depth (the header has the definition): rm_trace_rays' closest hit for the rays of numProbes positions times the
// numDirs rows of rm_light_probes' direction table, each distance and its square multiplied into the row's 64 texel weights and
// summed per probe and texel inside the kernel.  Its checks run in check_probes' order with maxDistance in the place of far and
// d_weights beside d_dirs; a march reads no material, so the scene is checked and staged as launch_trace's (check_object_table, a
// zeroed camera, no lights, no resources, the table's march class).  Then ONE launch of light_depth_kernel (rm_light_depth.hip),
// path 22: no tuner, tile-order or workspace state is read or changed and nothing is allocated.
struct ProbesDepthCall {
  const float *d_positions; int numProbes; const RmProbeDir *d_dirs; const float *d_weights; int numDirs, numSets; float maxDistance;
  const RmObject *objs; int numObjects; const RmGlobals *g; const RmSettings *s;
  RmProbeDepth *d_out; hipStream_t stream;
};
int check_probes_depth(const ProbesDepthCall &c) {
  if (c.numProbes < 0) { set_error("negative numProbes"); return RM_ERR_INVALID_ARGUMENT; }
  int st = check_probe_table(c.numDirs, c.numSets);
  if (st != RM_OK || c.numProbes == 0) return st;
  if ((long long)c.numProbes * c.numDirs > INT_MAX) { set_error("numProbes * numDirs exceeds INT_MAX rays"); return RM_ERR_INVALID_ARGUMENT; }
  if (!c.g || !c.s || (c.numObjects > 0 && !c.objs) || c.numObjects < 0) {
    set_error("null scene pointer or negative count");
    return RM_ERR_INVALID_ARGUMENT;
  }
  if (!(c.maxDistance > 0.0f) || c.maxDistance == __builtin_inff()) {
    set_error("maxDistance must be finite and greater than 0");
    return RM_ERR_INVALID_ARGUMENT;
  }
  st = refuse_layers(c.s, "rm_light_probes_depth marches rays against the object table: rays through TERRAIN / CLOUD / SEA are not defined");
  if (st != RM_OK || (st = refuse_two_d(c.g, "the 2-D mode (isTwoD) marches no ray")) != RM_OK) return st;
  if ((st = check_object_table(c.objs, c.numObjects, c.s)) != RM_OK) return st;
  if (!c.d_positions || !c.d_dirs || !c.d_weights || !c.d_out) {
    set_error("null d_positions, d_dirs, d_weights or d_out");
    return RM_ERR_INVALID_ARGUMENT;
  }
  if (((uintptr_t)c.d_positions | (uintptr_t)c.d_dirs | (uintptr_t)c.d_weights | (uintptr_t)c.d_out) & 15u) {
    set_error("d_positions, d_dirs, d_weights and d_out must be 16-byte aligned");
    return RM_ERR_INVALID_ARGUMENT;
  }
  return require_device_pointers({{"d_positions", c.d_positions}, {"d_dirs", c.d_dirs}, {"d_weights", c.d_weights}, {"d_out", c.d_out}});
}
int launch_probes_depth(const ProbesDepthCall &c) {
  int st = check_probes_depth(c);
  if (st != RM_OK || c.numProbes == 0) return st;
  const int bulbClass = table_bulb_class(c.objs, c.numObjects, bulb_plain(c.objs, c.numObjects, c.g) != 0);
  BlockCall b{c.objs, c.numObjects, c.g, c.s, c.stream, 22};
  return stage_block_launch(b, [&](const SceneBlock *sb, const SceneBlock *, void *) {
    return launch_probes_depth_kernel(sb, bulbClass, c.d_positions, c.numProbes, c.d_dirs, c.d_weights, c.numDirs, c.numSets, c.maxDistance,
                                      c.d_out, c.stream);
  });
}

// ---- points from memory (rm_shade_points) -----------------------------------------------------------------------------------------
// rm_shade_points (the header has the definition): the scene's distance, object, normal, ambient occlusion and shaded colour at the
// caller's points against ONE scene.  PointsCall stands beside ShadeCall and its checks run in check_shade's order with its helpers,
// every one but the last ahead of the first HIP call: numPoints, the pointers and counts, the point settings, the outputs (at least
// one), the layers and the 2-D mode, the scene, the arrays, device memory.  Only a call with d_rgba reads lights and samplers: it is
// checked and staged as launch_shade's (validate_scene, the caller's lights and resources, the frame's class); a call without it as
// launch_trace's (check_object_table, no lights, no resources, the table's march class).  The camera is zeros but for initialFar =
// ps->far.  Then ONE launch of shade_points_kernel (rm_points.hip), path 17: no tuner, tile-order or workspace state is read or changed.
struct PointsCall {
  const float *d_points, *d_view; int numPoints; const RmPointsSettings *ps;
  const RmObject *objs; int numObjects; const RmLight *lights; int numLights;
  const RmGlobals *g; const RmSettings *s; const RmResources &res;
  RmSurfacePoint *d_surface; float *d_ao, *d_rgba; hipStream_t stream;
};
int check_points(const PointsCall &c, const RmCamera &cam) {
  if (c.numPoints < 0) { set_error("negative numPoints"); return RM_ERR_INVALID_ARGUMENT; }
  if (c.numPoints == 0) return RM_OK;
  if (!c.ps || !c.g || !c.s || (c.numObjects > 0 && !c.objs) || (c.d_rgba && c.numLights > 0 && !c.lights) || c.numObjects < 0 ||
      c.numLights < 0) {
    set_error("null ps, scene pointer or negative count");
    return RM_ERR_INVALID_ARGUMENT;
  }
  const RmPointsSettings &ps = *c.ps;
  if (!(ps.far >= 0.0f) || ps.far == __builtin_inff()) { set_error("far must be finite and not negative"); return RM_ERR_INVALID_ARGUMENT; }
  if (!(ps.iso - ps.iso == 0.0f)) { set_error("iso must be finite"); return RM_ERR_INVALID_ARGUMENT; }
  if (!(ps.maxMove >= 0.0f)) { set_error("maxMove must not be negative (+inf: no limit)"); return RM_ERR_INVALID_ARGUMENT; }
  if (ps.projectSteps < 0 || ps.projectSteps > RM_MAX_PROJECT_STEPS) {
    set_error("projectSteps outside 0 … RM_MAX_PROJECT_STEPS");
    return RM_ERR_INVALID_ARGUMENT;
  }
  if (!c.d_surface && !c.d_ao && !c.d_rgba) { set_error("d_surface, d_ao and d_rgba are all null: nothing to compute"); return RM_ERR_INVALID_ARGUMENT; }
  int st = refuse_layers(c.s, "rm_shade_points shades points of the object table: TERRAIN / CLOUD / SEA have no distance field here");
  if (st != RM_OK || (st = refuse_two_d(c.g, "the 2-D mode (isTwoD) has no surface points")) != RM_OK) return st;
  if (c.d_rgba) st = validate_scene(&cam, c.objs, c.numObjects, c.lights, c.numLights, c.g, c.s, c.res);
  else st = check_object_table(c.objs, c.numObjects, c.s);
  if (st != RM_OK) return st;
  if (!c.d_points) { set_error("null d_points"); return RM_ERR_INVALID_ARGUMENT; }
  if (((uintptr_t)c.d_points | (uintptr_t)c.d_view | (uintptr_t)c.d_surface | (uintptr_t)c.d_rgba) & 15u) {
    set_error("d_points, d_view, d_surface and d_rgba must be 16-byte aligned");
    return RM_ERR_INVALID_ARGUMENT;
  }
  if ((uintptr_t)c.d_ao & 3u) { set_error("d_ao must be 4-byte aligned"); return RM_ERR_INVALID_ARGUMENT; }
  if ((st = require_device_pointers({{"d_points", c.d_points}, {"d_view", c.d_view}, {"d_surface", c.d_surface}, {"d_ao", c.d_ao}})) != RM_OK)
    return st;
  return c.d_rgba ? check_device_pointers(c.res, c.d_rgba, nullptr) : RM_OK;
}
int launch_points(const PointsCall &c) {
  RmCamera cam{};
  if (c.ps) cam.initialFar = c.ps->far;
  int st = check_points(c, cam);
  if (st != RM_OK || c.numPoints == 0) return st;
  const bool plain = bulb_plain(c.objs, c.numObjects, c.g) != 0;
  int bulbClass = table_bulb_class(c.objs, c.numObjects, plain);
  bool tex = false;
  BlockCall b{c.objs, c.numObjects, c.g, c.s, c.stream, 17};
  b.cam = &cam;
  if (c.d_rgba) {
    const FrameClass fc = classify_frame(c.objs, c.numObjects, c.lights, c.numLights, c.g, c.s, 0);
    bulbClass = bulb_class(fc, plain);
    tex = fc.textured;
    b.lights = c.lights; b.numLights = c.numLights; b.res = &c.res;
  }
  return stage_block_launch(b, [&](const SceneBlock *sb, const SceneBlock *, void *) {
    return launch_points_kernel(sb, bulbClass, tex, c.d_points, c.d_view, c.numPoints, c.ps->projectSteps, c.ps->iso, c.ps->maxMove, c.d_surface,
                                c.d_ao, c.d_rgba, c.stream);
  });
}

// ---- the field on a lattice (rm_sdf_grid) ----------------------------------------------------------------------------------------
// rm_sdf_grid (the header has the definition): sdScene at the points of a dense lattice against ONE object table.  The checks run in
// the header's order, every one but the last ahead of the first HIP call: the pointers and the table's count, the lattice
// (check_lattice, which rm_sdf_mesh shares), the layers and the 2-D mode, check_trace's table checks, then d_dist and whether the
// outputs are device memory.  Staging is launch_trace's: stage_block_launch with one block of the batch ring, filled with a camera
// of zeros and no lights.  Then ONE launch of sdf_grid_kernel (rm_volume.hip) of the table's march class, path 16: no tuner,
// tile-order or workspace state is read or changed.
int launch_sdf_grid(const RmObject *objs, int numObjects, const RmGlobals *g, const RmSettings *s, const float *origin, const float *step,
                    int nx, int ny, int nz, float *d_dist, int32_t *d_objectId, hipStream_t stream) {
  if (!g || !s || !origin || !step) { set_error("null g, s, origin or step"); return RM_ERR_INVALID_ARGUMENT; }
  if ((numObjects > 0 && !objs) || numObjects < 0) { set_error("null object table or negative count"); return RM_ERR_INVALID_ARGUMENT; }
  int st = check_lattice(origin, step, nx, ny, nz);
  if (st != RM_OK) return st;
  if ((st = refuse_layers(s, "rm_sdf_grid evaluates the object table: TERRAIN / CLOUD / SEA are not part of the lattice")) != RM_OK) return st;
  if ((st = refuse_two_d(g, "the 2-D mode (isTwoD) has no distance field")) != RM_OK) return st;
  if ((st = check_object_table(objs, numObjects, s)) != RM_OK) return st;
  if (!d_dist) { set_error("null d_dist"); return RM_ERR_INVALID_ARGUMENT; }
  if ((st = require_device_pointers({{"d_dist", d_dist}, {"d_objectId", d_objectId}})) != RM_OK) return st;
  const int bulbClass = table_bulb_class(objs, numObjects, bulb_plain(objs, numObjects, g) != 0);
  return stage_block_launch(BlockCall{objs, numObjects, g, s, stream, 16}, [&](const SceneBlock *sb, const SceneBlock *, void *) {
    return launch_sdf_grid_kernel(sb, bulbClass, origin, step, nx, ny, nz, d_dist, d_objectId, stream);
  });
}

// ---- the field on the blocks of a virtual lattice (rm_sdf_blocks_select, rm_sdf_grid_blocks) -------------------------------------
// Both (the header has the definitions) are rm_sdf_grid on blocks of 8×8×8 cells: launch_sdf_grid's checks in its order with
// check_block_lattice in check_lattice's place and the call's own behind it, every one but the last ahead of the first HIP call;
// launch_sdf_grid's staging behind the stream's workspace (kWsBlocks; BlockCall::workspaceBytes), which stage_block_launch takes
// under the device's lock as launch_adaptive takes its own.  rm_sdf_blocks_select: one launch of blocks_eval_kernel (rm_blocks.hip)
// over every block of the lattice, which keeps a flag per block, and the compaction of the flags, path 18;
// rm_sdf_blocks_select_pruned: the same flags from the pruning kernels of rm_blocks.hip, which evaluate only the blocks near the
// surface, path 20.  rm_sdf_grid_blocks: the block map of the list (void entries), then one launch of blocks_eval_kernel over the
// list's entries, path 19.
struct BlocksCall {
  const RmObject *objs; int numObjects; const RmGlobals *g; const RmSettings *s; const float *origin, *step; int mx, my, mz;
  hipStream_t stream;
  // the staging of the call, with `bytes` of the kWsBlocks workspace
  BlockCall staged(int path, size_t bytes) const {
    BlockCall b{objs, numObjects, g, s, stream, path};
    b.workspaceBytes = bytes;
    return b;
  }
  int bulbClass() const { return table_bulb_class(objs, numObjects, bulb_plain(objs, numObjects, g) != 0); }
};
int check_blocks_scene(const BlocksCall &c, const char *layersText) {
  int st = refuse_layers(c.s, layersText);
  if (st != RM_OK || (st = refuse_two_d(c.g, "the 2-D mode (isTwoD) has no distance field")) != RM_OK) return st;
  return check_object_table(c.objs, c.numObjects, c.s);
}
int check_blocks_head(const BlocksCall &c) {
  if (!c.g || !c.s || !c.origin || !c.step) { set_error("null g, s, origin or step"); return RM_ERR_INVALID_ARGUMENT; }
  if ((c.numObjects > 0 && !c.objs) || c.numObjects < 0) { set_error("null object table or negative count"); return RM_ERR_INVALID_ARGUMENT; }
  return check_block_lattice(c.origin, c.step, c.mx, c.my, c.mz);
}
// lipschitz: null for rm_sdf_blocks_select; (lipschitzOut, lipschitzIn) for rm_sdf_blocks_select_pruned, which has the same checks
// with its own between iso and maxBlocks, the same staging, the pruning kernels of rm_blocks.hip and path 20.
int launch_sdf_blocks_select(const BlocksCall &c, float iso, const float *lipschitz, int maxBlocks, int32_t *d_blocks, uint32_t *d_count) {
  int st = check_blocks_head(c);
  if (st != RM_OK) return st;
  if (!(iso - iso == 0.0f)) { set_error("iso must be finite"); return RM_ERR_INVALID_ARGUMENT; }
  if (lipschitz && !(lipschitz[0] >= 0.0f && lipschitz[1] >= 0.0f)) {
    set_error("lipschitzOut and lipschitzIn must not be NaN or negative (+inf: that side discards nothing)");
    return RM_ERR_INVALID_ARGUMENT;
  }
  if (maxBlocks < 0) { set_error("negative maxBlocks"); return RM_ERR_INVALID_ARGUMENT; }
  if ((st = check_blocks_scene(c, "rm_sdf_blocks_select evaluates the object table: TERRAIN / CLOUD / SEA are not part of the lattice")) != RM_OK)
    return st;
  if ((maxBlocks > 0 && !d_blocks) || !d_count) { set_error("null d_count, or null d_blocks with maxBlocks above 0"); return RM_ERR_INVALID_ARGUMENT; }
  if ((st = require_device_pointers({{"d_blocks", d_blocks}, {"d_count", d_count}})) != RM_OK) return st;
  const int bulbClass = c.bulbClass();
  if (lipschitz)
    return stage_block_launch(c.staged(20, blocks_prune_workspace(c.mx, c.my, c.mz)), [&](const SceneBlock *sb, const SceneBlock *, void *mem) {
      return launch_blocks_prune_kernels(sb, bulbClass, c.origin, c.step, c.mx, c.my, c.mz, iso, lipschitz[0], lipschitz[1], maxBlocks, d_blocks,
                                         d_count, mem, c.stream);
    });
  return stage_block_launch(c.staged(18, blocks_select_workspace(c.mx, c.my, c.mz)), [&](const SceneBlock *sb, const SceneBlock *, void *mem) {
    return launch_blocks_select_kernels(sb, bulbClass, c.origin, c.step, c.mx, c.my, c.mz, iso, maxBlocks, d_blocks, d_count, mem, c.stream);
  });
}
int launch_sdf_grid_blocks(const BlocksCall &c, const int32_t *d_blocks, int numBlocks, float *d_dist, int32_t *d_objectId) {
  int st = check_blocks_head(c);
  if (st != RM_OK) return st;
  if (numBlocks < 0 || numBlocks > RM_MAX_BLOCK_LIST) { set_error("numBlocks must be 0 … RM_MAX_BLOCK_LIST"); return RM_ERR_INVALID_ARGUMENT; }
  if ((st = check_blocks_scene(c, "rm_sdf_grid_blocks evaluates the object table: TERRAIN / CLOUD / SEA are not part of the lattice")) != RM_OK)
    return st;
  if (numBlocks == 0) return RM_OK;
  if (!d_blocks || !d_dist) { set_error("null d_blocks or d_dist"); return RM_ERR_INVALID_ARGUMENT; }
  if ((st = require_device_pointers({{"d_blocks", d_blocks}, {"d_dist", d_dist}, {"d_objectId", d_objectId}})) != RM_OK) return st;
  const int bulbClass = c.bulbClass();
  return stage_block_launch(c.staged(19, blocks_map_workspace(c.mx, c.my, c.mz)), [&](const SceneBlock *sb, const SceneBlock *, void *mem) {
    return launch_blocks_grid_kernels(sb, bulbClass, c.origin, c.step, c.mx, c.my, c.mz, d_blocks, numBlocks, d_dist, d_objectId, mem, c.stream);
  });
}

// The scene evaluator's probes (rm_probe_sdscene*, rm_probe_pool_cull): the table staged as a frame's (zero camera, no resources) on
// the ring of single frames.  A probe is no timed launch and leaves rm_debug_last_path alone: only the slot's event follows it.
BlockCall probe_call(const RmObject *objs, int numObjects, const RmGlobals *g, const RmSettings *s, hipStream_t stream) {
  BlockCall b{objs, numObjects, g, s, stream, 0};
  b.singleFrameRing = true; b.timed = false;
  return b;
}
}  // namespace
}  // namespace rm

using namespace rm;

extern "C" {

int rm_trace_rays(const RmRay *d_rays, int numRays, const RmObject *objs, int numObjects, const RmGlobals *g, const RmSettings *s,
                  unsigned mode, RmRayHit *d_hits, void *stream) {
  return launch_trace(TraceCall{d_rays, numRays, objs, numObjects, g, s, mode, d_hits, static_cast<hipStream_t>(stream)});
}

int rm_shade_rays(const RmRay *d_rays, int numRays, float far, const RmObject *objs, int numObjects, const RmLight *lights, int numLights,
                  const RmGlobals *g, const RmSettings *s, const RmResources *res, float *d_rgba, float *d_bright, void *stream) {
  return launch_shade(ShadeCall{d_rays, numRays, far, objs, numObjects, lights, numLights, g, s, res ? *res : kNoResources, d_rgba, d_bright,
                                static_cast<hipStream_t>(stream)});
}

int rm_shade_rays_layers(const RmRay *d_rays, int numRays, float far, int imageWidth, const RmObject *objs, int numObjects,
                         const RmLight *lights, int numLights, const RmGlobals *g, const RmSettings *s, const RmResources *res, float *d_rgba,
                         float *d_bright, void *stream) {
  return launch_shade(ShadeCall{d_rays, numRays, far, objs, numObjects, lights, numLights, g, s, res ? *res : kNoResources, d_rgba, d_bright,
                                static_cast<hipStream_t>(stream), true, imageWidth});
}

int rm_trace_rays_layers(const RmRay *d_rays, int numRays, int imageWidth, const RmObject *objs, int numObjects, const RmGlobals *g,
                         const RmSettings *s, unsigned mode, RmRayHit *d_hits, void *stream) {
  return launch_trace(TraceCall{d_rays, numRays, objs, numObjects, g, s, mode, d_hits, static_cast<hipStream_t>(stream), true, imageWidth});
}

int rm_light_probes(const float *d_positions, int numProbes, const RmProbeDir *d_dirs, int numDirs, int numSets, float far,
                    const RmObject *objs, int numObjects, const RmLight *lights, int numLights, const RmGlobals *g, const RmSettings *s,
                    const RmResources *res, RmLightProbe *d_out, void *stream) {
  return launch_probes(ProbesCall{d_positions, numProbes, d_dirs, numDirs, numSets, far, objs, numObjects, lights, numLights, g, s,
                                  res ? *res : kNoResources, d_out, static_cast<hipStream_t>(stream)});
}

int rm_shade_rays_indirect(const RmRay *d_rays, int numRays, float far, const RmObject *objs, int numObjects, const RmLight *lights,
                           int numLights, const RmGlobals *g, const RmSettings *s, const RmResources *res, const RmLightGridRef *grid,
                           float *d_rgba, void *stream) {
  return launch_shade_indirect(ShadeCall{d_rays, numRays, far, objs, numObjects, lights, numLights, g, s, res ? *res : kNoResources, d_rgba,
                                         nullptr, static_cast<hipStream_t>(stream)}, grid);
}

int rm_light_probes_indirect(const float *d_positions, int numProbes, const RmProbeDir *d_dirs, int numDirs, int numSets, float far,
                             const RmObject *objs, int numObjects, const RmLight *lights, int numLights, const RmGlobals *g,
                             const RmSettings *s, const RmResources *res, const RmLightGridRef *grid, RmLightProbe *d_out, void *stream) {
  return launch_probes_indirect(ProbesCall{d_positions, numProbes, d_dirs, numDirs, numSets, far, objs, numObjects, lights, numLights, g, s,
                                           res ? *res : kNoResources, d_out, static_cast<hipStream_t>(stream)}, grid);
}

// rm_sphere_directions (the header has the definition): host only, binary64 rounded once.  Spherical Fibonacci points and, per
// point, 4π / numDirs times the nine real spherical harmonics of bands 0 to 2.
int rm_sphere_directions(int numDirs, int numSets, RmProbeDir *out) {
  if (int st = check_probe_table(numDirs, numSets)) return st;
  if (!out) { set_error("null out"); return RM_ERR_INVALID_ARGUMENT; }
  const double K = (double)numDirs, pi = 3.14159265358979323846, twoPi = 2.0 * pi, w = 4.0 * pi / K;
  const double c0 = std::sqrt(1.0 / (4.0 * pi)), c1 = std::sqrt(3.0 / (4.0 * pi)), c2 = std::sqrt(15.0 / (4.0 * pi)),
               c20 = std::sqrt(5.0 / (16.0 * pi)), c22 = std::sqrt(15.0 / (16.0 * pi));
  for (int s = 0; s < numSets; s++)
    for (int k = 0; k < numDirs; k++) {
      const double z = 1.0 - (2.0 * (double)k + 1.0) / K, r = std::sqrt(1.0 - z * z);
      const double turn = (double)k * 0.6180339887498949 + (double)s * 0.7548776662466927, phi = twoPi * (turn - std::floor(turn));
      const double x = r * std::cos(phi), y = r * std::sin(phi);
      const double Y[9] = {c0, c1 * y, c1 * z, c1 * x, c2 * (x * y), c2 * (y * z), c20 * (3.0 * (z * z) - 1.0), c2 * (x * z), c22 * (x * x - y * y)};
      RmProbeDir &e = out[(size_t)s * (size_t)numDirs + (size_t)k];
      e.dir[0] = (float)x, e.dir[1] = (float)y, e.dir[2] = (float)z, e.reserved = 0.0f;
      for (int j = 0; j < 9; j++) e.basis[j] = (float)(w * Y[j]);
      e.pad[0] = e.pad[1] = e.pad[2] = 0.0f;
    }
  return RM_OK;
}

int rm_light_probes_depth(const float *d_positions, int numProbes, const RmProbeDir *d_dirs, const float *d_weights, int numDirs,
                          int numSets, float maxDistance, const RmObject *objs, int numObjects, const RmGlobals *g, const RmSettings *s,
                          RmProbeDepth *d_out, void *stream) {
  return launch_probes_depth(ProbesDepthCall{d_positions, numProbes, d_dirs, d_weights, numDirs, numSets, maxDistance, objs, numObjects, g, s,
                                             d_out, static_cast<hipStream_t>(stream)});
}

// rm_probe_depth_weights (the header has the definition): host only, binary64 rounded once.  Per set and texel the rows' lobes
// max(0, cos)^sharpness around the texel's centre direction, normalised over the set's valid rows; a texel that no lobe reaches
// goes to the nearest row whole.
int rm_probe_depth_weights(const RmProbeDir *dirs, int numDirs, int numSets, float sharpness, float *out) {
  if (int st = check_probe_table(numDirs, numSets)) return st;
  if (!dirs || !out) { set_error("null dirs or out"); return RM_ERR_INVALID_ARGUMENT; }
  if (!std::isfinite(sharpness) || sharpness < 0.0f) { set_error("sharpness must be finite and not negative"); return RM_ERR_INVALID_ARGUMENT; }
  double centre[RM_PROBE_DEPTH_TEXELS][3];
  for (int x = 0; x < RM_PROBE_DEPTH_TEXELS; x++) {
    const double u = (((double)(x % 8) + 0.5) / 8.0) * 2.0 - 1.0, v = (((double)(x / 8) + 0.5) / 8.0) * 2.0 - 1.0;
    const double z = 1.0 - std::fabs(u) - std::fabs(v);
    double cx = u, cy = v;
    if (z < 0.0) cx = (1.0 - std::fabs(v)) * (u >= 0.0 ? 1.0 : -1.0), cy = (1.0 - std::fabs(u)) * (v >= 0.0 ? 1.0 : -1.0);
    const double len = std::sqrt(cx * cx + cy * cy + z * z);
    centre[x][0] = cx / len, centre[x][1] = cy / len, centre[x][2] = z / len;
  }
  std::vector<double> dots((size_t)numDirs * RM_PROBE_DEPTH_TEXELS);
  std::vector<char> valid((size_t)numDirs);
  for (int s = 0; s < numSets; s++) {
    const RmProbeDir *rows = dirs + (size_t)s * (size_t)numDirs;
    float *w = out + (size_t)s * (size_t)numDirs * RM_PROBE_DEPTH_TEXELS;
    for (int k = 0; k < numDirs; k++) {
      const float *d = rows[k].dir;
      valid[k] = std::isfinite(d[0]) && std::isfinite(d[1]) && std::isfinite(d[2]) && (d[0] != 0.0f || d[1] != 0.0f || d[2] != 0.0f);
      if (!valid[k]) continue;
      const double dx = d[0], dy = d[1], dz = d[2], len = std::sqrt(dx * dx + dy * dy + dz * dz);
      for (int x = 0; x < RM_PROBE_DEPTH_TEXELS; x++)
        dots[(size_t)k * RM_PROBE_DEPTH_TEXELS + x] = centre[x][0] * (dx / len) + centre[x][1] * (dy / len) + centre[x][2] * (dz / len);
    }
    for (int x = 0; x < RM_PROBE_DEPTH_TEXELS; x++) {
      double sum = 0.0, best = -__builtin_inf();
      int nearest = -1;
      for (int k = 0; k < numDirs; k++) {
        if (!valid[k]) continue;
        const double dot = dots[(size_t)k * RM_PROBE_DEPTH_TEXELS + x];
        sum += std::pow(dot > 0.0 ? dot : 0.0, (double)sharpness);
        if (dot > best) best = dot, nearest = k;
      }
      for (int k = 0; k < numDirs; k++) {
        float &o = w[(size_t)k * RM_PROBE_DEPTH_TEXELS + x];
        if (!valid[k]) o = 0.0f;
        else if (sum == 0.0) o = k == nearest ? 1.0f : 0.0f;
        else {
          const double dot = dots[(size_t)k * RM_PROBE_DEPTH_TEXELS + x];
          o = (float)(std::pow(dot > 0.0 ? dot : 0.0, (double)sharpness) / sum);
        }
      }
    }
  }
  return RM_OK;
}

void rm_points_settings_default(RmPointsSettings *ps) {
  if (!ps) return;
  ps->far = 100.0f;
  ps->iso = 0.001f;
  ps->maxMove = __builtin_inff();
  ps->projectSteps = 0;
}
int rm_shade_points(const float *d_points, const float *d_view, int numPoints, const RmPointsSettings *ps, const RmObject *objs,
                    int numObjects, const RmLight *lights, int numLights, const RmGlobals *g, const RmSettings *s, const RmResources *res,
                    RmSurfacePoint *d_surface, float *d_ao, float *d_rgba, void *stream) {
  return launch_points(PointsCall{d_points, d_view, numPoints, ps, objs, numObjects, lights, numLights, g, s, res ? *res : kNoResources,
                                  d_surface, d_ao, d_rgba, static_cast<hipStream_t>(stream)});
}

int rm_sdf_grid(const RmObject *objs, int numObjects, const RmGlobals *g, const RmSettings *s, const float origin[3], const float step[3],
                int nx, int ny, int nz, float *d_dist, int32_t *d_objectId, void *stream) {
  return launch_sdf_grid(objs, numObjects, g, s, origin, step, nx, ny, nz, d_dist, d_objectId, static_cast<hipStream_t>(stream));
}

int rm_sdf_blocks_select(const RmObject *objs, int numObjects, const RmGlobals *g, const RmSettings *s, const float origin[3],
                         const float step[3], int mx, int my, int mz, float iso, int maxBlocks, int32_t *d_blocks, uint32_t *d_count,
                         void *stream) {
  return launch_sdf_blocks_select(BlocksCall{objs, numObjects, g, s, origin, step, mx, my, mz, static_cast<hipStream_t>(stream)}, iso, nullptr,
                                  maxBlocks, d_blocks, d_count);
}

int rm_sdf_blocks_select_pruned(const RmObject *objs, int numObjects, const RmGlobals *g, const RmSettings *s, const float origin[3],
                                const float step[3], int mx, int my, int mz, float iso, float lipschitzOut, float lipschitzIn, int maxBlocks,
                                int32_t *d_blocks, uint32_t *d_count, void *stream) {
  const float lipschitz[2] = {lipschitzOut, lipschitzIn};
  return launch_sdf_blocks_select(BlocksCall{objs, numObjects, g, s, origin, step, mx, my, mz, static_cast<hipStream_t>(stream)}, iso, lipschitz,
                                  maxBlocks, d_blocks, d_count);
}

int rm_sdf_grid_blocks(const RmObject *objs, int numObjects, const RmGlobals *g, const RmSettings *s, const float origin[3],
                       const float step[3], int mx, int my, int mz, const int32_t *d_blocks, int numBlocks, float *d_dist,
                       int32_t *d_objectId, void *stream) {
  return launch_sdf_grid_blocks(BlocksCall{objs, numObjects, g, s, origin, step, mx, my, mz, static_cast<hipStream_t>(stream)}, d_blocks,
                                numBlocks, d_dist, d_objectId);
}

int rm_probe_math(int fn, const float *d_x, const float *d_y, const float *d_z, float *d_out, int n, void *stream) {
  if (fn < 0 || fn >= RM_FN_COUNT || !d_x || !d_out || n < 0) { set_error("bad probe arguments"); return RM_ERR_INVALID_ARGUMENT; }
  if (int st = require_device_pointers({{"d_x", d_x}, {"d_y", d_y}, {"d_z", d_z}, {"d_out", d_out}})) return st;
  if (n == 0) return RM_OK;
  return launch_probe_math(fn, d_x, d_y, d_z, d_out, n, static_cast<hipStream_t>(stream));
}

int rm_probe_bump(const float *d_pts, float *d_out, int n, void *stream) {
  if (!d_pts || !d_out || n < 0) { set_error("bad probe arguments"); return RM_ERR_INVALID_ARGUMENT; }
  if (int st = require_device_pointers({{"d_pts", d_pts}, {"d_out", d_out}})) return st;
  if (n == 0) return RM_OK;
  return launch_probe_bump(d_pts, d_out, n, static_cast<hipStream_t>(stream));
}

int rm_probe_sdscene(const RmObject *objs, int numObjects, const RmGlobals *g, const RmSettings *s, const float *d_pts,
                     float *d_out, int n, void *stream) {
  RmCamera cam{};
  int st = validate_scene(&cam, objs, numObjects, nullptr, 0, g, s, kNoResources);
  if (st != RM_OK) return st;
  if (!d_pts || !d_out || n < 0) { set_error("bad probe arguments"); return RM_ERR_INVALID_ARGUMENT; }
  if (int st2 = require_device_pointers({{"d_pts", d_pts}, {"d_out", d_out}})) return st2;
  if (n == 0) return RM_OK;
  const hipStream_t hs = static_cast<hipStream_t>(stream);
  return stage_block_launch(probe_call(objs, numObjects, g, s, hs), [&](const SceneBlock *sb, const SceneBlock *, void *) {
    return launch_probe_sdscene(sb, d_pts, d_out, n, hs);
  });
}

int rm_probe_sdscene_variant(const RmObject *objs, int numObjects, const RmGlobals *g, const RmSettings *s, int bulbClass,
                             int count, int trap, int skip, int track, int one, const float *d_pts, const float *d_ub,
                             float *d_out, int n, void *stream) {
  RmCamera cam{};
  int st = validate_scene(&cam, objs, numObjects, nullptr, 0, g, s, kNoResources);
  if (st != RM_OK) return st;
  auto bad = [](const char *msg) { set_error(msg); return (int)RM_ERR_INVALID_ARGUMENT; };
  if (!sdscene_variant_exists(bulbClass, count, trap, skip, track, one >= 0))
    return bad("no production kernel instantiates this sdScene variant");
  if (bulbClass != 0 && (numObjects != 1 || objs[0].type != RM_MANDELBULB)) return bad("a bulb class needs a table of one Mandelbulb");
  if (bulbClass == kBulbPlain && !bulb_plain(objs, numObjects, g)) return bad("the plain bulb form does not apply to this table");
  if (one < -1 || one >= numObjects || (one >= 0 && !(objs[one].type >= RM_CUBE && objs[one].type <= RM_RECTANGLE)))
    return bad("`one` must name a primitive of the table");
  if (!d_pts || !d_out || n < 0) return bad("bad probe arguments");
  if (int st2 = require_device_pointers({{"d_pts", d_pts}, {"d_ub", d_ub}, {"d_out", d_out}})) return st2;
  if (n == 0) return RM_OK;
  const hipStream_t hs = static_cast<hipStream_t>(stream);
  return stage_block_launch(probe_call(objs, numObjects, g, s, hs), [&](const SceneBlock *sb, const SceneBlock *, void *) {
    return launch_sdscene_variant(sb, bulbClass, count, trap, skip, track, one, d_pts, d_ub, d_out, n, hs);
  });
}

int rm_probe_pool_cull(const RmObject *objs, int numObjects, const RmLight *lights, int numLights, const RmGlobals *g,
                       const RmSettings *s, int bulbClass, int light, float far, const float *d_pts, float *d_out, int n, void *stream) {
  RmCamera cam{};
  int st = validate_scene(&cam, objs, numObjects, lights, numLights, g, s, kNoResources);
  if (st != RM_OK) return st;
  auto bad = [](const char *msg) { set_error(msg); return (int)RM_ERR_INVALID_ARGUMENT; };
  if (bulbClass != kBulbGeneral && bulbClass != kBulbPlain) return bad("bulbClass must be 1 (general) or 2 (plain)");
  if (numObjects != 1 || objs[0].type != RM_MANDELBULB) return bad("a bulb class needs a table of one Mandelbulb");
  if (bulbClass == kBulbPlain && !bulb_plain(objs, numObjects, g)) return bad("the plain bulb form does not apply to this table");
  if (light < 0 || light >= numLights || lights[light].type != RM_LIGHT_DIRECTIONAL) return bad("`light` must name a directional light of the table");
  if (!d_pts || !d_out || n < 0) return bad("bad probe arguments");
  if (int st2 = require_device_pointers({{"d_pts", d_pts}, {"d_out", d_out}})) return st2;
  if (n == 0) return RM_OK;
  const hipStream_t hs = static_cast<hipStream_t>(stream);
  BlockCall b = probe_call(objs, numObjects, g, s, hs);
  b.lights = lights; b.numLights = numLights;
  return stage_block_launch(b, [&](const SceneBlock *sb, const SceneBlock *, void *) {
    return launch_probe_pool_cull(sb, bulbClass, light, far, d_pts, d_out, n, hs);
  });
}

}  // extern "C"
