// rm_frame.cpp — the host-only scene prep of a launch: what is checked, derived and decided from the caller's tables before
// anything reaches the GPU.  validate_scene; the SceneBlock fields that fill_frames derives (cull ball and box, per-object
// balls, evaluation records, ray planes, the plain-bulb flag); the class of a frame (classify_frame, wavefront_pays) and
// the key its picture is remembered by.  No HIP: plain C++, built with the library's flags (-ffp-contract=off: the binary64
// bounds and the explicit fmaf chain are pinned bit for bit by tests) and, for tests/host_fuzz, under ASan + UBSan.
#include "rm_frame.h"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>

#include "rm_wavefront.h"

namespace rm {

// A knob for A/B runs (the defaults are the measured best), read once per process by its caller (a static): `def` if the variable
// is unset, otherwise atoi of its text (0 when empty), clamped to [lo, hi].  Where an rm_* call sets the same thing (the g_* atomics
// of rm_launcher.hip), the call takes precedence.
int env_int(const char *name, int def, int lo, int hi) {
  const char *e = std::getenv(name);
  const int v = e ? std::atoi(e) : def;
  return v < lo ? lo : (v > hi ? hi : v);
}

namespace {
bool tex_ok(const RmTexture &t) { return t.pixels && t.width > 0 && t.height > 0; }
}  // namespace

// object i's type is one the kernels evaluate
static int check_object_type(const RmObject *objs, int i) {
  if (objs[i].type >= 0 && objs[i].type < RM_CUSTOM) return RM_OK;
  set_error("object " + std::to_string(i) + ": CUSTOM / unknown type (the reference's sdCUSTOM returns an unset value)");
  return RM_ERR_UNSUPPORTED;
}
int check_object_table(const RmObject *objs, int numObjects, const RmSettings *s) {
  if (numObjects > RM_MAX_OBJECTS) { set_error("scene exceeds RM_MAX_OBJECTS"); return RM_ERR_CAPACITY; }
  if (s->maxSteps < 0 || s->fractalIters < 0 || s->mengerLevels < 0) {
    set_error("negative loop bound in RmSettings");
    return RM_ERR_INVALID_ARGUMENT;
  }
  for (int i = 0; i < numObjects; i++)
    if (int st = check_object_type(objs, i)) return st;
  return RM_OK;
}

int validate_scene(const RmCamera *cam, const RmObject *objs, int numObjects, const RmLight *lights, int numLights,
                   const RmGlobals *g, const RmSettings *s, const RmResources &res) {
  const RmTexture *tex = res.textures;
  const int numTex = res.numTextures;
  if (numTex < 0 || (numTex > 0 && !tex)) { set_error("bad texture table"); return RM_ERR_INVALID_ARGUMENT; }
  if (numTex > RM_MAX_TEXTURES) { set_error("more than RM_MAX_TEXTURES textures"); return RM_ERR_CAPACITY; }
  if (!cam || !g || !s || (numObjects > 0 && !objs) || (numLights > 0 && !lights) || numObjects < 0 || numLights < 0) {
    set_error("null scene pointer or negative count");
    return RM_ERR_INVALID_ARGUMENT;
  }
  if (numObjects > RM_MAX_OBJECTS || numLights > RM_MAX_LIGHTS) {
    set_error("scene exceeds RM_MAX_OBJECTS / RM_MAX_LIGHTS");
    return RM_ERR_CAPACITY;
  }
  if (s->maxSteps < 0 || s->fractalIters < 0 || s->mengerLevels < 0 || s->numReflection < 0) {
    set_error("negative loop bound in RmSettings");
    return RM_ERR_INVALID_ARGUMENT;
  }
  if ((s->features & (RM_FEAT_NIGHTSKY_BACKGROUND | RM_FEAT_SEA)) && !tex_ok(res.noise)) {
    set_error("NIGHTSKY_BACKGROUND / SEA read the noise texture: supply RmResources.noise (rm_render_res)");
    return RM_ERR_UNSUPPORTED;
  }
  if (s->enableSkyBox) {
    for (int f = 0; f < 6; f++)
      if (!tex_ok(res.skybox[f])) {
        set_error("enableSkyBox without six cube-map faces in RmResources.skybox (rm_render_res)");
        return RM_ERR_UNSUPPORTED;
      }
  }
  for (int i = 0; i < numObjects; i++) {
    if (int st = check_object_type(objs, i)) return st;
    if (objs[i].texLoc != -1) {
      const int t = objs[i].texLoc, ty = objs[i].type;
      if (t < 0 || t >= numTex) {
        set_error("object " + std::to_string(i) + ": texLoc without a matching texture (use rm_render_ex)");
        return RM_ERR_UNSUPPORTED;
      }
      if (ty != RM_CUBE && ty != RM_CONE && ty != RM_CYLINDER && ty != RM_SPHERE) {
        set_error("object " + std::to_string(i) + ": textures are only defined for cube, cone, cylinder, sphere");
        return RM_ERR_UNSUPPORTED;
      }
      if (!tex_ok(tex[t])) {
        set_error("texture " + std::to_string(t) + ": null pixels or empty size");
        return RM_ERR_INVALID_ARGUMENT;
      }
    }
  }
  for (int i = 0; i < numLights; i++) {
    if (lights[i].type < 0 || lights[i].type > RM_LIGHT_AREA) {
      set_error("light " + std::to_string(i) + ": unknown light type");
      return RM_ERR_UNSUPPORTED;
    }
    if (lights[i].type == RM_LIGHT_AREA && (!res.ltc1 || !res.ltc2)) {
      set_error("light " + std::to_string(i) + ": area lights read the LTC tables: supply RmResources.ltc1/ltc2 (rm_render_res)");
      return RM_ERR_UNSUPPORTED;
    }
  }
  return RM_OK;
}

// A world-space ball that contains every object, grown by a margin δ such that outside it every object's distance value
// exceeds the hit threshold by a wide factor (so a march out there can only miss).  Per object: unit-shape radius r in
// object space (sdMatch's sizes, frag:1262-1293), world centre c = −A⁻¹b and extent r·σ(A⁻¹) of the ball's image under
// the model matrix (A, b = linear part and translation of invModel; σ = largest singular value), and κ = scaleFactor / σ(A⁻¹), a lower bound of
// (distance value) / (world distance to the object's ball) for the exact SDFs.  The Mandelbulb (power 8, |seed| <= 2)
// enters with r = 2.1: beyond it the estimate is >= 0.68·scaleFactor.  Scenes with a type that has no bound here
// (2-D Mandelbrot, Sierpinski) get cullOk = 0.
// Largest singular value of a 3×3 matrix: the largest eigenvalue of the symmetric M·Mᵀ in closed form, padded.
double sigma_max3(const double m[3][3]) {
  double B[3][3];
  for (int r0 = 0; r0 < 3; r0++)
    for (int c0 = 0; c0 < 3; c0++) B[r0][c0] = m[r0][0] * m[c0][0] + m[r0][1] * m[c0][1] + m[r0][2] * m[c0][2];
  const double p1 = B[0][1] * B[0][1] + B[0][2] * B[0][2] + B[1][2] * B[1][2];
  const double q = (B[0][0] + B[1][1] + B[2][2]) / 3.0;
  const double p2 = (B[0][0] - q) * (B[0][0] - q) + (B[1][1] - q) * (B[1][1] - q) + (B[2][2] - q) * (B[2][2] - q) + 2.0 * p1;
  double lmax;
  if (!(p2 > 1e-300)) lmax = q;
  else {
    const double pp = std::sqrt(p2 / 6.0);
    double C3[3][3];
    for (int r0 = 0; r0 < 3; r0++)
      for (int c0 = 0; c0 < 3; c0++) C3[r0][c0] = (B[r0][c0] - (r0 == c0 ? q : 0.0)) / pp;
    double hd = (C3[0][0] * (C3[1][1] * C3[2][2] - C3[1][2] * C3[2][1]) - C3[0][1] * (C3[1][0] * C3[2][2] - C3[1][2] * C3[2][0]) +
                 C3[0][2] * (C3[1][0] * C3[2][1] - C3[1][1] * C3[2][0])) / 2.0;
    hd = hd < -1.0 ? -1.0 : (hd > 1.0 ? 1.0 : hd);
    lmax = q + 2.0 * pp * std::cos(std::acos(hd) / 3.0);
  }
  return std::sqrt(lmax > 0.0 ? lmax : 0.0) * (1.0 + 1e-6);
}

void scene_cull_ball(SceneBlock *h) {
  h->cullOk = 0;
  h->objBallOk = 0;
  h->cullC[0] = h->cullC[1] = h->cullC[2] = 0.0f;
  h->cullR2 = 0.0f;
  h->cullR2Soft = 0.0f;
  h->cullBoxOk = 0;
  for (int k = 0; k < 3; k++) h->cullLo[k] = h->cullHi[k] = 0.0f;
  {  // Lipschitz bound of the distance values per unit of world length (the skip test's seed, rm_device.hip.h nextMinBound):
     // scaleFactor × the stretch of invModel's linear part, for the shapes whose SDF is 1-Lipschitz in object space
    double lip = 0.0;
    for (int i = 0; i < h->numObjects; i++) {
      const RmObject &o = h->objs[i];
      const bool lipschitz = (o.type >= RM_CUBE && o.type <= RM_RECTANGLE) || o.type == RM_MENGERSPONGE;
      const float *M = o.invModel;
      const double a[3][3] = {{M[0], M[4], M[8]}, {M[1], M[5], M[9]}, {M[2], M[6], M[10]}};
      const double li = lipschitz ? std::fabs((double)o.scaleFactor) * sigma_max3(a) : INFINITY;
      lip = (li > lip || !(li == li)) ? li : lip;
    }
    h->cullLip = (std::isfinite(lip) && lip < 1e6) ? (float)(lip * (1.0 + 1e-5)) : INFINITY;
    bool prim = h->numObjects > 0;
    for (int i = 0; i < h->numObjects; i++) prim = prim && h->objs[i].type >= RM_CUBE && h->objs[i].type <= RM_RECTANGLE;
    h->cullOneOk = (prim && std::isfinite(h->cullLip)) ? 1 : 0;
  }
  const int n = h->numObjects;
  if (n <= 0) return;
  // half-extents of the unit shapes' object-space bounding boxes (sdMatch's sizes; the capsule's segment runs from 0 to 0.5 in y)
  static const double kExtent[][3] = {{.5, .5, .5}, {.5, .5, .5}, {.5, .5, .5}, {.5, .5, .5}, {.5, .5, .5}, {.625, .125, .625},
                                      {.1, .6, .1}, {.5, .5, .5}, {.5, .5, 0.0}};  // cube … rectangle
  double lo[3] = {1e30, 1e30, 1e30}, hi[3] = {-1e30, -1e30, -1e30};
  static const double kRadius[] = {0.8661, 0.7072, 0.7072, 0.5001, 0.5001, 0.6251, 0.6001, 0.5001, 0.7072};  // cube … rectangle
  double cx[RM_MAX_OBJECTS], cy[RM_MAX_OBJECTS], cz[RM_MAX_OBJECTS], rad[RM_MAX_OBJECTS];
  double kappa = 1e30, kappaSoft = 1e30, C[3] = {0, 0, 0};
  for (int i = 0; i < n; i++) {
    const RmObject &o = h->objs[i];
    double r;
    if (o.type >= RM_CUBE && o.type <= RM_RECTANGLE) r = kRadius[o.type];
    else if (o.type == RM_MENGERSPONGE) r = 1.7322;
    else if (o.type == RM_MANDELBULB) {
      const double jx = h->g.juliaSeed[0], jy = h->g.juliaSeed[1];
      if (!(h->g.power == 8.0f) || !(jx * jx + jy * jy <= 4.0) || !(o.scaleFactor >= 0.01f)) return;
      r = 2.1;
    } else return;
    const float *M = o.invModel;
    const double a[3][3] = {{M[0], M[4], M[8]}, {M[1], M[5], M[9]}, {M[2], M[6], M[10]}};  // a[row][col]
    const double det = a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0]) +
                       a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]);
    if (!(std::fabs(det) > 1e-12) || !std::isfinite(det)) return;
    double inv[3][3];
    inv[0][0] = (a[1][1] * a[2][2] - a[1][2] * a[2][1]) / det; inv[0][1] = (a[0][2] * a[2][1] - a[0][1] * a[2][2]) / det;
    inv[0][2] = (a[0][1] * a[1][2] - a[0][2] * a[1][1]) / det; inv[1][0] = (a[1][2] * a[2][0] - a[1][0] * a[2][2]) / det;
    inv[1][1] = (a[0][0] * a[2][2] - a[0][2] * a[2][0]) / det; inv[1][2] = (a[0][2] * a[1][0] - a[0][0] * a[1][2]) / det;
    inv[2][0] = (a[1][0] * a[2][1] - a[1][1] * a[2][0]) / det; inv[2][1] = (a[0][1] * a[2][0] - a[0][0] * a[2][1]) / det;
    inv[2][2] = (a[0][0] * a[1][1] - a[0][1] * a[1][0]) / det;
    // nf = the largest singular value of A⁻¹ (how much the model matrix can stretch a length): the largest eigenvalue of the
    // symmetric B = A⁻¹·A⁻¹ᵀ in closed form, with a relative safety margin.  (The Frobenius norm used before is an upper bound
    // too, but √3 too large for a uniform scale: every ball was 1.7× wider than it had to be.)
    const double nf = sigma_max3(inv);
    const double b[3] = {M[12], M[13], M[14]};
    cx[i] = -(inv[0][0] * b[0] + inv[0][1] * b[1] + inv[0][2] * b[2]);
    cy[i] = -(inv[1][0] * b[0] + inv[1][1] * b[1] + inv[1][2] * b[2]);
    cz[i] = -(inv[2][0] * b[0] + inv[2][1] * b[1] + inv[2][2] * b[2]);
    rad[i] = r * nf;
    {
      double e[3] = {r, r, r};  // Menger sponge: the box of half-size 1 (r = √3 is its corner); Mandelbulb: the ball's box
      if (o.type >= RM_CUBE && o.type <= RM_RECTANGLE) for (int k = 0; k < 3; k++) e[k] = kExtent[o.type][k] + 1e-4;
      else if (o.type == RM_MENGERSPONGE) e[0] = e[1] = e[2] = 1.0001;
      const double c[3] = {cx[i], cy[i], cz[i]};
      for (int k = 0; k < 3; k++) {
        const double w = std::fabs(inv[k][0]) * e[0] + std::fabs(inv[k][1]) * e[1] + std::fabs(inv[k][2]) * e[2];
        lo[k] = std::fmin(lo[k], c[k] - w);
        hi[k] = std::fmax(hi[k], c[k] + w);
      }
    }
    const double ki = (double)o.scaleFactor / nf;
    if (!(ki > 1e-6) || !std::isfinite(rad[i]) || !std::isfinite(cx[i] + cy[i] + cz[i])) return;
    // hard bound: the bulb's constant 0.68·scaleFactor needs no δ; soft bound: beyond ρ = 2.1 its estimate ≈ 0.5·ρ·ln ρ has
    // slope >= 0.87 in object space
    if (o.type != RM_MANDELBULB) kappa = ki < kappa ? ki : kappa;
    const double ksi = (o.type == RM_MANDELBULB) ? 0.8 * ki : ki;
    kappaSoft = ksi < kappaSoft ? ksi : kappaSoft;
    C[0] += cx[i] / n; C[1] += cy[i] / n; C[2] += cz[i] / n;
  }
  for (int i = 0; i < n; i++) {  // the per-object balls, for the geometric tile order (the bulb's tight radius where it holds)
    const RmObject &o = h->objs[i];
    double r = rad[i];
    if (o.type == RM_MANDELBULB) {
      const double jx = h->g.juliaSeed[0], jy = h->g.juliaSeed[1];
      if (o.scaleFactor >= 0.05f && jx * jx + jy * jy <= 1.2996) r = rad[i] * (1.15 / 2.1);
    }
    h->objBall[i][0] = (float)cx[i]; h->objBall[i][1] = (float)cy[i]; h->objBall[i][2] = (float)cz[i]; h->objBall[i][3] = (float)r;
  }
  h->objBallOk = 1;
  double R = 0.0;
  for (int i = 0; i < n; i++) {
    const double d = std::sqrt((cx[i] - C[0]) * (cx[i] - C[0]) + (cy[i] - C[1]) * (cy[i] - C[1]) + (cz[i] - C[2]) * (cz[i] - C[2])) + rad[i];
    R = d > R ? d : R;
  }
  if (kappa > 1e29) kappa = 1.0;                         // only Mandelbulbs: any margin does
  const double delta = std::fmax(0.05, 4.0e-3 / kappa);  // κ·δ >= 4× the hit threshold
  R = (R + delta) * 1.001;
  if (!std::isfinite(R) || R > 1e6) return;
  h->cullC[0] = (float)C[0]; h->cullC[1] = (float)C[1]; h->cullC[2] = (float)C[2];
  h->cullR2 = (float)(R * R);
  h->cullOk = 1;
  // The same argument for the axis-aligned box around the objects' bounding boxes, grown by the same margin δ: a point outside
  // it is at least δ away from every object's box, so every distance value there exceeds 4× the hit threshold.  Hard-shadow,
  // primary and bounce marches end where their ray leaves ball ∩ box (flat or elongated scenes: the box is much tighter).
  bool boxOk = true;
  for (int k = 0; k < 3; k++) {
    const double m = delta * 1.001 + 1e-3 * std::fmax(std::fabs(lo[k]), std::fabs(hi[k]));
    lo[k] -= m; hi[k] += m;
    boxOk = boxOk && std::isfinite(lo[k]) && std::isfinite(hi[k]) && hi[k] > lo[k] && std::fabs(lo[k]) < 1e6 && std::fabs(hi[k]) < 1e6;
  }
  static const bool boxOn = env_int("RM_CULL_BOX", 1) != 0;
  // Only where the box is much tighter than the ball (flat or elongated scenes: a floor slab, a row of objects): for a compact
  // scene — the lone Menger cube of C5: box / ball volume 0.39 — the three reciprocals per ray cost more than the 5 % of
  // evaluations they save (measured: 21.9 -> 22.3 ms), while directional_light_2.json (0.07) executes 16 % fewer evaluations.
  const double volBox = (hi[0] - lo[0]) * (hi[1] - lo[1]) * (hi[2] - lo[2]), volBall = 4.18879 * R * R * R;
  boxOk = boxOk && volBox < 0.3 * volBall;
  if (boxOk && boxOn) {
    for (int k = 0; k < 3; k++) { h->cullLo[k] = (float)lo[k]; h->cullHi[k] = (float)hi[k]; }
    h->cullBoxOk = 1;
  }
  // Soft shadows: a shadow ray starts on a surface, i.e. inside the ball (radius R), and at distance ρ from the centre has
  // travelled t <= ρ + R while every distance value is >= κ·(ρ − R).  8·κ·(ρ − R) >= ρ + R  ⇔  ρ >= R·(8κ + 1)/(8κ − 1):
  // past that radius min(pen, 8·d/t) is settled.
  const double ks = kappaSoft;
  if (ks > 0.2 && ks < 1e29) {
    const double Rs = R * (8.0 * ks + 1.0) / (8.0 * ks - 1.0) * 1.001;
    if (std::isfinite(Rs) && Rs < 1e6) h->cullR2Soft = (float)(Rs * Rs);
  }
}

// nearClip / farClip (raymarch.vert:23-24) at the corners of the full-screen quad, as the vertex shader computes them, per
// triangle: P0, P1 − P0, P2 − P0 with P0 = (sg, sg), P1 = (−sg, sg), P2 = (sg, −sg), sg = −1 below the TL-BR diagonal and
// +1 above it.  invProjView·(x, y, z, 1) = ((M0·x + M1·y) + M2·z) + M3, fused — the oracle's mat4_mul_v4, on the host's
// binary32 FMA (the same bits on any IEEE machine).
namespace {
void ray_planes_of(const float *M, float rayPlane[2][2][3][4]) {
  auto corner = [&](float x, float y, float z, float out[4]) {
    for (int c = 0; c < 4; c++) out[c] = std::fmaf(M[12 + c], 1.0f, std::fmaf(M[8 + c], z, std::fmaf(M[4 + c], y, M[c] * x)));
  };
  for (int tri = 0; tri < 2; tri++) {
    const float sg = tri ? 1.0f : -1.0f;
    for (int k = 0; k < 2; k++) {
      const float z = k ? 1.0f : -1.0f;
      float p0[4], p1[4], p2[4];
      corner(sg, sg, z, p0); corner(-sg, sg, z, p1); corner(sg, -sg, z, p2);
      for (int c = 0; c < 4; c++) {
        rayPlane[tri][k][0][c] = p0[c];
        rayPlane[tri][k][1][c] = p1[c] - p0[c];
        rayPlane[tri][k][2][c] = p2[c] - p0[c];
      }
    }
  }
}
}  // namespace
void ray_planes(SceneBlock *h) { ray_planes_of(h->cam.invProjView, h->rayPlane); }

// What an evaluation reads of an object (SceneBlock::evalRec), incl. the bound of the table walk's pass-over test, from h->objs.
void scene_eval_records(SceneBlock *h) {
  for (int i = 0; i < h->numObjects; i++) {
    const RmObject &o = h->objs[i];
    EvalRecord &e = h->evalRec[i];
    for (int c = 0; c < 4; c++)
      for (int r = 0; r < 3; r++) e.m[c * 3 + r] = o.invModel[c * 4 + r];
    e.scaleFactor = o.scaleFactor;
    e.type = o.type;
    // the skip test's bound (rm_device.hip.h, sdScene<…, kSkip>): radius of the unit shape's bounding ball, with a margin
    static const float kBound[] = {0.8662f, 0.7073f, 0.7073f, 0.5001f, 0.5001f, 0.6252f, 0.6002f, 0.5001f, 0.7073f};  // cube … rectangle
    const float sf = o.scaleFactor;
    const bool ok = std::isfinite(sf) && sf > 1e-6f && sf < 1e6f;
    e.invScale = ok ? 1.0f / sf : 0.0f;
    // the primitives only: a fractal's evaluation also writes the orbit trap that sdScene returns — the trap of the LAST
    // evaluated fractal in table order, nearest or not — so passing over one would change it
    e.boundR = (ok && o.type >= RM_CUBE && o.type <= RM_RECTANGLE) ? kBound[o.type] : INFINITY;
  }
}

// SceneBlock::bulbPlain: the single-Mandelbulb class whose evaluations can skip the object transform, the ·scaleFactor and
// the Julia select (rm_device.hip.h, sdSceneImpl, has the argument).  Decided on the bits: the three rows of invModel that
// sdScene reads hold exactly 1 on the diagonal and a zero of either sign everywhere else (the scenefile loader writes −0 in
// some of them); scaleFactor is exactly 1; power is 8; both Julia seed components are zero, so frag:782's length is 0.
int bulb_plain(const RmObject *objs, int numObjects, const RmGlobals *g) {
  if (numObjects != 1 || objs[0].type != RM_MANDELBULB) return 0;
  auto bits = [](float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; };
  for (int c = 0; c < 4; c++)
    for (int r = 0; r < 3; r++) {
      const uint32_t u = bits(objs[0].invModel[c * 4 + r]);
      if (c == r ? (u != 0x3f800000u) : ((u & 0x7fffffffu) != 0u)) return 0;
    }
  if (bits(objs[0].scaleFactor) != 0x3f800000u || !(g->power == 8.0f)) return 0;
  return (g->juliaSeed[0] == 0.0f && g->juliaSeed[1] == 0.0f) ? 1 : 0;
}

// SceneBlock::lightPrep from the block's light table and objs[0]: what the bulb kernels' shadow pool read per light instead of
// computing it per ray.  The device's own operations in the device's order, so the same bits: normalize(−dir) is
// scale(v, rcp_(len(v))) with dot = fma(z, z, fma(y, y, x·x)), sqrt_ the correctly rounded square root (sqrtf) and rcp_ the
// correctly rounded reciprocal (1.0f / x; both for every input, denormals, zeros and non-finite values included); pd and a are
// bulbCullEnd's products.  -ffp-contract=off: nothing is fused but the fmaf calls.
void scene_light_prep(SceneBlock *h) {
  const float *M = h->objs[0].invModel;
  for (int i = 0; i < RM_MAX_LIGHTS; i++) {
    LightPrep &q = h->lightPrep[i];
    q = LightPrep{};
    if (i >= h->numLights || h->lights[i].type != RM_LIGHT_DIRECTIONAL) continue;
    const float x = -h->lights[i].dir[0], y = -h->lights[i].dir[1], z = -h->lights[i].dir[2];
    const float inv = 1.0f / std::sqrt(std::fmaf(z, z, std::fmaf(y, y, x * x)));
    const float lx = x * inv, ly = y * inv, lz = z * inv;
    q.L[0] = lx; q.L[1] = ly; q.L[2] = lz;
    if (h->numObjects < 1) continue;
    for (int r = 0; r < 3; r++) q.pd[r] = std::fmaf(M[8 + r], lz, std::fmaf(M[4 + r], ly, M[r] * lx));
    q.a = std::fmaf(q.pd[2], q.pd[2], std::fmaf(q.pd[1], q.pd[1], q.pd[0] * q.pd[0]));
  }
}

// The fill step of a launch: everything of the SceneBlocks of frames 0 … n−1 of one scene that the caller's tables decide (the
// launch fields are upload_frames').  Block 0 from the tables; every other frame a copy of it with its own camera and globals
// (globals[numGlobals == 1 ? 0 : f]) and what they decide: the ray planes, the plain-bulb flag and, where the globals differ per
// frame and the table holds a Mandelbulb (the only type whose cull bounds read them), the cull bounds.
void fill_frames(SceneBlock *h, int n, const RmCamera *cams, const RmGlobals *globals, int numGlobals, const RmObject *objs,
                 int numObjects, const RmLight *lights, int numLights, const RmSettings *s, const RmResources &res) {
  h->cam = cams[0]; h->g = globals[0]; h->s = *s;
  h->numObjects = numObjects; h->numLights = numLights;
  for (int i = 0; i < numObjects; i++) h->objs[i] = objs[i];
  scene_eval_records(h);
  for (int i = 0; i < numLights; i++) h->lights[i] = lights[i];
  scene_light_prep(h);  // reads the two tables only: the copies below take it over
  h->numTextures = res.numTextures;
  for (int i = 0; i < res.numTextures; i++) h->tex[i] = res.textures[i];
  h->noise = res.noise;
  for (int f = 0; f < 6; f++) h->skybox[f] = res.skybox[f];
  h->ltc1 = res.ltc1; h->ltc2 = res.ltc2;
  scene_cull_ball(h);
  ray_planes(h);
  h->bulbPlain = bulb_plain(objs, numObjects, &globals[0]);
  bool bulbInTable = false;
  for (int i = 0; i < numObjects; i++) bulbInTable = bulbInTable || objs[i].type == RM_MANDELBULB;
  for (int f = 1; f < n; f++) {
    SceneBlock *b = h + f;
    *b = *h;
    b->cam = cams[f];
    b->g = globals[numGlobals == 1 ? 0 : f];
    if (bulbInTable && numGlobals > 1) scene_cull_ball(b);
    ray_planes(b);
    b->bulbPlain = bulb_plain(objs, numObjects, &b->g);
  }
}

// The fill step of rm_render_animated: fill_frames where every block may have an object table and a light table of its own
// (objs + b·numObjects when numObjectTables > 1, table 0 otherwise; the lights likewise).  Nothing is taken over from block 0 but
// what a call shares (settings, resources, the counts): the table copies, the evaluation records, the per-light constants, the cull ball and box with
// cullLip, cullOneOk and objBall, the ray planes and the plain-bulb flag all come from the block's own tables, camera and globals.
// With both counts 1 every block holds what fill_frames gives it.  restage (or null): bit b set where block b's object table
// differs, byte for byte, from block b − 1's (never for b = 0) — what render_anim_kernel stages anew.
void fill_frames_animated(SceneBlock *h, int n, const RmCamera *cams, const RmGlobals *globals, int numGlobals, const RmObject *objs,
                          int numObjects, int numObjectTables, const RmLight *lights, int numLights, int numLightTables,
                          const RmSettings *s, const RmResources &res, RestageBits *restage) {
  const size_t tableBytes = sizeof(RmObject) * (size_t)numObjects;
  if (restage) std::memset(restage, 0, sizeof(*restage));
  for (int f = 0; f < n; f++) {
    SceneBlock *b = h + f;
    const RmObject *o = objs + (numObjectTables == 1 ? 0 : (size_t)f * (size_t)numObjects);
    const RmLight *l = lights + (numLightTables == 1 ? 0 : (size_t)f * (size_t)numLights);
    const RmGlobals *g = &globals[numGlobals == 1 ? 0 : f];
    if (f == 0) {
      fill_frames(b, 1, cams, g, 1, o, numObjects, l, numLights, s, res);
      continue;
    }
    const RmObject *prev = objs + (numObjectTables == 1 ? 0 : (size_t)(f - 1) * (size_t)numObjects);
    const bool sameObjs = o == prev || tableBytes == 0 || std::memcmp(o, prev, tableBytes) == 0;
    *b = *(b - 1);  // the shared part, and the previous block's tables where this block's are the same
    b->cam = cams[f];
    b->g = *g;
    if (!sameObjs) {
      for (int i = 0; i < numObjects; i++) b->objs[i] = o[i];
      scene_eval_records(b);
      if (restage) restage->set(f);
    }
    for (int i = 0; i < numLights; i++) b->lights[i] = l[i];
    if (!sameObjs || numLightTables > 1) scene_light_prep(b);  // the block's own tables
    // the cull bounds read the table and, for a Mandelbulb, the globals: recomputed whenever either may differ from the previous block's
    if (!sameObjs || numGlobals > 1) scene_cull_ball(b);
    ray_planes(b);
    b->bulbPlain = bulb_plain(o, numObjects, g);
  }
}

// Whether the wavefront pipeline is expected to beat the one-lane-per-pixel kernel on this scene (measured).
// Measured (profiles/r03_b_wavefront.md): with reflection bounces the regrouping wins from 4K frames up (8K Menger frame
// with two bounces 39.0 -> 24.4 ms, the same scene at 4K 12.0 -> 9.2 ms, reflections_complex.json at 4K with two bounces
// 25.4 -> 20.2 ms, with one 16.8 -> 16.4 ms); at 1080p its dozen launches of persistent waves cost more than the idle lanes
// they remove (4.5 -> 5.2 ms, 5.4 -> 7.2 ms), and without secondary rays the one-lane-per-pixel kernel keeps 89-95 % of its
// lanes busy by itself (directional_light_2.json: 1.3 ms against 3.5 ms).
// Round 3, after the table walk learnt to pass over far objects (sdScene<…, kSkip>) and to follow a single object (march()'s
// fast path, all-primitive tables): for all-primitive tables the one-lane-per-pixel kernel is ahead at every bounce count
// (reflections_complex.json 4K: 7.5 ms against 12.4 with one bounce, 12.4 against 15.7 with two) — in the wavefront kernels a
// wave's lanes are unrelated rays, and both tests need the whole wave to agree.  Mixed tables (primitives and a fractal): the
// pass-over test applies, the fast path does not; two or more bounces as measured before the fast path.
bool skip_applies(const RmObject *objs, int numObjects) {
  bool prim = false;
  for (int i = 0; i < numObjects; i++) prim = prim || (objs[i].type >= RM_CUBE && objs[i].type <= RM_RECTANGLE);
  return prim && numObjects >= 2;
}
bool all_primitives(const RmObject *objs, int numObjects) {
  bool prim = numObjects > 0;
  for (int i = 0; i < numObjects; i++) prim = prim && objs[i].type >= RM_CUBE && objs[i].type <= RM_RECTANGLE;
  return prim;
}
// Size threshold: whole frames and row ranges from 2^22 pixels (one launch after the other on a stream: 4K and up).  Row-TILE
// shards (rm_render_tiles with numShards > 1) come from multi-GPU hosts, which keep several frames in flight per GPU
// (dist.FramePipeline, scripts/mgpu_host.cpp): the pipeline's dozen launches per frame then overlap those of its neighbours and
// it pays from 2^21 pixels — measured on shards of the C5 scene with three frames in flight (profiles/r04_j_c5_shards.md):
// 4.18 M pixels (1/8 of the 8K frame) 3.41 against 4.34 ms per frame, 2.09 M 2.47 against 2.73, 1.04 M 1.70 against 1.44.
bool wavefront_pays(const RmObject *objs, int numObjects, int bounces, size_t pixels, bool tileShard) {
  if (all_primitives(objs, numObjects)) return false;
  return bounces >= (skip_applies(objs, numObjects) ? 2 : 1) && pixels >= (size_t(1) << (tileShard ? 21 : 22));
}

FrameClass classify_frame(const RmObject *objs, int numObjects, const RmLight *lights, int numLights, const RmGlobals *g,
                          const RmSettings *s, int count) {
  FrameClass fc{};
  fc.bulb = numObjects == 1 && objs[0].type == RM_MANDELBULB;
  fc.twoD = g->isTwoD != 0;
  auto nonzero3 = [](const float *v) { return v[0] != 0.0f || v[1] != 0.0f || v[2] != 0.0f; };
  fc.envFeatures = (s->features & (RM_FEAT_TERRAIN | RM_FEAT_CLOUD | RM_FEAT_SKY_BACKGROUND | RM_FEAT_NIGHTSKY_BACKGROUND | RM_FEAT_SEA)) != 0;
  // anything that reads a sampler or takes the area-light branches: object textures, sky box, emissive rectangles, area lights
  fc.textured = s->enableSkyBox != 0;
  for (int i = 0; i < numObjects; i++) fc.textured = fc.textured || objs[i].texLoc != -1 || objs[i].isEmissive;
  for (int i = 0; i < numLights; i++) fc.textured = fc.textured || lights[i].type == RM_LIGHT_AREA;
  // The wavefront pipeline (rm_wavefront.hip.h) covers the table-walk classes whose evaluations cost the same on every
  // lane: no Mandelbulb / 2-D Mandelbrot in the table, no samplers or procedural layers, no refraction.
  fc.wfOk = !fc.bulb && !count && !fc.envFeatures && !fc.textured && !fc.twoD && s->maxSteps >= 1 && s->numReflection <= kWfMaxBounces;
  bool anyReflective = false, anyTransparent = false;
  for (int i = 0; i < numObjects; i++) {
    if (objs[i].type == RM_MANDELBULB || objs[i].type == RM_MANDELBROT) fc.wfOk = false;
    if (s->enableRefraction && nonzero3(objs[i].cTransparent)) fc.wfOk = false;
    anyReflective = anyReflective || nonzero3(objs[i].cReflective);
    anyTransparent = anyTransparent || nonzero3(objs[i].cTransparent);
  }
  fc.wfBounces = (s->enableReflection && anyReflective) ? s->numReflection : 0;
  // whether main's secondary rays (frag:2491-2570) can fire for any pixel of this frame: a reflective object with reflection on and
  // at least one bounce, or a transparent one with refraction on — otherwise the plain instantiations compile them out (SEC = false)
  fc.secondary = (s->enableReflection && anyReflective && s->numReflection > 0) || (s->enableRefraction && anyTransparent);
  fc.wfSkip = skip_applies(objs, numObjects);
  return fc;
}

// The BULB argument of a frame's production kernels (dispatch_class): the bulb class only without layers and samplers, its plain
// form where the launcher found it.
int bulb_class(const FrameClass &fc, bool plainBulb) {
  return (fc.bulb && !fc.envFeatures && !fc.textured) ? (plainBulb ? kBulbPlain : kBulbGeneral) : 0;
}
// The same for the calls that march a bare object table (no layers, no samplers): the bulb class of a lone Mandelbulb.
int table_bulb_class(const RmObject *objs, int numObjects, bool plainBulb) {
  return (numObjects == 1 && objs[0].type == RM_MANDELBULB) ? (plainBulb ? kBulbPlain : kBulbGeneral) : 0;
}

// The picture this launch renders: everything that decides a pixel (FNV-1a over the caller's tables and the row map) — what the
// tile-order feedback and the tuners key their measurements by.
unsigned long long picture_key(const RmCamera *cam, const RmObject *objs, int numObjects, const RmLight *lights, int numLights,
                               const RmGlobals *g, const RmSettings *s, const RowMap &map) {
  unsigned long long key = 1469598103934665603ull;
  auto mix = [&](const void *p, size_t nb) {
    const unsigned char *b8 = static_cast<const unsigned char *>(p);
    for (size_t k = 0; k < nb; k++) key = (key ^ b8[k]) * 1099511628211ull;
  };
  mix(cam, sizeof(*cam)); mix(g, sizeof(*g)); mix(s, sizeof(*s)); mix(&map, sizeof(map));
  mix(objs, sizeof(RmObject) * (size_t)numObjects); mix(lights, sizeof(RmLight) * (size_t)numLights);
  return key;
}

// the row map of the rows [rowBegin, rowEnd) of an H-row frame (rm_render*, rm_render_counted*)
int row_range(int H, int rowBegin, int rowEnd, RowMap *map, int *nRows) {
  if (rowBegin < 0 || rowEnd > H || rowBegin > rowEnd) { set_error("rows out of range"); return RM_ERR_INVALID_ARGUMENT; }
  *nRows = rowEnd - rowBegin;
  *map = RowMap{rowBegin, *nRows > 0 ? *nRows : 1, 0, 1, 0};
  return RM_OK;
}

}  // namespace rm

using namespace rm;

extern "C" {

int rm_debug_ray_planes(const RmCamera *cam, float *out48) {
  if (!cam || !out48) { set_error("null pointer"); return RM_ERR_INVALID_ARGUMENT; }
  static SceneBlock blk;  // host-only scratch; the planes are a pure function of the camera
  static std::mutex mu;
  std::lock_guard<std::mutex> lock(mu);
  blk.cam = *cam;
  ray_planes(&blk);
  std::memcpy(out48, blk.rayPlane, sizeof(blk.rayPlane));
  return RM_OK;
}
int rm_debug_cull_bounds(const RmObject *objs, int numObjects, const RmGlobals *g, float *out14) {
  if ((!objs && numObjects > 0) || !g || !out14) { set_error("null pointer"); return RM_ERR_INVALID_ARGUMENT; }
  if (numObjects < 0 || numObjects > RM_MAX_OBJECTS) { set_error("numObjects out of range"); return RM_ERR_INVALID_ARGUMENT; }
  static SceneBlock blk;  // host-only scratch; the bounds are a pure function of the object table and the globals
  static std::mutex mu;
  std::lock_guard<std::mutex> lock(mu);
  blk.g = *g;
  blk.numObjects = numObjects;
  for (int i = 0; i < numObjects; i++) blk.objs[i] = objs[i];
  scene_cull_ball(&blk);
  out14[0] = (float)blk.cullOk;
  for (int k = 0; k < 3; k++) { out14[1 + k] = blk.cullC[k]; out14[7 + k] = blk.cullLo[k]; out14[10 + k] = blk.cullHi[k]; }
  out14[4] = blk.cullR2; out14[5] = blk.cullR2Soft; out14[6] = (float)blk.cullBoxOk;
  out14[13] = blk.cullLip;
  return RM_OK;
}
int rm_debug_light_prep(const RmObject *objs, int numObjects, const RmLight *lights, int numLights, float *out) {
  if ((!objs && numObjects > 0) || (!lights && numLights > 0) || !out) { set_error("null pointer"); return RM_ERR_INVALID_ARGUMENT; }
  if (numObjects < 0 || numObjects > RM_MAX_OBJECTS) { set_error("numObjects out of range"); return RM_ERR_INVALID_ARGUMENT; }
  if (numLights < 0 || numLights > RM_MAX_LIGHTS) { set_error("numLights out of range"); return RM_ERR_INVALID_ARGUMENT; }
  static SceneBlock blk;  // host-only scratch; the constants are a pure function of the two tables
  static std::mutex mu;
  std::lock_guard<std::mutex> lock(mu);
  blk.numObjects = numObjects;
  blk.numLights = numLights;
  if (numObjects > 0) blk.objs[0] = objs[0];
  for (int i = 0; i < numLights; i++) blk.lights[i] = lights[i];
  scene_light_prep(&blk);
  for (int i = 0; i < numLights; i++) std::memcpy(out + 8 * i, &blk.lightPrep[i], sizeof(LightPrep));
  return RM_OK;
}
int rm_debug_bulb_plain(const RmObject *objs, int numObjects, const RmGlobals *g) {
  if ((!objs && numObjects > 0) || !g) { set_error("null pointer"); return -1; }
  if (numObjects < 0 || numObjects > RM_MAX_OBJECTS) { set_error("numObjects out of range"); return -1; }
  return bulb_plain(objs, numObjects, g);
}

// rm_camera_rays (the header has the definition): the host restatement of ray_planes + the device's primaryRay (rm_device.hip.h:
// quadCoord, the two fused interpolations, the divisions by w, normalize = v · (1 / len)) with the same operations in the same
// order — binary32 fmaf, correctly rounded divide and square root, nothing contracted (-ffp-contract=off) — so the same bits.
int rm_camera_rays(const RmCamera *cam, int W, int H, const int32_t *xy, int n, RmRay *out) {
  if (!cam || !out) { set_error("null camera or output"); return RM_ERR_INVALID_ARGUMENT; }
  if (W <= 0 || H <= 0 || n < 0) { set_error("bad frame size or count"); return RM_ERR_INVALID_ARGUMENT; }
  if (!xy && (long long)n != (long long)W * H) { set_error("without a pixel list n must be W·H"); return RM_ERR_INVALID_ARGUMENT; }
  if (xy)
    for (int i = 0; i < n; i++)
      if (xy[2 * i] < 0 || xy[2 * i] >= W || xy[2 * i + 1] < 0 || xy[2 * i + 1] >= H) {
        set_error("pixel " + std::to_string(i) + " lies outside the frame");
        return RM_ERR_INVALID_ARGUMENT;
      }
  float P[2][2][3][4];
  ray_planes_of(cam->invProjView, P);
  for (int i = 0; i < n; i++) {
    const int px = xy ? xy[2 * i] : i % W, py = xy ? xy[2 * i + 1] : i / W;
    const float tx = ((float)px + 0.5f) / (float)W, ty = ((float)py + 0.5f) / (float)H;
    const int upper = (tx + ty) > 1.0f;
    const float I = upper ? 1.0f - tx : tx, J = upper ? 1.0f - ty : ty;
    float nc[4], fc[4];
    for (int k = 0; k < 4; k++) {
      nc[k] = std::fmaf(J, P[upper][0][2][k], std::fmaf(I, P[upper][0][1][k], P[upper][0][0][k]));
      fc[k] = std::fmaf(J, P[upper][1][2][k], std::fmaf(I, P[upper][1][1][k], P[upper][1][0][k]));
    }
    RmRay &r = out[i];
    float d[3];
    for (int k = 0; k < 3; k++) {
      r.origin[k] = nc[k] / nc[3];
      d[k] = fc[k] / fc[3] - r.origin[k];
    }
    const float inv = 1.0f / std::sqrt(std::fmaf(d[2], d[2], std::fmaf(d[1], d[1], d[0] * d[0])));
    for (int k = 0; k < 3; k++) r.dir[k] = d[k] * inv;
    r.tMax = cam->initialFar;
    r.reserved = 0;
  }
  return RM_OK;
}

}  // extern "C"
