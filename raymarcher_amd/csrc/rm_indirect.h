// rm_indirect.h — the arithmetic of rm_shade_rays_indirect behind the hit (include/raymarcher_amd.h has the definition): the clamp of
// the grid's irradiance, the products with the hit's diffuse colour and the strength, the palette of the two fractals and the one
// addition to the shaded colour.  term() does all of it for one ray: a lane's work in rm_indirect.hip.h behind the grid lookup
// (rm_light_grid.h) and the whole of the host program's (tests/light_bounce_spec).  The palette colour c is an argument — the
// kernel has it from bulbTrapColor or the sponge's cosine palette, which are device code — so nothing here needs a device built-in.
//   Plain C++, so the kernel and a host program run the very same code.  Every operation is one binary32 operation as written:
// compile with -ffp-contract=off.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RM_IND_FN __host__ __device__ inline
#else
#define RM_IND_FN inline
#endif

namespace rm {
namespace ind {

constexpr float kInvPi = (float)0.31830988618379067;  // RM_INV_PI: 1/π in binary64, rounded once
enum Palette : int { kPlain = 0, kBulb = 1, kSponge = 2 };

// k = strength · RM_INV_PI: one multiplication, on the host, once per call.
RM_IND_FN float scale_of(float strength) { return strength * kInvPi; }

// ec = e > 0 ? e : +0: SH ringing, −0 and NaN become +0.
RM_IND_FN float clamp_e(float e) { return e > 0.0f ? e : 0.0f; }

// x[ch] = (dif[ch] · ec[ch]) · k.
RM_IND_FN void diffuse_term(const float dif[3], const float e[3], float k, float x[3]) {
  for (int ch = 0; ch < 3; ch++) x[ch] = (dif[ch] * clamp_e(e[ch])) * k;
}

// The palette multiplies the term as render() multiplies Phong: c · (x · 8) on the Mandelbulb, c · x on the sponge, x elsewhere
// (c is not read).
RM_IND_FN void apply_palette(int palette, const float c[3], const float x[3], float ind[3]) {
  for (int ch = 0; ch < 3; ch++) {
    if (palette == kBulb) ind[ch] = c[ch] * (x[ch] * 8.0f);
    else if (palette == kSponge) ind[ch] = c[ch] * x[ch];
    else ind[ch] = x[ch];
  }
}

// out.rgb = colour.rgb + ind, one addition per channel; alpha is colour's.  probes <= 0 (no corner took part, an invalid point):
// colour's words unchanged, no addition performed.
RM_IND_FN void term(const float colour[4], int probes, const float e[3], const float dif[3], float k, int palette, const float c[3],
                    float out[4]) {
  out[0] = colour[0], out[1] = colour[1], out[2] = colour[2], out[3] = colour[3];
  if (probes <= 0) return;
  float x[3], ind[3];
  diffuse_term(dif, e, k, x);
  apply_palette(palette, c, x, ind);
  for (int ch = 0; ch < 3; ch++) out[ch] = colour[ch] + ind[ch];
}

}  // namespace ind
}  // namespace rm
