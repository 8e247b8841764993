// The term of rm_shade_rays_indirect on the CPU, serially, through the very functions the kernels call per lane behind the hit
// (raymarcher_amd/csrc/rm_light_grid.h: grid_light, grid_light_visible; rm_indirect.h: term).  A stand-alone program, so that it can
// run under the host sanitizers.
//   rm_light_bounce_cpu <query file> <result file>
//     query: int32 dims[3], numRays, flags, hasDepth; float origin[3], step[3], normalBias, k; the grid's records of 160 bytes
//     (RmLightProbe); with hasDepth its records of 512 bytes (RmProbeDepth); then numRays·4 floats each of hit points, normals,
//     shaded colours, diffuse colours and palette colours (w not read but of the colours); numRays int32 of the palette kind
//     (0 plain, 1 Mandelbulb, 2 sponge); numRays int32 of "the ray has a term" (a valid ray that hit an object that is not emissive).
//     result: numRays·4 floats.
// The loader counts what it is asked for: neither a coefficient nor a depth word of an invalid probe must ever be read, and the grid
// is not looked up for a ray without a term.
// Build with -ffp-contract=off: every operation of the definition is one binary32 operation.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../raymarcher_amd/csrc/rm_indirect.h"
#include "../../raymarcher_amd/csrc/rm_light_grid.h"

namespace lg = rm::lg;
namespace ind = rm::ind;

struct Probe { float sh[lg::kBasis][4]; int32_t hits; int32_t reserved[3]; };  // RmLightProbe
struct Depth { float moments[64][2]; };                                         // RmProbeDepth

struct Records {
  const std::vector<Probe> &probes;
  const std::vector<Depth> &depths;
  long *badReads;
  int hits(size_t i) const { return probes.at(i).hits; }
  void sh(size_t i, int j, float out[4]) const {
    const Probe &r = probes.at(i);
    if (r.hits < 0) ++*badReads;
    std::memcpy(out, r.sh[j], sizeof(float) * 4);
  }
  void depth(size_t i, int texel, float out[2]) const {
    if (probes.at(i).hits < 0 || texel < 0 || texel >= 64) ++*badReads;
    std::memcpy(out, depths.at(i).moments[texel], sizeof(float) * 2);
  }
};

template <class T>
static bool get(FILE *f, T *p, size_t n) { return n == 0 || std::fread(p, sizeof(T), n, f) == n; }

int main(int argc, char **argv) {
  static_assert(sizeof(Probe) == 160 && sizeof(Depth) == 512 && sizeof(lg::GridLight) == 32, "the records' sizes");
  if (argc != 3) { std::fprintf(stderr, "usage: %s query result\n", argv[0]); return 2; }
  FILE *in = std::fopen(argv[1], "rb");
  if (!in) { std::perror(argv[1]); return 2; }
  int32_t head[6];
  lg::Grid G;
  float tail[2];
  if (!get(in, head, 6) || !get(in, G.origin, 3) || !get(in, G.step, 3) || !get(in, tail, 2)) { std::fprintf(stderr, "short header\n"); return 2; }
  const int numRays = head[3];
  const unsigned flags = (unsigned)head[4];
  const bool hasDepth = head[5] != 0;
  const float normalBias = tail[0], k = tail[1];
  long long count = 1;
  for (int a = 0; a < 3; a++) {
    G.dims[a] = head[a];
    if (G.dims[a] < 2 || G.dims[a] > lg::kMaxDim) { std::fprintf(stderr, "bad dimensions\n"); return 2; }
    count *= G.dims[a];
  }
  if (count > (1 << 20) || numRays < 0 || numRays > (1 << 20) || (flags & ~lg::kFacing)) { std::fprintf(stderr, "bad query\n"); return 2; }
  const size_t n = (size_t)numRays;
  std::vector<Probe> probes((size_t)count);
  std::vector<Depth> depths(hasDepth ? (size_t)count : 0);
  std::vector<float> points(n * 4), normals(n * 4), colour(n * 4), dif(n * 4), pal(n * 4);
  std::vector<int32_t> kind(n), hasTerm(n);
  if (!get(in, probes.data(), probes.size()) || !get(in, depths.data(), depths.size()) || !get(in, points.data(), points.size()) ||
      !get(in, normals.data(), normals.size()) || !get(in, colour.data(), colour.size()) || !get(in, dif.data(), dif.size()) ||
      !get(in, pal.data(), pal.size()) || !get(in, kind.data(), kind.size()) || !get(in, hasTerm.data(), hasTerm.size())) {
    std::fprintf(stderr, "short query\n");
    return 2;
  }
  std::fclose(in);
  long badReads = 0;
  const Records load{probes, depths, &badReads};
  std::vector<float> out(n * 4);
  for (size_t i = 0; i < n; i++) {
    if (!hasTerm[i]) {  // the colour's words, and no lookup
      std::memcpy(&out[4 * i], &colour[4 * i], sizeof(float) * 4);
      continue;
    }
    const lg::GridLight r = hasDepth ? lg::grid_light_visible(G, &points[4 * i], &normals[4 * i], flags, normalBias, load)
                                     : lg::grid_light(G, &points[4 * i], &normals[4 * i], flags, load);
    ind::term(&colour[4 * i], r.probes, r.e, &dif[4 * i], k, kind[i], &pal[4 * i], &out[4 * i]);
  }
  if (badReads != 0) { std::fprintf(stderr, "%ld words of invalid probes were read\n", badReads); return 3; }
  FILE *of = std::fopen(argv[2], "wb");
  if (!of) { std::perror(argv[2]); return 2; }
  const bool ok = out.empty() || std::fwrite(out.data(), sizeof(float), out.size(), of) == out.size();
  if (std::fclose(of) != 0 || !ok) { std::fprintf(stderr, "short write\n"); return 2; }
  return 0;
}
