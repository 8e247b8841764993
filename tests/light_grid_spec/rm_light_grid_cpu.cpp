// rm_light_grid_irradiance on the CPU, serially, through the very function the kernel calls per lane
// (raymarcher_amd/csrc/rm_light_grid.h: grid_light).  A stand-alone program, so that it can run under the host sanitizers.
//   rm_light_grid_cpu <query file> <result file>
// query file: int32 dims[3], numPoints, flags; float origin[3], step[3]; dims[0]·dims[1]·dims[2] records of 160 bytes
// (RmLightProbe); numPoints·4 floats (the points); numPoints·4 floats (the normals).
// result file: numPoints records of 32 bytes (RmGridLight).
// The loader counts what it is asked for: a coefficient of an invalid probe must never be read.
// Build with -ffp-contract=off: every operation of the definition is one binary32 operation.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../raymarcher_amd/csrc/rm_light_grid.h"

namespace lg = rm::lg;

struct Probe { float sh[lg::kBasis][4]; int32_t hits; int32_t reserved[3]; };  // RmLightProbe

struct Records {
  const std::vector<Probe> &probes;
  long *badReads;
  int hits(size_t i) const { return probes.at(i).hits; }
  void sh(size_t i, int j, float out[4]) const {
    const Probe &r = probes.at(i);
    if (r.hits < 0) ++*badReads;
    std::memcpy(out, r.sh[j], sizeof(float) * 4);
  }
};

template <class T>
static bool get(FILE *f, T *p, size_t n) { return n == 0 || std::fread(p, sizeof(T), n, f) == n; }

int main(int argc, char **argv) {
  static_assert(sizeof(Probe) == 160 && sizeof(lg::GridLight) == 32, "records of 160 and 32 bytes");
  if (argc != 3) { std::fprintf(stderr, "usage: %s query result\n", argv[0]); return 2; }
  FILE *in = std::fopen(argv[1], "rb");
  if (!in) { std::perror(argv[1]); return 2; }
  int32_t head[5];
  lg::Grid G;
  if (!get(in, head, 5) || !get(in, G.origin, 3) || !get(in, G.step, 3)) { std::fprintf(stderr, "short header\n"); return 2; }
  const int numPoints = head[3];
  const unsigned flags = (unsigned)head[4];
  long long count = 1;
  for (int a = 0; a < 3; a++) {
    G.dims[a] = head[a];
    if (G.dims[a] < 2 || G.dims[a] > lg::kMaxDim) { std::fprintf(stderr, "bad dimensions\n"); return 2; }
    count *= G.dims[a];
  }
  if (count > (1 << 20) || numPoints < 0 || numPoints > (1 << 20) || (flags & ~lg::kFacing)) { std::fprintf(stderr, "bad query\n"); return 2; }
  std::vector<Probe> probes((size_t)count);
  std::vector<float> points((size_t)numPoints * 4), normals((size_t)numPoints * 4);
  if (!get(in, probes.data(), probes.size()) || !get(in, points.data(), points.size()) || !get(in, normals.data(), normals.size())) {
    std::fprintf(stderr, "short query\n");
    return 2;
  }
  std::fclose(in);
  long badReads = 0;
  const Records load{probes, &badReads};
  std::vector<lg::GridLight> out((size_t)numPoints);
  for (size_t i = 0; i < (size_t)numPoints; i++) out[i] = lg::grid_light(G, &points[4 * i], &normals[4 * i], flags, load);
  if (badReads != 0) { std::fprintf(stderr, "%ld coefficients of invalid probes were read\n", badReads); return 3; }
  FILE *of = std::fopen(argv[2], "wb");
  if (!of) { std::perror(argv[2]); return 2; }
  const bool ok = out.empty() || std::fwrite(out.data(), sizeof(lg::GridLight), out.size(), of) == out.size();
  if (std::fclose(of) != 0 || !ok) { std::fprintf(stderr, "short write\n"); return 2; }
  return 0;
}
