// rm_light_probes_depth and rm_light_grid_irradiance_visible on the CPU, serially, through the very functions the kernels call per
// lane (raymarcher_amd/csrc/rm_light_depth.h: probe_depth; rm_light_grid.h: grid_light_visible).  A stand-alone program, so that
// it can run under the host sanitizers.
//   rm_light_depth_cpu bake <query file> <result file>
//     query: int32 numProbes, numDirs, numSets; numProbes·4 floats (positions); numSets·numDirs rows of 64 bytes (RmProbeDir);
//     numSets·numDirs·64 floats (weights); numProbes·numDirs floats (the t of every ray).  result: numProbes records of 512 bytes.
//   rm_light_depth_cpu look <query file> <result file>
//     query: int32 dims[3], numPoints, flags; float origin[3], step[3], normalBias; the grid's records of 160 bytes (RmLightProbe),
//     then its records of 512 bytes (RmProbeDepth); numPoints·4 floats (points); numPoints·4 floats (normals).
//     result: numPoints records of 32 bytes (RmGridLight).
// The loader counts what it is asked for: neither a coefficient nor a depth word of an invalid probe must ever be read.
// Build with -ffp-contract=off: every operation of the definitions is one binary32 operation.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../raymarcher_amd/csrc/rm_light_depth.h"
#include "../../raymarcher_amd/csrc/rm_light_grid.h"

namespace lg = rm::lg;
namespace lp = rm::lp;
namespace ld = rm::ld;

struct Probe { float sh[lg::kBasis][4]; int32_t hits; int32_t reserved[3]; };  // RmLightProbe

struct Records {
  const std::vector<Probe> &probes;
  const std::vector<ld::Depth> &depths;
  long *badReads;
  int hits(size_t i) const { return probes.at(i).hits; }
  void sh(size_t i, int j, float out[4]) const {
    const Probe &r = probes.at(i);
    if (r.hits < 0) ++*badReads;
    std::memcpy(out, r.sh[j], sizeof(float) * 4);
  }
  void depth(size_t i, int texel, float out[2]) const {
    if (probes.at(i).hits < 0 || texel < 0 || texel >= ld::kTexels) ++*badReads;
    std::memcpy(out, depths.at(i).moments[texel], sizeof(float) * 2);
  }
};

template <class T>
static bool get(FILE *f, T *p, size_t n) { return n == 0 || std::fread(p, sizeof(T), n, f) == n; }

template <class T>
static int put(const char *path, const std::vector<T> &out) {
  FILE *of = std::fopen(path, "wb");
  if (!of) { std::perror(path); return 2; }
  const bool ok = out.empty() || std::fwrite(out.data(), sizeof(T), out.size(), of) == out.size();
  if (std::fclose(of) != 0 || !ok) { std::fprintf(stderr, "short write\n"); return 2; }
  return 0;
}

static int bake(FILE *in, const char *result) {
  int32_t head[3];
  if (!get(in, head, 3)) { std::fprintf(stderr, "short header\n"); return 2; }
  const int numProbes = head[0], numDirs = head[1], numSets = head[2];
  if (numProbes < 0 || numProbes > (1 << 20) || numDirs < 1 || numDirs > lp::kMaxDirs || (numDirs & (numDirs - 1)) != 0 || numSets < 1 ||
      numSets * numDirs > 4096) {
    std::fprintf(stderr, "bad dimensions\n");
    return 2;
  }
  const size_t rows = (size_t)numSets * (size_t)numDirs;
  std::vector<float> positions((size_t)numProbes * 4), weights(rows * ld::kTexels), t((size_t)numProbes * (size_t)numDirs);
  std::vector<lp::Row> table(rows);
  if (!get(in, positions.data(), positions.size()) || !get(in, table.data(), table.size()) || !get(in, weights.data(), weights.size()) ||
      !get(in, t.data(), t.size())) {
    std::fprintf(stderr, "short query\n");
    return 2;
  }
  std::vector<ld::Depth> out((size_t)numProbes);
  for (size_t i = 0; i < (size_t)numProbes; i++) {
    const size_t set = (i % (size_t)numSets) * (size_t)numDirs;
    out[i] = ld::probe_depth(&positions[4 * i], t.data() + i * (size_t)numDirs, table.data() + set, weights.data() + set * ld::kTexels, numDirs);
  }
  return put(result, out);
}

static int look(FILE *in, const char *result) {
  int32_t head[5];
  lg::Grid G;
  float normalBias;
  if (!get(in, head, 5) || !get(in, G.origin, 3) || !get(in, G.step, 3) || !get(in, &normalBias, 1)) { std::fprintf(stderr, "short header\n"); return 2; }
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
  std::vector<ld::Depth> depths((size_t)count);
  std::vector<float> points((size_t)numPoints * 4), normals((size_t)numPoints * 4);
  if (!get(in, probes.data(), probes.size()) || !get(in, depths.data(), depths.size()) || !get(in, points.data(), points.size()) ||
      !get(in, normals.data(), normals.size())) {
    std::fprintf(stderr, "short query\n");
    return 2;
  }
  long badReads = 0;
  const Records load{probes, depths, &badReads};
  std::vector<lg::GridLight> out((size_t)numPoints);
  for (size_t i = 0; i < (size_t)numPoints; i++) out[i] = lg::grid_light_visible(G, &points[4 * i], &normals[4 * i], flags, normalBias, load);
  if (badReads != 0) { std::fprintf(stderr, "%ld words of invalid probes were read\n", badReads); return 3; }
  return put(result, out);
}

int main(int argc, char **argv) {
  static_assert(sizeof(Probe) == 160 && sizeof(lg::GridLight) == 32 && sizeof(ld::Depth) == 512 && sizeof(lp::Row) == 64, "the records' sizes");
  const bool isBake = argc == 4 && std::strcmp(argv[1], "bake") == 0, isLook = argc == 4 && std::strcmp(argv[1], "look") == 0;
  if (!isBake && !isLook) { std::fprintf(stderr, "usage: %s bake|look query result\n", argv[0]); return 2; }
  FILE *in = std::fopen(argv[2], "rb");
  if (!in) { std::perror(argv[2]); return 2; }
  const int st = isBake ? bake(in, argv[3]) : look(in, argv[3]);
  std::fclose(in);
  return st;
}
