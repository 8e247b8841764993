// rm_field_ambient on the CPU, serially, through the very function the kernel's pieces come from
// (raymarcher_amd/csrc/rm_field_ambient.h: ambient_point, the sequential walk of the tree).  A stand-alone program, so that it can run
// under the host sanitizers.  The block map and the coarse level are built here by a plain loop over the list.
//   rm_field_ambient_cpu <query file> <result file>
// query file: int32 sparse, d0, d1, d2 (n per axis, or m per axis with sparse), numBlocks, hasIds, numPoints, hasNormals, numDirs,
// numSets, maxSteps, mode (0 RM_AMBIENT_SOFT, 1 RM_AMBIENT_HARD); float origin[3], step[3], bias, maxDistance, iso; numBlocks·4 int32
// (the list, sparse only); the values — d0·d1·d2 floats, or numBlocks·729 with sparse —; as many int32 with hasIds; numPoints·4
// floats; as many with hasNormals; numSets·numDirs·4 floats.
// result file: numPoints records of 32 bytes (RmAmbient).
// Build with -ffp-contract=off: every operation of the definition is one binary32 operation.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../raymarcher_amd/csrc/rm_field_ambient.h"

namespace fm = rm::fm;
namespace fs = rm::fs;
namespace fa = rm::fa;
namespace snb = rm::snb;

template <class T>
static bool get(FILE *f, T *p, size_t n) { return n == 0 || std::fread(p, sizeof(T), n, f) == n; }

struct Query {
  std::vector<float> points, normals, table;
  int numDirs, numSets, maxSteps, mode;
  float bias, maxDistance, iso;
};

template <class Field>
static void run(const Field &F, const fs::Coarse &C, const fm::Frame &L, const Query &q, std::vector<unsigned char> &out) {
  static_assert(sizeof(fa::Ambient) == 32, "records of 32 bytes");
  const size_t np = q.points.size() / 4;
  out.resize(np * 32);
  for (size_t i = 0; i < np; i++) {
    const float *p = &q.points[4 * i];
    const float *given = q.normals.empty() ? nullptr : &q.normals[4 * i];
    const float *dirs = &q.table[4 * (i % (size_t)q.numSets) * (size_t)q.numDirs];
    const fa::Ambient r = q.mode == 0 ? fa::ambient_point<true>(F, C, L, p, given, dirs, q.numDirs, q.bias, q.maxDistance, q.iso, q.maxSteps)
                                      : fa::ambient_point<false>(F, C, L, p, given, dirs, q.numDirs, q.bias, q.maxDistance, q.iso, q.maxSteps);
    std::memcpy(&out[32 * i], &r, 32);
  }
}

int main(int argc, char **argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s query result\n", argv[0]); return 2; }
  FILE *in = std::fopen(argv[1], "rb");
  if (!in) { std::perror(argv[1]); return 2; }
  int32_t head[12];
  float origin[3], step[3], scalars[3];
  if (!get(in, head, 12) || !get(in, origin, 3) || !get(in, step, 3) || !get(in, scalars, 3)) { std::fprintf(stderr, "short header\n"); return 2; }
  const bool sparse = head[0] != 0;
  const int d0 = head[1], d1 = head[2], d2 = head[3], numBlocks = head[4], numPoints = head[6];
  Query q;
  q.numDirs = head[8], q.numSets = head[9], q.maxSteps = head[10], q.mode = head[11];
  q.bias = scalars[0], q.maxDistance = scalars[1], q.iso = scalars[2];
  const int lo = sparse ? 1 : 2, hi = sparse ? 512 : 4096;
  if (d0 < lo || d1 < lo || d2 < lo || d0 > hi || d1 > hi || d2 > hi || numBlocks < 0 || numBlocks > (1 << 22) || numPoints < 0 || q.maxSteps < 0 ||
      q.maxSteps > 65536 || q.mode < 0 || q.mode > 1 || q.numDirs < 1 || q.numDirs > fa::kMaxDirs || (q.numDirs & (q.numDirs - 1)) != 0 ||
      q.numSets < 1 || q.numSets * q.numDirs > 1024) {
    std::fprintf(stderr, "bad dimensions\n");
    return 2;
  }
  const size_t values = sparse ? (size_t)numBlocks * snb::kBlockPoints : (size_t)d0 * d1 * d2;
  std::vector<int32_t> list(sparse ? (size_t)numBlocks * 4 : 0), ids(head[5] ? values : 0);
  std::vector<float> dist(values);
  q.points.resize((size_t)numPoints * 4);
  q.normals.resize(head[7] ? (size_t)numPoints * 4 : 0);
  q.table.resize((size_t)q.numSets * q.numDirs * 4);
  if (!get(in, list.data(), list.size()) || !get(in, dist.data(), values) || !get(in, ids.data(), ids.size()) ||
      !get(in, q.points.data(), q.points.size()) || !get(in, q.normals.data(), q.normals.size()) || !get(in, q.table.data(), q.table.size())) {
    std::fprintf(stderr, "short query\n");
    return 2;
  }
  std::fclose(in);
  const fm::Frame L{{origin[0], origin[1], origin[2]}, {step[0], step[1], step[2]}};
  std::vector<unsigned char> out;
  if (sparse) {
    std::vector<uint32_t> first((size_t)d0 * d1 * d2, snb::kNoEntry);
    const snb::Blocks B{first.data(), d0, d1, d2};
    const int g[3] = {fs::groups(d0), fs::groups(d1), fs::groups(d2)};
    std::vector<unsigned long long> mask((size_t)g[0] * g[1] * g[2], 0ull);
    for (int n = 0; n < numBlocks; n++) {
      const int bi = list[4 * (size_t)n], bj = list[4 * (size_t)n + 1], bk = list[4 * (size_t)n + 2];
      if (!snb::in_range(B, bi, bj, bk)) continue;
      if (first[snb::block_linear(B, bi, bj, bk)] == snb::kNoEntry) first[snb::block_linear(B, bi, bj, bk)] = (uint32_t)n;
      mask[fs::group_linear(g, bi, bj, bk)] |= 1ull << fs::block_bit(bi, bj, bk);
    }
    run(fm::Blocks{dist.data(), head[5] ? ids.data() : nullptr, B}, fs::Coarse{mask.data(), {g[0], g[1], g[2]}}, L, q, out);
  } else {
    run(fm::Dense{dist.data(), head[5] ? ids.data() : nullptr, {d0, d1, d2}}, fs::Coarse{nullptr, {0, 0, 0}}, L, q, out);
  }
  FILE *of = std::fopen(argv[2], "wb");
  if (!of) { std::perror(argv[2]); return 2; }
  const bool ok = out.empty() || std::fwrite(out.data(), 1, out.size(), of) == out.size();
  if (std::fclose(of) != 0 || !ok) { std::fprintf(stderr, "short write\n"); return 2; }
  return 0;
}
