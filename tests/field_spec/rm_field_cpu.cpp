// rm_sdf_sample, rm_sdf_sample_blocks, rm_sdf_trace and rm_sdf_trace_blocks on the CPU, serially, through the very functions the
// kernels of rm_field.hip call (raymarcher_amd/csrc/rm_field_march.h).  A stand-alone program, so that it can run under the host
// sanitizers.
//   rm_field_cpu <query file> <result file>
// query file: int32 sparse, d0, d1, d2 (n per axis, or m per axis with sparse), numBlocks, hasIds, numPoints, numRays, maxSteps,
// noNormal; float origin[3], step[3], iso; numBlocks·4 int32 (the list, sparse only); the values — d0·d1·d2 floats, or numBlocks·729
// with sparse —; as many int32 with hasIds; numPoints·4 floats; numRays·8 floats.
// result file: numPoints records of 32 bytes (RmFieldSample), then numRays records of 32 bytes (RmRayHit).
// Build with -ffp-contract=off: every operation of the definition is one binary32 operation.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../raymarcher_amd/csrc/rm_field_march.h"

namespace fm = rm::fm;
namespace snb = rm::snb;

template <class T>
static bool get(FILE *f, T *p, size_t n) { return n == 0 || std::fread(p, sizeof(T), n, f) == n; }

template <class Field>
static void run(const Field &F, const fm::Frame &L, const std::vector<float> &points, const std::vector<float> &rays, float iso, int maxSteps,
                bool noNormal, std::vector<unsigned char> &out) {
  static_assert(sizeof(fm::Sample) == 32 && sizeof(fm::Hit) == 32, "records of 32 bytes");
  const size_t np = points.size() / 4, nr = rays.size() / 8;
  out.resize((np + nr) * 32);
  for (size_t i = 0; i < np; i++) {
    const fm::Sample s = fm::sample_point(F, L, &points[4 * i]);
    std::memcpy(&out[32 * i], &s, 32);
  }
  for (size_t i = 0; i < nr; i++) {
    const float *q = &rays[8 * i];
    const fm::Ray r{{q[0], q[1], q[2]}, q[3], {q[4], q[5], q[6]}};
    const fm::Hit h = fm::march_ray(F, L, r, iso, maxSteps, noNormal);
    std::memcpy(&out[32 * (np + i)], &h, 32);
  }
}

int main(int argc, char **argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s query result\n", argv[0]); return 2; }
  FILE *in = std::fopen(argv[1], "rb");
  if (!in) { std::perror(argv[1]); return 2; }
  int32_t head[10];
  float origin[3], step[3], iso;
  if (!get(in, head, 10) || !get(in, origin, 3) || !get(in, step, 3) || !get(in, &iso, 1)) { std::fprintf(stderr, "short header\n"); return 2; }
  const bool sparse = head[0] != 0;
  const int d0 = head[1], d1 = head[2], d2 = head[3], numBlocks = head[4], numPoints = head[6], numRays = head[7], maxSteps = head[8];
  const int lo = sparse ? 1 : 2, hi = sparse ? 512 : 4096;
  if (d0 < lo || d1 < lo || d2 < lo || d0 > hi || d1 > hi || d2 > hi || numBlocks < 0 || numBlocks > (1 << 22) || numPoints < 0 || numRays < 0 ||
      maxSteps < 0 || maxSteps > 65536) {
    std::fprintf(stderr, "bad dimensions\n");
    return 2;
  }
  const size_t values = sparse ? (size_t)numBlocks * snb::kBlockPoints : (size_t)d0 * d1 * d2;
  std::vector<int32_t> list(sparse ? (size_t)numBlocks * 4 : 0), ids(head[5] ? values : 0);
  std::vector<float> dist(values), points((size_t)numPoints * 4), rays((size_t)numRays * 8);
  if (!get(in, list.data(), list.size()) || !get(in, dist.data(), values) || !get(in, ids.data(), ids.size()) ||
      !get(in, points.data(), points.size()) || !get(in, rays.data(), rays.size())) {
    std::fprintf(stderr, "short query\n");
    return 2;
  }
  std::fclose(in);
  const fm::Frame L{{origin[0], origin[1], origin[2]}, {step[0], step[1], step[2]}};
  std::vector<unsigned char> out;
  if (sparse) {
    // the block map: the first entry that names a block
    std::vector<uint32_t> first((size_t)d0 * d1 * d2, snb::kNoEntry);
    const snb::Blocks B{first.data(), d0, d1, d2};
    for (int n = 0; n < numBlocks; n++) {
      const int bi = list[4 * (size_t)n], bj = list[4 * (size_t)n + 1], bk = list[4 * (size_t)n + 2];
      if (snb::in_range(B, bi, bj, bk) && first[snb::block_linear(B, bi, bj, bk)] == snb::kNoEntry) first[snb::block_linear(B, bi, bj, bk)] = (uint32_t)n;
    }
    run(fm::Blocks{dist.data(), head[5] ? ids.data() : nullptr, B}, L, points, rays, iso, maxSteps, head[9] != 0, out);
  } else {
    run(fm::Dense{dist.data(), head[5] ? ids.data() : nullptr, {d0, d1, d2}}, L, points, rays, iso, maxSteps, head[9] != 0, out);
  }
  FILE *of = std::fopen(argv[2], "wb");
  if (!of) { std::perror(argv[2]); return 2; }
  const bool ok = out.empty() || std::fwrite(out.data(), 1, out.size(), of) == out.size();
  if (std::fclose(of) != 0 || !ok) { std::fprintf(stderr, "short write\n"); return 2; }
  return 0;
}
