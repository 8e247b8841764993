// rm_field_trace on the CPU, serially, through the very function the handle kernels of rm_field.hip call
// (raymarcher_amd/csrc/rm_field_skip.h).  A stand-alone program, so that it can run under the host sanitizers.  The block map and the
// coarse level are built here by a plain loop over the list.
//   rm_field_handle_cpu <query file> <result file>
// query file: int32 sparse, d0, d1, d2 (n per axis, or m per axis with sparse), numBlocks, hasIds, numRays, maxSteps, mode (0, 1 or
// 2: RM_TRACE_CLOSEST, RM_TRACE_NO_NORMAL, RM_TRACE_OCCLUSION); float origin[3], step[3], iso; numBlocks·4 int32 (the list, sparse
// only); the values — d0·d1·d2 floats, or numBlocks·729 with sparse —; as many int32 with hasIds; numRays·8 floats.
// result file: numRays records of 32 bytes (RmRayHit).
// Build with -ffp-contract=off: every operation of the definition is one binary32 operation; -DRM_FIELD_COARSE=0 builds the march
// that does not read the coarse level.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../raymarcher_amd/csrc/rm_field_skip.h"

namespace fm = rm::fm;
namespace fs = rm::fs;
namespace snb = rm::snb;

template <class T>
static bool get(FILE *f, T *p, size_t n) { return n == 0 || std::fread(p, sizeof(T), n, f) == n; }

template <class Field>
static void run(const Field &F, const fs::Coarse &C, const fm::Frame &L, const std::vector<float> &rays, float iso, int maxSteps, int mode,
                std::vector<unsigned char> &out) {
  static_assert(sizeof(fm::Hit) == 32, "records of 32 bytes");
  const size_t nr = rays.size() / 8;
  out.resize(nr * 32);
  for (size_t i = 0; i < nr; i++) {
    const float *q = &rays[8 * i];
    const fm::Ray r{{q[0], q[1], q[2]}, q[3], {q[4], q[5], q[6]}};
    const fm::Hit h = mode == 2 ? fs::march_ray<true>(F, C, L, r, iso, maxSteps, false) : fs::march_ray<false>(F, C, L, r, iso, maxSteps, mode == 1);
    std::memcpy(&out[32 * i], &h, 32);
  }
}

int main(int argc, char **argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s query result\n", argv[0]); return 2; }
  FILE *in = std::fopen(argv[1], "rb");
  if (!in) { std::perror(argv[1]); return 2; }
  int32_t head[9];
  float origin[3], step[3], iso;
  if (!get(in, head, 9) || !get(in, origin, 3) || !get(in, step, 3) || !get(in, &iso, 1)) { std::fprintf(stderr, "short header\n"); return 2; }
  const bool sparse = head[0] != 0;
  const int d0 = head[1], d1 = head[2], d2 = head[3], numBlocks = head[4], numRays = head[6], maxSteps = head[7], mode = head[8];
  const int lo = sparse ? 1 : 2, hi = sparse ? 512 : 4096;
  if (d0 < lo || d1 < lo || d2 < lo || d0 > hi || d1 > hi || d2 > hi || numBlocks < 0 || numBlocks > (1 << 22) || numRays < 0 || maxSteps < 0 ||
      maxSteps > 65536 || mode < 0 || mode > 2) {
    std::fprintf(stderr, "bad dimensions\n");
    return 2;
  }
  const size_t values = sparse ? (size_t)numBlocks * snb::kBlockPoints : (size_t)d0 * d1 * d2;
  std::vector<int32_t> list(sparse ? (size_t)numBlocks * 4 : 0), ids(head[5] ? values : 0);
  std::vector<float> dist(values), rays((size_t)numRays * 8);
  if (!get(in, list.data(), list.size()) || !get(in, dist.data(), values) || !get(in, ids.data(), ids.size()) || !get(in, rays.data(), rays.size())) {
    std::fprintf(stderr, "short query\n");
    return 2;
  }
  std::fclose(in);
  const fm::Frame L{{origin[0], origin[1], origin[2]}, {step[0], step[1], step[2]}};
  std::vector<unsigned char> out;
  if (sparse) {
    // the block map — the first entry that names a block — and the coarse level: a bit per block an entry names
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
    run(fm::Blocks{dist.data(), head[5] ? ids.data() : nullptr, B}, fs::Coarse{mask.data(), {g[0], g[1], g[2]}}, L, rays, iso, maxSteps, mode, out);
  } else {
    run(fm::Dense{dist.data(), head[5] ? ids.data() : nullptr, {d0, d1, d2}}, fs::Coarse{nullptr, {0, 0, 0}}, L, rays, iso, maxSteps, mode, out);
  }
  FILE *of = std::fopen(argv[2], "wb");
  if (!of) { std::perror(argv[2]); return 2; }
  const bool ok = out.empty() || std::fwrite(out.data(), 1, out.size(), of) == out.size();
  if (std::fclose(of) != 0 || !ok) { std::fprintf(stderr, "short write\n"); return 2; }
  return 0;
}
