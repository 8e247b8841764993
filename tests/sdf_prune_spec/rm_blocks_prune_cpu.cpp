// rm_sdf_blocks_select_pruned's classification on the CPU, serially, through the very functions the library calls
// (raymarcher_amd/csrc/rm_blocks_prune.h): the bounds from the step and the two constants, the far tests of a corner, the
// eight-corner rule.  A stand-alone program, so that it can run under the host sanitizers.
//   rm_blocks_prune_cpu <corners file> <flags file>
// corners file: int32 mx, my, mz; float step[3], iso, lipschitzOut, lipschitzIn; (mx + 1)(my + 1)(mz + 1) floats, x fastest.
// flags file: float bOut, bIn; then one uint32 per block in linear order (bk·my + bj)·mx + bi: 1 for a candidate, 0 for a discarded
// block.
// Build with -ffp-contract=off: every operation of the definition is one binary32 operation.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../raymarcher_amd/csrc/rm_blocks_prune.h"

namespace prune = rm::prune;

template <class T>
static bool get(FILE *f, T *p, size_t n) { return n == 0 || std::fread(p, sizeof(T), n, f) == n; }
template <class T>
static bool put(FILE *f, const T *p, size_t n) { return n == 0 || std::fwrite(p, sizeof(T), n, f) == n; }

int main(int argc, char **argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s corners flags\n", argv[0]); return 2; }
  FILE *in = std::fopen(argv[1], "rb");
  if (!in) { std::perror(argv[1]); return 2; }
  int32_t dims[3];
  float step[3], rest[3];  // iso, lipschitzOut, lipschitzIn
  if (!get(in, dims, 3) || !get(in, step, 3) || !get(in, rest, 3)) { std::fprintf(stderr, "short header\n"); return 2; }
  const int mx = dims[0], my = dims[1], mz = dims[2];
  if (mx < 1 || my < 1 || mz < 1 || mx > 512 || my > 512 || mz > 512) { std::fprintf(stderr, "bad dimensions\n"); return 2; }
  std::vector<float> corners((size_t)(mx + 1) * (my + 1) * (mz + 1));
  if (!get(in, corners.data(), corners.size())) { std::fprintf(stderr, "short corners\n"); return 2; }
  std::fclose(in);

  const prune::Bounds b = prune::bounds(step, rest[1], rest[2]);
  std::vector<uint32_t> flags((size_t)mx * my * mz);
  for (int bk = 0; bk < mz; bk++)
    for (int bj = 0; bj < my; bj++)
      for (int bi = 0; bi < mx; bi++) {
        float c[8];
        prune::block_corners(corners.data(), mx, my, bi, bj, bk, c);
        flags[((size_t)bk * my + bj) * mx + bi] = prune::discarded(c, rest[0], b) ? 0u : 1u;
      }

  FILE *out = std::fopen(argv[2], "wb");
  if (!out) { std::perror(argv[2]); return 2; }
  const float bs[2] = {b.out, b.in};
  if (!put(out, bs, 2) || !put(out, flags.data(), flags.size())) { std::fprintf(stderr, "short write\n"); return 2; }
  return std::fclose(out) == 0 ? 0 : 2;
}
