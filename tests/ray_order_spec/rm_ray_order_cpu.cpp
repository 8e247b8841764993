// rm_ray_order_cpu.cpp — rm_rays_order's arithmetic on the CPU: raymarcher_amd/csrc/rm_ray_key.h, the header the kernels compile,
// run serially — the bounds, the keys, a plain stable sort.  A stand-alone program so that the tests can run it under the host
// sanitizers as a child process (tests/ray_order_helpers.py builds it: g++, ASan and UBSan linked statically, -ffp-contract=off).
//   rm_ray_order_cpu <in> <out>
//   in : int32 n, originBits, dirBits, flipZeros; then n rays of 8 float32
//   out: n uint64 keys in input order; n int32 order; 5 float32 lo; 5 float32 hi
// flipZeros != 0: every bound that is a zero has its sign bit inverted before the keys are made (which of −0 and +0 becomes a bound
// is not defined, and must not matter).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <vector>

#include "../../raymarcher_amd/csrc/rm_ray_key.h"

static int fail(const char *what) {
  std::fprintf(stderr, "rm_ray_order_cpu: %s\n", what);
  return 1;
}

int main(int argc, char **argv) {
  if (argc != 3) return fail("usage: rm_ray_order_cpu <in> <out>");
  std::FILE *f = std::fopen(argv[1], "rb");
  if (!f) return fail("cannot open the input");
  int32_t head[4];
  if (std::fread(head, sizeof(int32_t), 4, f) != 4) return fail("short header");
  const int32_t n = head[0], originBits = head[1], dirBits = head[2], flipZeros = head[3];
  if (n < 0 || originBits < 0 || originBits > rk::kMaxOriginBits || dirBits < 0 || dirBits > rk::kMaxDirBits) return fail("bad header");
  std::vector<float> rays((size_t)n * 8);
  if (n > 0 && std::fread(rays.data(), sizeof(float), rays.size(), f) != rays.size()) return fail("short ray array");  // n = 0: data() may be null
  std::fclose(f);

  rk::Bounds b;
  rk::bounds_empty(b);
  for (int32_t i = 0; i < n; i++) {
    float c[rk::kCoords];
    if (rk::coords(&rays[(size_t)i * 8], &rays[(size_t)i * 8 + 4], c)) rk::bounds_add(b, c);
  }
  if (flipZeros) {
    for (int k = 0; k < rk::kCoords; k++) {
      if (b.lo[k] == 0.0f) b.lo[k] = -b.lo[k];
      if (b.hi[k] == 0.0f) b.hi[k] = -b.hi[k];
    }
  }
  std::vector<uint64_t> keys((size_t)n);
  for (int32_t i = 0; i < n; i++) keys[(size_t)i] = rk::ray_key(&rays[(size_t)i * 8], &rays[(size_t)i * 8 + 4], b, originBits, dirBits);
  std::vector<int32_t> order((size_t)n);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&keys](int32_t a, int32_t c) { return keys[(size_t)a] < keys[(size_t)c]; });

  std::FILE *o = std::fopen(argv[2], "wb");
  if (!o) return fail("cannot open the output");
  bool ok = n == 0 || std::fwrite(keys.data(), sizeof(uint64_t), keys.size(), o) == keys.size();
  ok = ok && (n == 0 || std::fwrite(order.data(), sizeof(int32_t), order.size(), o) == order.size());
  ok = ok && std::fwrite(b.lo, sizeof(float), rk::kCoords, o) == (size_t)rk::kCoords;
  ok = ok && std::fwrite(b.hi, sizeof(float), rk::kCoords, o) == (size_t)rk::kCoords;
  ok = (std::fclose(o) == 0) && ok;
  return ok ? 0 : fail("short write");
}
