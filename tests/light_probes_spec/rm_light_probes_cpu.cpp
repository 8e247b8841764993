// rm_light_probes behind the shaded ray on the CPU, serially, through the very functions the kernel's pieces come from
// (raymarcher_amd/csrc/rm_light_probes.h: probe_record, the sequential walk of the tree).  A stand-alone program, so that it can run
// under the host sanitizers.
//   rm_light_probes_cpu <query file> <result file>
// query file: int32 numProbes, numDirs, numSets; numProbes·4 floats (the positions); numSets·numDirs·16 floats (the table);
// numProbes·numDirs·4 floats (the rays' colours, probe-major); numProbes·numDirs bytes (their hit flags).
// result file: numProbes records of 160 bytes (RmLightProbe).
// Build with -ffp-contract=off: every operation of the definition is one binary32 operation.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../raymarcher_amd/csrc/rm_light_probes.h"

namespace lp = rm::lp;

template <class T>
static bool get(FILE *f, T *p, size_t n) { return n == 0 || std::fread(p, sizeof(T), n, f) == n; }

int main(int argc, char **argv) {
  static_assert(sizeof(lp::Row) == 64 && sizeof(lp::Probe) == 160, "rows of 64 bytes, records of 160");
  if (argc != 3) { std::fprintf(stderr, "usage: %s query result\n", argv[0]); return 2; }
  FILE *in = std::fopen(argv[1], "rb");
  if (!in) { std::perror(argv[1]); return 2; }
  int32_t head[3];
  if (!get(in, head, 3)) { std::fprintf(stderr, "short header\n"); return 2; }
  const int numProbes = head[0], numDirs = head[1], numSets = head[2];
  if (numProbes < 0 || numProbes > (1 << 20) || numDirs < 1 || numDirs > lp::kMaxDirs || (numDirs & (numDirs - 1)) != 0 || numSets < 1 ||
      numSets * numDirs > 4096) {
    std::fprintf(stderr, "bad dimensions\n");
    return 2;
  }
  const size_t raysN = (size_t)numProbes * (size_t)numDirs;
  std::vector<float> positions((size_t)numProbes * 4), colours(raysN * 4);
  std::vector<lp::Row> table((size_t)numSets * (size_t)numDirs);
  std::vector<uint8_t> hit(raysN);
  if (!get(in, positions.data(), positions.size()) || !get(in, table.data(), table.size()) || !get(in, colours.data(), colours.size()) ||
      !get(in, hit.data(), hit.size())) {
    std::fprintf(stderr, "short query\n");
    return 2;
  }
  std::fclose(in);
  std::vector<lp::Probe> out((size_t)numProbes);
  for (size_t i = 0; i < (size_t)numProbes; i++)
    out[i] = lp::probe_record(&positions[4 * i], colours.data() + 4 * i * (size_t)numDirs, hit.data() + i * (size_t)numDirs,
                              table.data() + (i % (size_t)numSets) * (size_t)numDirs, numDirs);
  FILE *of = std::fopen(argv[2], "wb");
  if (!of) { std::perror(argv[2]); return 2; }
  const bool ok = out.empty() || std::fwrite(out.data(), sizeof(lp::Probe), out.size(), of) == out.size();
  if (std::fclose(of) != 0 || !ok) { std::fprintf(stderr, "short write\n"); return 2; }
  return 0;
}
