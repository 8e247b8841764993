// rm_sdf_mesh_blocks and rm_sdf_blocks_select's rule on the CPU, serially, through the very functions the kernels of rm_blocks.hip call
// (raymarcher_amd/csrc/rm_surface_nets_blocks.h and, through it, rm_surface_nets.h): the block map, the neighbour lookup, the
// stored-quad and open-vertex tests, a cell's vertex number from its block's base and mask.  A stand-alone program, so that it can
// run under the host sanitizers.
//   rm_sdf_blocks_cpu <blocks file> <mesh file>
// blocks file: int32 mx, my, mz, numBlocks, hasIds; float origin[3], step[3], iso; numBlocks·4 int32 (the list); numBlocks·729
// floats; then as many int32 with hasIds.
// mesh file: uint32 numVertices, numQuads, numOpen; 4 floats per vertex; one int32 per vertex; 4 int32 per quad; then one int32 per
// entry: −1 for a void entry, else whether the block is active under rm_sdf_blocks_select's rule.
// Build with -ffp-contract=off: every operation of the definition is one binary32 operation.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../raymarcher_amd/csrc/rm_surface_nets_blocks.h"

namespace sn = rm::sn;
namespace snb = rm::snb;

template <class T>
static bool get(FILE *f, T *p, size_t n) { return n == 0 || std::fread(p, sizeof(T), n, f) == n; }
template <class T>
static bool put(FILE *f, const T *p, size_t n) { return n == 0 || std::fwrite(p, sizeof(T), n, f) == n; }

int main(int argc, char **argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s blocks mesh\n", argv[0]); return 2; }
  FILE *in = std::fopen(argv[1], "rb");
  if (!in) { std::perror(argv[1]); return 2; }
  int32_t head[5];
  float origin[3], step[3], iso;
  if (!get(in, head, 5) || !get(in, origin, 3) || !get(in, step, 3) || !get(in, &iso, 1)) { std::fprintf(stderr, "short header\n"); return 2; }
  const int mx = head[0], my = head[1], mz = head[2], numBlocks = head[3];
  if (mx < 1 || my < 1 || mz < 1 || mx > 512 || my > 512 || mz > 512 || numBlocks < 0 || numBlocks > (1 << 22)) {
    std::fprintf(stderr, "bad dimensions\n");
    return 2;
  }
  const size_t values = (size_t)numBlocks * snb::kBlockPoints;
  std::vector<int32_t> list((size_t)numBlocks * 4), ids(head[4] ? values : 0);
  std::vector<float> dist(values);
  if (!get(in, list.data(), list.size()) || !get(in, dist.data(), values) || (head[4] && !get(in, ids.data(), values))) {
    std::fprintf(stderr, "short blocks\n");
    return 2;
  }
  std::fclose(in);

  // the block map: the first entry that names a block
  std::vector<uint32_t> first((size_t)mx * my * mz, snb::kNoEntry);
  const snb::Blocks B{first.data(), mx, my, mz};
  for (int n = 0; n < numBlocks; n++) {
    const int bi = list[4 * (size_t)n], bj = list[4 * (size_t)n + 1], bk = list[4 * (size_t)n + 2];
    if (snb::in_range(B, bi, bj, bk) && first[snb::block_linear(B, bi, bj, bk)] == snb::kNoEntry) first[snb::block_linear(B, bi, bj, bk)] = (uint32_t)n;
  }
  auto self_of = [&](int n) { return snb::Self{list[4 * (size_t)n], list[4 * (size_t)n + 1], list[4 * (size_t)n + 2], (uint32_t)n}; };
  auto is_listed = [&](const snb::Self &s) { return snb::entry_listed(B, s.bi, s.bj, s.bk, s.n); };

  // the count: bases, masks, open vertices, the select rule
  std::vector<unsigned long long> base((size_t)numBlocks + 1, 0);
  std::vector<uint32_t> masks((size_t)numBlocks * snb::kMaskWords, 0u);
  std::vector<int32_t> active(numBlocks, -1);
  uint32_t open = 0;
  for (int n = 0; n < numBlocks; n++) {
    base[n + 1] = base[n];
    const snb::Self s = self_of(n);
    if (!is_listed(s)) continue;
    const float *vals = dist.data() + (size_t)n * snb::kBlockPoints;
    active[n] = snb::block_active(vals, iso) ? 1 : 0;
    for (int c = 0; c < 8; c++)
      for (int b = 0; b < 8; b++)
        for (int a = 0; a < 8; a++) {
          float v[8];
          snb::cell_corners(vals, a, b, c, v);
          const unsigned mask = sn::corner_mask(v, iso);
          if (!sn::cell_active(mask)) continue;
          const int cell = snb::cell_index(a, b, c);
          masks[(size_t)n * snb::kMaskWords + (cell >> 5)] |= 1u << (cell & 31);
          base[n + 1]++;
          if (snb::cell_open(B, s, mask, a, b, c)) open++;
        }
  }
  const unsigned long long total = base[numBlocks];

  // the vertices and the quads, in the definition's order
  std::vector<float> verts;
  std::vector<int32_t> vobj, quads;
  for (int n = 0; n < numBlocks; n++) {
    const snb::Self s = self_of(n);
    if (!is_listed(s)) continue;
    const float *vals = dist.data() + (size_t)n * snb::kBlockPoints;
    for (int c = 0; c < 8; c++)
      for (int b = 0; b < 8; b++)
        for (int a = 0; a < 8; a++) {
          float v[8];
          snb::cell_corners(vals, a, b, c, v);
          const unsigned mask = sn::corner_mask(v, iso);
          if (sn::cell_active(mask)) {
            float local[3];
            sn::cell_vertex(v, iso, mask, local);
            if ((unsigned long long)vobj.size() != base[n] + snb::mask_rank(masks.data() + (size_t)n * snb::kMaskWords, (unsigned)snb::cell_index(a, b, c))) {
              std::fprintf(stderr, "a vertex number disagrees with its base and mask\n");
              return 3;
            }
            verts.push_back(sn::vertex_world(origin[0], step[0], 8 * s.bi + a, local[0]));
            verts.push_back(sn::vertex_world(origin[1], step[1], 8 * s.bj + b, local[1]));
            verts.push_back(sn::vertex_world(origin[2], step[2], 8 * s.bk + c, local[2]));
            verts.push_back(0.0f);
            const int k = sn::first_inside_corner(mask);
            vobj.push_back(head[4] ? ids[(size_t)n * snb::kBlockPoints + snb::point_index(a + (k & 1), b + ((k >> 1) & 1), c + ((k >> 2) & 1))] : -1);
          }
          for (int axis = 0; axis < 3; axis++) {
            if (snb::owned_edge_state(B, s, mask, axis, a, b, c) != snb::kEdgeQuad) continue;
            int32_t vtx[4];
            snb::quad_vertices(B, s, base.data(), masks.data(), total, axis, a, b, c, (mask & 1u) != 0u, vtx);
            for (int q = 0; q < 4; q++) quads.push_back(vtx[q]);
          }
        }
  }

  FILE *out = std::fopen(argv[2], "wb");
  if (!out) { std::perror(argv[2]); return 2; }
  const uint32_t counts[3] = {(uint32_t)vobj.size(), (uint32_t)(quads.size() / 4), open};
  const bool ok = put(out, counts, 3) && put(out, verts.data(), verts.size()) && put(out, vobj.data(), vobj.size()) &&
                  put(out, quads.data(), quads.size()) && put(out, active.data(), active.size());
  if (std::fclose(out) != 0 || !ok) { std::fprintf(stderr, "short write\n"); return 2; }
  return 0;
}
