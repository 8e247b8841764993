// rm_sdf_mesh on the CPU, serially, through the very functions the kernels of rm_volume.hip call (raymarcher_amd/csrc/rm_surface_nets.h):
// the per-cell vertex and the per-edge quad.  A stand-alone program, so that it can run under the host sanitizers.
//   rm_sdf_mesh_cpu <lattice file> <mesh file>
// lattice file: int32 nx, ny, nz, hasIds; float origin[3], step[3], iso; nx·ny·nz floats, x fastest; then as many int32 with hasIds.
// mesh file: uint32 numVertices, numQuads; 4 floats per vertex; one int32 per vertex; 4 int32 per quad.
// Build with -ffp-contract=off: every operation of the definition is one binary32 operation.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../raymarcher_amd/csrc/rm_surface_nets.h"

namespace sn = rm::sn;

template <class T>
static bool get(FILE *f, T *p, size_t n) { return std::fread(p, sizeof(T), n, f) == n; }
template <class T>
static bool put(FILE *f, const T *p, size_t n) { return n == 0 || std::fwrite(p, sizeof(T), n, f) == n; }

int main(int argc, char **argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s lattice mesh\n", argv[0]); return 2; }
  FILE *in = std::fopen(argv[1], "rb");
  if (!in) { std::perror(argv[1]); return 2; }
  int32_t head[4];
  float origin[3], step[3], iso;
  if (!get(in, head, 4) || !get(in, origin, 3) || !get(in, step, 3) || !get(in, &iso, 1)) { std::fprintf(stderr, "short header\n"); return 2; }
  const int nx = head[0], ny = head[1], nz = head[2];
  if (nx < 1 || ny < 1 || nz < 1 || nx > 4096 || ny > 4096 || nz > 4096) { std::fprintf(stderr, "bad dimensions\n"); return 2; }
  const size_t points = (size_t)nx * ny * nz;
  std::vector<float> dist(points);
  std::vector<int32_t> ids(head[3] ? points : 0);
  if (!get(in, dist.data(), points) || (head[3] && !get(in, ids.data(), points))) { std::fprintf(stderr, "short lattice\n"); return 2; }
  std::fclose(in);

  auto at = [&](int i, int j, int k) { return ((size_t)k * ny + j) * nx + i; };
  const int cx = nx - 1, cy = ny - 1, cz = nz - 1;
  auto cell = [&](int i, int j, int k) { return ((size_t)k * cy + j) * cx + i; };
  std::vector<int32_t> number((size_t)cx * cy * cz, -1), vobj, quads;
  std::vector<float> verts;
  for (int k = 0; k < cz; k++)
    for (int j = 0; j < cy; j++)
      for (int i = 0; i < cx; i++) {
        float v[8];
        for (int c = 0; c < 8; c++) v[c] = dist[at(i + (c & 1), j + ((c >> 1) & 1), k + ((c >> 2) & 1))];
        const unsigned mask = sn::corner_mask(v, iso);
        if (!sn::cell_active(mask)) continue;
        float local[3];
        sn::cell_vertex(v, iso, mask, local);
        number[cell(i, j, k)] = (int32_t)vobj.size();
        verts.push_back(sn::vertex_world(origin[0], step[0], i, local[0]));
        verts.push_back(sn::vertex_world(origin[1], step[1], j, local[1]));
        verts.push_back(sn::vertex_world(origin[2], step[2], k, local[2]));
        verts.push_back(0.0f);
        const int c = sn::first_inside_corner(mask);
        vobj.push_back(head[3] ? ids[at(i + (c & 1), j + ((c >> 1) & 1), k + ((c >> 2) & 1))] : -1);
      }
  for (int k = 0; k < nz; k++)
    for (int j = 0; j < ny; j++)
      for (int i = 0; i < nx; i++)
        for (int axis = 0; axis < 3; axis++) {
          if (!sn::edge_interior(axis, i, j, k, nx, ny, nz)) continue;
          const bool p = sn::inside(dist[at(i, j, k)], iso);
          const bool e = sn::inside(dist[at(i + (axis == 0), j + (axis == 1), k + (axis == 2))], iso);
          if (p == e) continue;
          int cells[4][3];
          sn::edge_cells(axis, i, j, k, p, cells);
          for (int q = 0; q < 4; q++) quads.push_back(number[cell(cells[q][0], cells[q][1], cells[q][2])]);
        }

  FILE *out = std::fopen(argv[2], "wb");
  if (!out) { std::perror(argv[2]); return 2; }
  const uint32_t counts[2] = {(uint32_t)vobj.size(), (uint32_t)(quads.size() / 4)};
  const bool ok = put(out, counts, 2) && put(out, verts.data(), verts.size()) && put(out, vobj.data(), vobj.size()) &&
                  put(out, quads.data(), quads.size());
  if (std::fclose(out) != 0 || !ok) { std::fprintf(stderr, "short write\n"); return 2; }
  return 0;
}
