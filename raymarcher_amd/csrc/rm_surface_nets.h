// rm_surface_nets.h — the arithmetic of rm_sdf_mesh (naive surface nets; include/raymarcher_amd.h has the definition): the vertex of
// one cell and the quad of one lattice edge.  Plain C++ with no device built-in, so the kernels of rm_volume.hip and a host program
// (tests/sdf_mesh_spec/rm_sdf_mesh_cpu.cpp) run the very same code.  Every operation is one binary32 operation as written: compile
// with -ffp-contract=off (the library's flags), or the vertex's multiply-add fuses.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define RM_SN_FN __host__ __device__ inline
#else
#define RM_SN_FN inline
#endif

namespace rm {
namespace sn {

// inside(v) = v < iso: a NaN is outside
RM_SN_FN bool inside(float v, float iso) { return v < iso; }

// Bit c of the mask: corner c = cx + 2·cy + 4·cz of the cell, v[c] the lattice value at (i + cx, j + cy, k + cz), is inside.
RM_SN_FN unsigned corner_mask(const float v[8], float iso) {
  unsigned m = 0;
#pragma unroll
  for (int c = 0; c < 8; c++) m |= inside(v[c], iso) ? (1u << c) : 0u;
  return m;
}
RM_SN_FN bool cell_active(unsigned mask) { return mask != 0u && mask != 0xffu; }
// the first inside corner in corner order (an active cell has one)
RM_SN_FN int first_inside_corner(unsigned mask) {
  int c = 0;
  while (c < 7 && !((mask >> c) & 1u)) c++;
  return c;
}

// The vertex of an ACTIVE cell in the cell's own coordinates, each in [0, 1]: the mean of the crossings of the twelve edges in
// their order — x-edges (0,1) (2,3) (4,5) (6,7), y-edges (0,2) (1,3) (4,6) (5,7), z-edges (0,4) (1,5) (2,6) (3,7).  A crossing is
// corner a with the edge's axis component replaced by t = (iso − v_a) / (v_b − v_a), or by 0.5 where t is not in [0, 1] (a NaN
// from infinities included).  An active cell has at least one crossing.
RM_SN_FN void cell_vertex(const float v[8], float iso, unsigned mask, float local[3]) {
  float acc[3] = {0.0f, 0.0f, 0.0f};
  int n = 0;
#pragma unroll
  for (int axis = 0; axis < 3; axis++) {
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const int a = axis == 0 ? 2 * e : (axis == 1 ? (e & 1) + 4 * (e >> 1) : e), b = a + (1 << axis);
      if (((mask >> a) ^ (mask >> b)) & 1u) {
        float t = (iso - v[a]) / (v[b] - v[a]);
        if (!(t >= 0.0f && t <= 1.0f)) t = 0.5f;
        float c[3] = {(float)(a & 1), (float)((a >> 1) & 1), (float)((a >> 2) & 1)};
        c[axis] = t;
        acc[0] += c[0];
        acc[1] += c[1];
        acc[2] += c[2];
        n++;
      }
    }
  }
  const float inv = 1.0f / (float)n;
  local[0] = acc[0] * inv;
  local[1] = acc[1] * inv;
  local[2] = acc[2] * inv;
}
// one world coordinate of the vertex of the cell whose index on that axis is i: add, multiply, add
RM_SN_FN float vertex_world(float origin, float step, int i, float local) {
  const float cell = (float)i + local;
  const float scaled = cell * step;
  return origin + scaled;
}

// The lattice edge from P = (i, j, k) to P + e_axis exists and is interior in the other two axes: only such an edge has four cells
// around it.
RM_SN_FN bool edge_interior(int axis, int i, int j, int k, int nx, int ny, int nz) {
  const bool xi = i >= 1 && i <= nx - 2, yi = j >= 1 && j <= ny - 2, zi = k >= 1 && k <= nz - 2;
  if (axis == 0) return i <= nx - 2 && yi && zi;
  if (axis == 1) return j <= ny - 2 && xi && zi;
  return k <= nz - 2 && xi && yi;
}
// The four cells around that edge in the quad's order: counter-clockwise seen from +axis when P is inside, so that the normal
// points from the inside end to the outside end; (c0, c3, c2, c1) when P is outside.
RM_SN_FN void edge_cells(int axis, int i, int j, int k, bool pInside, int cells[4][3]) {
  const int d[3][4][3] = {{{0, -1, -1}, {0, 0, -1}, {0, 0, 0}, {0, -1, 0}},
                          {{-1, 0, -1}, {-1, 0, 0}, {0, 0, 0}, {0, 0, -1}},
                          {{-1, -1, 0}, {0, -1, 0}, {0, 0, 0}, {-1, 0, 0}}};
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int s = pInside ? q : (4 - q) & 3;
    cells[q][0] = i + d[axis][s][0];
    cells[q][1] = j + d[axis][s][1];
    cells[q][2] = k + d[axis][s][2];
  }
}

}  // namespace sn
}  // namespace rm
