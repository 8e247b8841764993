// rm_volume.hip — where the surface is (gfx950 only): the kernel of rm_sdf_grid, sdScene on a dense lattice, and the kernels and the
// entry point of rm_sdf_mesh, a quad mesh from any lattice of floats by naive surface nets.  include/raymarcher_amd.h has both
// definitions.  rm_sdf_grid's argument checks and staging are launch_sdf_grid in rm_queries.hip; everything of rm_sdf_mesh is
// here, as the post passes are in rm_post.hip.  rm_lattice.h has the lattice rules, rm_compact.hip.h the scan.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "rm_compact.hip.h"
#include "rm_device.hip.h"
#include "rm_lattice.h"
#include "rm_surface_nets.h"

namespace rm {

// ---- rm_sdf_grid ---------------------------------------------------------------------------------------------------------------
// One lane per lattice point, one wave per BRICK of the lattice: 4×4×4 points, lane l at (l & 3, (l >> 2) & 3, l >> 4) of it
// (RM_SDF_BRICK = 1: 8×8×1, lane l at (l & 7, l >> 3, 0)).  Neighbours in space share the evaluator's wave-uniform choices (the
// sponge's and the plain bulb's ballots), and a Mandelbulb's iteration counts — the wave runs as long as its slowest lane — differ
// least inside a compact brick.  A workgroup is four bricks that follow each other in x.  A lane outside the lattice leaves
// before the evaluation, as the probe kernels' lanes past n do: the evaluator's ballots are proofs about the lanes that are live,
// so a point's value does not depend on which other points share its wave.
// The evaluation is sdSceneImpl<BULB, 0, kTrapNone>: the instantiation of the table's march class (the table walk, the
// general Mandelbulb, the plain Mandelbulb) that the shadow marches of rm_trace_rays' kernels call, with no pass-over bound, no
// runner-up and no orbit trap — minD and minObjIdx are the same bits with and without the trap (rm_probe_sdscene_variant's tests).
// The point is origin + (float)i · step per axis: one multiply, one add, never fused (-ffp-contract=off, like every kernel here).
// Stores: a 4×4×4 brick writes sixteen 16-byte runs of d_dist, an 8×8×1 brick eight 32-byte runs; profiles/sdf_grid.md has both
// measured.
#ifndef RM_SDF_BRICK
#define RM_SDF_BRICK 0
#endif
static_assert(RM_SDF_BRICK == 0 || RM_SDF_BRICK == 1, "RM_SDF_BRICK: 0 = 4×4×4 bricks, 1 = 8×8×1 bricks");
constexpr int kBrickX = RM_SDF_BRICK ? 8 : 4, kBrickY = RM_SDF_BRICK ? 8 : 4, kBrickZ = RM_SDF_BRICK ? 1 : 4;

template <int BULB>
__global__ __launch_bounds__(256) void sdf_grid_kernel(const SceneBlock *__restrict__ sb, float ox, float oy, float oz, float sx,
                                                       float sy, float sz, int nx, int ny, int nz, float *__restrict__ dist,
                                                       int32_t *__restrict__ ids) {
  // the grid is (bricks along x / 4, bricks along y, bricks along z): a brick's place costs no division
  const unsigned bx = blockIdx.x * 4u + (threadIdx.x >> 6), by = blockIdx.y, bz = blockIdx.z, lane = threadIdx.x & 63u;
  const int i = (int)(bx * kBrickX + (RM_SDF_BRICK ? (lane & 7u) : (lane & 3u)));
  const int j = (int)(by * kBrickY + (RM_SDF_BRICK ? (lane >> 3) : ((lane >> 2) & 3u)));
  const int k = (int)(bz * kBrickZ + (RM_SDF_BRICK ? 0u : (lane >> 4)));
  if (i >= nx || j >= ny || k >= nz) return;
  const float fx = (float)i * sx, fy = (float)j * sy, fz = (float)k * sz;
  const V3 p = v3(ox + fx, oy + fy, oz + fz);
  Counters cnt{0, 0, 0, 0, 0, 0};
  float unused;
  const SceneMin m = sdSceneImpl<BULB, 0, kTrapNone>(sb, p, cnt, __builtin_inff(), unused);
  const size_t at = ((size_t)k * (size_t)ny + (size_t)j) * (size_t)nx + (size_t)i;
  dist[at] = m.d;
  if (ids) ids[at] = m.idx;
}

int launch_sdf_grid_kernel(const void *sbv, int bulbClass, const float origin[3], const float step[3], int nx, int ny, int nz,
                           float *d_dist, int32_t *d_objectId, hipStream_t stream) {
  const SceneBlock *sb = static_cast<const SceneBlock *>(sbv);
  // at most 1024 (4×4×4) or 512 (8×8×1) bricks along x and y and 4096 along z: every grid dimension is far below its limit of 65535
  const unsigned bricksX = (unsigned)((nx + kBrickX - 1) / kBrickX), bricksY = (unsigned)((ny + kBrickY - 1) / kBrickY),
                 bricksZ = (unsigned)((nz + kBrickZ - 1) / kBrickZ);
  const dim3 grid((bricksX + 3u) / 4u, bricksY, bricksZ), block(256);
  dispatch_march_class(bulbClass, [&](auto c) {
    hipLaunchKernelGGL(sdf_grid_kernel<decltype(c)::bulb>, grid, block, 0, stream, sb, origin[0], origin[1], origin[2], step[0], step[1],
                       step[2], nx, ny, nz, d_dist, d_objectId);
  });
  HIP_OK(hipGetLastError());
  return RM_OK;
}

// ---- rm_sdf_mesh ---------------------------------------------------------------------------------------------------------------
// Lattice points in their linear order q = (k·ny + j)·nx + i are dealt to workgroups of ONE wave, kMeshShare = 1024 consecutive
// points each (16 rounds of 64: a round reads 64 consecutive floats per corner).  Point q stands for two things: the cell whose
// corner 0 it is (where i < nx − 1, j < ny − 1, k < nz − 1) — the cells' linear order is the order of their corner 0 — and the three
// lattice edges that start at it.  So ONE pass in q order numbers the vertices (active cells) and the quads (edges whose ends
// differ, in axis order behind their point) as the definition orders them.
//   1. mesh_count_kernel: the share's active cells and quads → vOff[share], qOff[share]
//   2. mesh_scan_kernel: one workgroup turns both into exclusive offsets in place, carrying the totals from one round of 1024
//      shares to the next, and stores the totals in d_counts (the quads' in 64 bits, saturated at 2^32 − 1 where stored)
//   3. mesh_vertices_kernel: classifies again, numbers the share's active cells behind vOff[share] (ballot + popcount, a running
//      base per round), stores the vertices numbered below maxVertices and every active cell's number in cellVertex[cell]
//   4. mesh_quads_kernel: the same for the edges, reading the four cells' numbers from cellVertex (all four are active: each has
//      the edge's two ends among its corners)
// Steps 3 and 4 are left out of a counting call, step 4 where maxQuads = 0.  Workspace (kWsMesh, per device and stream, grow-only):
// 4 B per cell for cellVertex, 12 B per share of 1024 points for the offsets.
constexpr int kMeshRounds = 16, kMeshShare = 64 * kMeshRounds;

struct Lattice { const float *dist; int nx, ny, nz; float iso; };

// What point q of the lattice says: the inside mask of the cell's corners where the cell exists (else `cell` is false), and which of
// its three edges give a quad.  Corners outside the lattice are not read.
struct PointClass { float v[8]; unsigned mask; bool cell; bool quad[3]; int i, j, k; };
RM_DEV PointClass classify_point(const Lattice &L, unsigned q) {
  PointClass c;
  c.i = (int)(q % (unsigned)L.nx);
  const unsigned row = q / (unsigned)L.nx;
  c.j = (int)(row % (unsigned)L.ny);
  c.k = (int)(row / (unsigned)L.ny);
  const bool mx = c.i < L.nx - 1, my = c.j < L.ny - 1, mz = c.k < L.nz - 1;
  const size_t sy = (size_t)L.nx, sz = (size_t)L.nx * (size_t)L.ny;
#pragma unroll
  for (int n = 0; n < 8; n++) {
    const bool in = ((n & 1) == 0 || mx) && ((n & 2) == 0 || my) && ((n & 4) == 0 || mz);
    c.v[n] = in ? L.dist[(size_t)q + (size_t)(n & 1) + (size_t)((n >> 1) & 1) * sy + (size_t)((n >> 2) & 1) * sz] : 0.0f;
  }
  c.mask = sn::corner_mask(c.v, L.iso);
  c.cell = mx && my && mz;
  const bool p = (c.mask & 1u) != 0u;
#pragma unroll
  for (int a = 0; a < 3; a++)
    c.quad[a] = sn::edge_interior(a, c.i, c.j, c.k, L.nx, L.ny, L.nz) && (((c.mask >> (1 << a)) & 1u) != 0u) != p;
  return c;
}

__global__ __launch_bounds__(64) void mesh_count_kernel(Lattice L, unsigned numPoints, uint32_t *__restrict__ vOff,
                                                        unsigned long long *__restrict__ qOff) {
  unsigned nv = 0, nq = 0;  // wave-uniform
  for (int r = 0; r < kMeshRounds; r++) {
    const unsigned q = (blockIdx.x * kMeshRounds + r) * 64u + threadIdx.x;
    bool act = false, qa[3] = {false, false, false};
    if (q < numPoints) {
      const PointClass c = classify_point(L, q);
      act = c.cell && sn::cell_active(c.mask);
      for (int a = 0; a < 3; a++) qa[a] = c.quad[a];
    }
    nv += (unsigned)__popcll(__ballot(act));
    nq += (unsigned)(__popcll(__ballot(qa[0])) + __popcll(__ballot(qa[1])) + __popcll(__ballot(qa[2])));
  }
  if (threadIdx.x == 0) {
    vOff[blockIdx.x] = nv;
    qOff[blockIdx.x] = nq;
  }
}

__global__ __launch_bounds__(1024) void mesh_scan_kernel(uint32_t *__restrict__ vOff, unsigned long long *__restrict__ qOff, unsigned n,
                                                         uint32_t *__restrict__ counts) {
  __shared__ uint32_t waveV[16];
  __shared__ unsigned long long waveQ[16];
  uint32_t carryV = 0;  // the same in every lane; at most the number of cells, below 2^31
  unsigned long long carryQ = 0;
  for (unsigned base = 0; base < n; base += 1024u) {
    const unsigned i = base + threadIdx.x;
    ScanRound<uint32_t> v;
    ScanRound<unsigned long long> q;
    scan_round_1024(i < n ? vOff[i] : 0u, waveV, v, i < n ? qOff[i] : 0ull, waveQ, q);
    if (i < n) {
      vOff[i] = carryV + v.before;
      qOff[i] = carryQ + q.before;
    }
    carryV += v.all;
    carryQ += q.all;
  }
  if (threadIdx.x == 0) {
    counts[0] = carryV;
    counts[1] = carryQ > 0xffffffffull ? 0xffffffffu : (uint32_t)carryQ;
  }
}

__global__ __launch_bounds__(64) void mesh_vertices_kernel(Lattice L, const int32_t *__restrict__ objectId, unsigned numPoints, float ox,
                                                           float oy, float oz, float sx, float sy, float sz,
                                                           const uint32_t *__restrict__ vOff, int maxVertices,
                                                           float *__restrict__ vertices, int32_t *__restrict__ vertexObject,
                                                           int32_t *__restrict__ cellVertex) {
  unsigned base = vOff[blockIdx.x];  // wave-uniform
  for (int r = 0; r < kMeshRounds; r++) {
    const unsigned q = (blockIdx.x * kMeshRounds + r) * 64u + threadIdx.x;
    PointClass c;
    bool act = false;
    if (q < numPoints) {
      c = classify_point(L, q);
      act = c.cell && sn::cell_active(c.mask);
    }
    const unsigned long long ballot = __ballot(act);
    if (act) {
      const unsigned number = base + lanes_below(ballot, threadIdx.x);
      cellVertex[((size_t)c.k * (size_t)(L.ny - 1) + (size_t)c.j) * (size_t)(L.nx - 1) + (size_t)c.i] = (int32_t)number;
      if (number < (unsigned)maxVertices) {
        float local[3];
        sn::cell_vertex(c.v, L.iso, c.mask, local);
        float *o = vertices + 4 * (size_t)number;  // four words: the ABI asks no alignment of d_vertices beyond a float's
        o[0] = sn::vertex_world(ox, sx, c.i, local[0]);
        o[1] = sn::vertex_world(oy, sy, c.j, local[1]);
        o[2] = sn::vertex_world(oz, sz, c.k, local[2]);
        o[3] = 0.0f;
        if (vertexObject) {
          int32_t id = -1;
          if (objectId) {
            const int n = sn::first_inside_corner(c.mask);
            id = objectId[(size_t)q + (size_t)(n & 1) + (size_t)((n >> 1) & 1) * (size_t)L.nx +
                          (size_t)((n >> 2) & 1) * (size_t)L.nx * (size_t)L.ny];
          }
          vertexObject[number] = id;
        }
      }
    }
    base += (unsigned)__popcll(ballot);
  }
}

__global__ __launch_bounds__(64) void mesh_quads_kernel(Lattice L, unsigned numPoints, const unsigned long long *__restrict__ qOff,
                                                        int maxQuads, const int32_t *__restrict__ cellVertex, int32_t *__restrict__ quads) {
  unsigned long long base = qOff[blockIdx.x];  // wave-uniform
  for (int r = 0; r < kMeshRounds; r++) {
    const unsigned q = (blockIdx.x * kMeshRounds + r) * 64u + threadIdx.x;
    PointClass c;
    c.quad[0] = c.quad[1] = c.quad[2] = false;
    if (q < numPoints) c = classify_point(L, q);
    const unsigned long long b0 = __ballot(c.quad[0]), b1 = __ballot(c.quad[1]), b2 = __ballot(c.quad[2]);
    // the quads of the points before this one in the round, then this point's own, in axis order
    unsigned long long number = base + lanes_below(b0, threadIdx.x) + lanes_below(b1, threadIdx.x) + lanes_below(b2, threadIdx.x);
#pragma unroll
    for (int a = 0; a < 3; a++) {
      if (!c.quad[a]) continue;
      if (number < (unsigned long long)maxQuads) {
        int cells[4][3], vtx[4];
        sn::edge_cells(a, c.i, c.j, c.k, (c.mask & 1u) != 0u, cells);
#pragma unroll
        for (int n = 0; n < 4; n++)
          vtx[n] = cellVertex[((size_t)cells[n][2] * (size_t)(L.ny - 1) + (size_t)cells[n][1]) * (size_t)(L.nx - 1) + (size_t)cells[n][0]];
#pragma unroll
        for (int n = 0; n < 4; n++) quads[4 * (size_t)number + n] = vtx[n];
      }
      number++;
    }
    base += (unsigned long long)(__popcll(b0) + __popcll(b1) + __popcll(b2));
  }
}

// the workspace of a call: a vertex number per cell, the shares' quad and vertex offsets; measured where mem is null
struct MeshWs { int32_t *cellVertex; unsigned long long *qOff; uint32_t *vOff; size_t bytes; };
static MeshWs mesh_workspace(size_t cells, size_t shares, void *mem) {
  Carve c(mem);  // a braced list is evaluated left to right: the members' order is the layout
  return MeshWs{c.take<int32_t>(cells), c.take<unsigned long long>(shares), c.take<uint32_t>(shares), c.bytes()};
}

}  // namespace rm

using namespace rm;

extern "C" int rm_sdf_mesh(const float *d_dist, const int32_t *d_objectId, int nx, int ny, int nz, const float origin[3],
                           const float step[3], float iso, int maxVertices, int maxQuads, float *d_vertices, int32_t *d_vertexObject,
                           int32_t *d_quads, uint32_t *d_counts, void *stream) {
  auto bad = [](const char *msg) { set_error(msg); return (int)RM_ERR_INVALID_ARGUMENT; };
  if (int st = check_lattice(origin, step, nx, ny, nz)) return st;
  if (!std::isfinite(iso)) return bad("iso must be finite");
  if (maxVertices < 0 || maxQuads < 0) return bad("negative capacity");
  if ((maxVertices > 0 && !d_vertices) || (maxQuads > 0 && !d_quads)) return bad("null d_vertices or d_quads with a capacity above 0");
  if (!d_dist || !d_counts) return bad("null d_dist or d_counts");
  if (int st = require_device_pointers({{"d_dist", d_dist}, {"d_objectId", d_objectId}, {"d_vertices", d_vertices},
                                        {"d_vertexObject", d_vertexObject}, {"d_quads", d_quads}, {"d_counts", d_counts}}))
    return st;
  const hipStream_t hs = static_cast<hipStream_t>(stream);
  if (nx == 1 || ny == 1 || nz == 1) {  // no cell, so no vertex and no quad
    HIP_OK(hipMemsetAsync(d_counts, 0, 2 * sizeof(uint32_t), hs));
    return RM_OK;
  }
  const unsigned numPoints = (unsigned)((long long)nx * ny * nz), shares = (numPoints + kMeshShare - 1u) / kMeshShare;
  const size_t cells = (size_t)(nx - 1) * (size_t)(ny - 1) * (size_t)(nz - 1);
  // the workspace is in use until the last launch is enqueued: the device's launcher lock keeps rm_release_workspaces away
  std::unique_lock<std::mutex> lock;
  if (int st = lock_current_device(lock)) return st;
  void *mem = nullptr;
  if (int st = stream_workspace(kWsMesh, hs, mesh_workspace(cells, shares, nullptr).bytes, &mem)) return st;
  const MeshWs ws = mesh_workspace(cells, shares, mem);
  const Lattice L{d_dist, nx, ny, nz, iso};
  hipLaunchKernelGGL(mesh_count_kernel, dim3(shares), dim3(64), 0, hs, L, numPoints, ws.vOff, ws.qOff);
  hipLaunchKernelGGL(mesh_scan_kernel, dim3(1), dim3(1024), 0, hs, ws.vOff, ws.qOff, shares, d_counts);
  if (maxVertices > 0 || maxQuads > 0)
    hipLaunchKernelGGL(mesh_vertices_kernel, dim3(shares), dim3(64), 0, hs, L, d_objectId, numPoints, origin[0], origin[1], origin[2],
                       step[0], step[1], step[2], ws.vOff, maxVertices, d_vertices, d_vertexObject, ws.cellVertex);
  if (maxQuads > 0)
    hipLaunchKernelGGL(mesh_quads_kernel, dim3(shares), dim3(64), 0, hs, L, numPoints, ws.qOff, maxQuads, ws.cellVertex,
                       d_quads);
  HIP_OK(hipGetLastError());
  return RM_OK;
}
