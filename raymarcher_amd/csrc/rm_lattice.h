// rm_lattice.h — the host side of the lattice family: rm_sdf_grid and rm_sdf_mesh (rm_volume.hip), the block-sparse forms
// rm_sdf_blocks_select, rm_sdf_blocks_select_pruned, rm_sdf_grid_blocks and rm_sdf_mesh_blocks (rm_blocks.hip), the lattice queries
// and the RmField handles (rm_field.hip).  The argument checks the entry points have in common, each once and host only with no
// HIP call — a caller's "no HIP call ahead of the last check" holds through them —, and what the units call of one another and
// rm_queries.hip, which checks and stages the scene entries, calls of them.  include/raymarcher_amd.h has the definitions.
#pragma once
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/raymarcher_amd.h"
#include "rm_internal.h"

namespace rm {

// ---- the checks -------------------------------------------------------------------------------------------------------------------
namespace fchk {
inline bool aligned(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
inline int bad(const char *msg) { set_error(msg); return (int)RM_ERR_INVALID_ARGUMENT; }
// origin and step of either kind of lattice
inline int check_frame(const float *origin, const float *step) {
  if (!origin || !step) return bad("null origin or step");
  for (int a = 0; a < 3; a++)
    if (!std::isfinite(origin[a])) return bad("origin must be finite");
  for (int a = 0; a < 3; a++)
    if (!std::isfinite(step[a]) || !(step[a] > 0.0f)) return bad("step must be finite and greater than 0 on every axis");
  return RM_OK;
}
}  // namespace fchk

// The lattice rules that rm_sdf_grid, rm_sdf_mesh and the dense queries share, in the header's order.
inline int check_lattice(const float *origin, const float *step, int nx, int ny, int nz) {
  if (int st = fchk::check_frame(origin, step)) return st;
  if (nx < 1 || ny < 1 || nz < 1 || nx > RM_MAX_LATTICE_DIM || ny > RM_MAX_LATTICE_DIM || nz > RM_MAX_LATTICE_DIM)
    return fchk::bad("every lattice dimension must be 1 … RM_MAX_LATTICE_DIM (4096)");
  if ((long long)nx * ny * nz > INT_MAX) return fchk::bad("more than INT_MAX lattice points");
  return RM_OK;
}
// The rules the block-sparse entry points share for origin, step and the block dimensions, in the header's order.
inline int check_block_lattice(const float *origin, const float *step, int mx, int my, int mz) {
  if (int st = fchk::check_frame(origin, step)) return st;
  if (mx < 1 || my < 1 || mz < 1 || mx > RM_MAX_LATTICE_BLOCKS || my > RM_MAX_LATTICE_BLOCKS || mz > RM_MAX_LATTICE_BLOCKS)
    return fchk::bad("every block dimension must be 1 … RM_MAX_LATTICE_BLOCKS (512)");
  return RM_OK;
}

// What the lattice queries and the handles have in common; what differs between them — the accepted mode bits, the texts that
// name a call's own arrays — is an argument.
namespace fchk {
// The lattice of a call: block-sparse (dims = m; check_block_lattice, then the list's length) or dense (dims = n; check_lattice,
// then a cell along every axis).  A dense call has numBlocks = −1.
inline int check_field_lattice(bool sparse, const int dims[3], const float *origin, const float *step, int numBlocks) {
  if (sparse) {
    if (int st = check_block_lattice(origin, step, dims[0], dims[1], dims[2])) return st;
    if (numBlocks < 0 || numBlocks > RM_MAX_BLOCK_LIST) return bad("numBlocks must be 0 … RM_MAX_BLOCK_LIST");
    return RM_OK;
  }
  if (int st = check_lattice(origin, step, dims[0], dims[1], dims[2])) return st;
  if (dims[0] < 2 || dims[1] < 2 || dims[2] < 2) return bad("every lattice dimension must be at least 2: a query needs a cell");
  return RM_OK;
}

// The parameters of a march.  modes: the mode bits the entry point accepts, modesText its refusal of any other.  NO_NORMAL with
// OCCLUSION is refused wherever OCCLUSION is a mode (elsewhere the bits' check has refused it).
inline int check_field_march(float iso, int maxSteps, unsigned mode, unsigned modes, const char *modesText) {
  if (!std::isfinite(iso)) return bad("iso must be finite");
  if (maxSteps < 0 || maxSteps > RM_MAX_FIELD_STEPS) return bad("maxSteps must be 0 … RM_MAX_FIELD_STEPS (65536)");
  if ((mode & ~modes) != 0u) return bad(modesText);
  if ((mode & RM_TRACE_NO_NORMAL) && (mode & RM_TRACE_OCCLUSION))
    return bad("RM_TRACE_NO_NORMAL is a flag on RM_TRACE_CLOSEST: occlusion stores no normal anyway");
  return RM_OK;
}

// The lattice's arrays, and (null, null from a create) the call's own 16-byte arrays `in` and `out`, whose alignment is part of the
// same rule: d_dist may be null only behind an empty list, of which nothing is read; d_blocks only with numBlocks = 0; then the
// alignment of all of them.  nullText and alignText name the arrays of the call.
inline int check_field_arrays(const void *in, const void *out, const float *dist, const int32_t *ids, const int32_t *blocks, int numBlocks,
                              bool sparse, const char *nullText, const char *alignText) {
  const bool emptyList = sparse && numBlocks == 0;
  if (!dist && !emptyList) return bad(nullText);
  if (sparse && numBlocks > 0 && !blocks) return bad("null d_blocks with numBlocks above 0");
  if (!aligned(in, 16) || !aligned(out, 16) || !aligned(dist, 4) || !aligned(ids, 4) || !aligned(blocks, 4)) return bad(alignText);
  return RM_OK;
}
}  // namespace fchk

// ---- the launches, arguments already checked, `sb` the ONE staged SceneBlock (device pointer) ----------------------------------------
// rm_volume.hip: sdf_grid_kernel<bulbClass>, one lane per lattice point, a wave per brick — nx·ny·nz values into d_dist and, when
// d_objectId is not null, as many object indices.
int launch_sdf_grid_kernel(const void *sb, int bulbClass, const float origin[3], const float step[3], int nx, int ny, int nz,
                           float *d_dist, int32_t *d_objectId, hipStream_t stream);
// rm_blocks.hip.  Every launch takes a `workspace` of as many bytes as the function named after it returns.
// select: blocks_eval_kernel<bulbClass, select>, a workgroup per block of the virtual lattice, then the compaction of the active
// flags into d_blocks and d_count.  prune (rm_sdf_blocks_select_pruned): the corner lattice, the classification, the candidates'
// exact evaluation and the same compaction; the candidates' number goes into d_count[1].  grid: the block map of the list, then
// blocks_eval_kernel<bulbClass, grid>, a workgroup per entry — 729 values per entry that is not void into d_dist and, when
// d_objectId is not null, as many object indices; its workspace is the block map's: take_block_map's lines, alone or at the head of
// a larger layout, so whoever sizes the map and whoever points into it read the same description.
inline uint32_t *take_block_map(Carve &c, int mx, int my, int mz) { return c.take<uint32_t>((size_t)mx * (size_t)my * (size_t)mz); }
inline size_t blocks_map_workspace(int mx, int my, int mz) { Carve c; take_block_map(c, mx, my, mz); return c.bytes(); }
size_t blocks_select_workspace(int mx, int my, int mz);
size_t blocks_prune_workspace(int mx, int my, int mz);
int launch_blocks_select_kernels(const void *sb, int bulbClass, const float origin[3], const float step[3], int mx, int my, int mz, float iso,
                                 int maxBlocks, int32_t *d_blocks, uint32_t *d_count, void *workspace, hipStream_t stream);
int launch_blocks_prune_kernels(const void *sb, int bulbClass, const float origin[3], const float step[3], int mx, int my, int mz, float iso,
                                float lipschitzOut, float lipschitzIn, int maxBlocks, int32_t *d_blocks, uint32_t *d_count, void *workspace,
                                hipStream_t stream);
int launch_blocks_grid_kernels(const void *sb, int bulbClass, const float origin[3], const float step[3], int mx, int my, int mz,
                               const int32_t *d_blocks, int numBlocks, float *d_dist, int32_t *d_objectId, void *workspace, hipStream_t stream);
// The block map of a list, blocks_map_workspace bytes at `first`: first[block] = the smallest list position that names the block,
// all bits set where none does.  An empty list (numBlocks = 0, d_blocks is not read) lists no block.
int enqueue_block_map(const int32_t *d_blocks, int numBlocks, int mx, int my, int mz, uint32_t *first, hipStream_t stream);

}  // namespace rm
