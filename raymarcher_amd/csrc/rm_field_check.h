// rm_field_check.h — the host checks that rm_field.hip (rm_sdf_sample / rm_sdf_trace and their block forms) and rm_field_handle.hip
// (RmField handles) have in common, each once: the records' sizes and codes, the dense or block-sparse lattice, the march's
// parameters, the lattice's arrays.  Host only, no HIP call: a caller's "no HIP call ahead of the last check" holds through them.
// What differs between the two units — the accepted mode bits, the texts that name a call's own arrays — is an argument.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/raymarcher_amd.h"
#include "rm_field_march.h"
#include "rm_internal.h"

namespace rm {
namespace fchk {

static_assert(sizeof(fm::Sample) == 32 && sizeof(RmFieldSample) == 32 && sizeof(fm::Hit) == 32 && sizeof(RmRayHit) == 32, "two float4 per record");
static_assert(fm::kInvalid == RM_RAY_INVALID && fm::kOutside == RM_FIELD_OUTSIDE && fm::kUnlisted == RM_FIELD_UNLISTED, "the header's codes");

inline bool aligned(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
inline int bad(const char *msg) {
  set_error(msg);
  return (int)RM_ERR_INVALID_ARGUMENT;
}

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

// The lattice's arrays, and (rm_field.hip; null, null from a create) the call's own 16-byte arrays `in` and `out`, whose alignment
// is part of the same rule: d_dist may be null only behind an empty list, of which nothing is read; d_blocks only with numBlocks
// = 0; then the alignment of all of them.  nullText and alignText name the arrays of the call.
inline int check_field_arrays(const void *in, const void *out, const float *dist, const int32_t *ids, const int32_t *blocks, int numBlocks,
                              bool sparse, const char *nullText, const char *alignText) {
  const bool emptyList = sparse && numBlocks == 0;
  if (!dist && !emptyList) return bad(nullText);
  if (sparse && numBlocks > 0 && !blocks) return bad("null d_blocks with numBlocks above 0");
  if (!aligned(in, 16) || !aligned(out, 16) || !aligned(dist, 4) || !aligned(ids, 4) || !aligned(blocks, 4)) return bad(alignText);
  return RM_OK;
}

}  // namespace fchk
}  // namespace rm
