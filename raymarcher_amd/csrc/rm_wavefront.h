// rm_wavefront.h — what the host sees of the wavefront pipeline (rm_wavefront.hip.h has the kernels and the design): its bounce
// limit, the counters of a generation, the register budgets and chunk sizes the launcher sizes its launches by.  Plain C++, no device
// code; the records of the pipeline's workspace (WfWs) are in rm_launch.h.
#pragma once
#include <cstdint>

namespace rm {

constexpr int kWfMaxBounces = 7;
enum { WF_SRC = 0, WF_HITS = 1, WF_SHADOW = 2, WF_NEXT = 3, WF_STRIDE = 8 };  // counters of one generation

// Register budgets (waves per SIMD) of the march kernels: the shadow kernel fits 64 VGPRs; the primary / bounce kernels carry
// the ray set-up of their refill path (primaryRay's IEEE divisions) and spill 15 / 5 registers at that budget.
#ifndef RM_WF_MARCH_WAVES
#define RM_WF_MARCH_WAVES 8
#endif
#ifndef RM_WF_PRIMARY_WAVES
#define RM_WF_PRIMARY_WAVES 6
#endif
constexpr int wfMarchWaves(int kind) { return kind == 2 ? RM_WF_MARCH_WAVES : RM_WF_PRIMARY_WAVES; }
// Cursor granularity.  One device counter sustains ≈88 atomics per µs (measured in round 1): with 64-slot hit chunks the 20 M
// primary hits of the 8K Menger frame were 311 k atomics ≈ 3.5 ms of a 5.0 ms kernel (the bounce kernels likewise), so hit
// slots, rays and pixels are reserved 256 at a time (a wave's unused remainder becomes holes; 64 was atomic-bound, 1024 and
// guided chunks measured slower: profiles/r03_b_wavefront.md).
#ifndef RM_WF_SLOT_CHUNK
#define RM_WF_SLOT_CHUNK 256
#endif
#ifndef RM_WF_RAY_CHUNK
#define RM_WF_RAY_CHUNK 256
#endif
#ifndef RM_WF_PIXEL_CHUNK
#define RM_WF_PIXEL_CHUNK 256
#endif
constexpr uint32_t kWfSlotChunk = RM_WF_SLOT_CHUNK;
constexpr uint32_t kWfStripes = 64;  // power of two
constexpr uint32_t wfRayChunk(int kind) { return kind == 0 ? RM_WF_PIXEL_CHUNK : RM_WF_RAY_CHUNK; }

}  // namespace rm
