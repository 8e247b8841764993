// rm_compact.hip.h — what the compaction kernels share (rm_volume.hip, rm_blocks.hip, rm_order.hip): a lane's rank within a ballot
// and one round of a 1024-lane workgroup's exclusive scan.  Integers only, so the results are exact; no other header is needed.
#pragma once
#include <hip/hip_runtime.h>

namespace rm {

// how many lanes below `lane` are set in the ballot
__device__ __forceinline__ unsigned lanes_below(unsigned long long ballot, unsigned lane) { return (unsigned)__popcll(ballot & ((1ull << lane) - 1ull)); }

// One round of the scan of a workgroup of 1024 lanes, all of which call it: `before` is the sum of the values of the lanes below
// this one, `all` the sum of the 1024 values (the same in every lane).  waveSum is the kernel's own LDS array of 16 words; the
// round ends with a barrier behind its last read, so the next round may use the array again at once.  A kernel that scans more
// than 1024 values carries `all` from round to round itself.  The second form scans two sequences behind the same two barriers.
template <class T> struct ScanRound { T before, all; };
namespace detail {  // the two halves of a round; kernels call scan_round_1024 only
template <class T> __device__ __forceinline__ T scan_publish_wave(T v, T *waveSum) {  // → inclusive within the wave; the wave's sum into waveSum
  const unsigned lane = threadIdx.x & 63u;
  T s = v;
  for (unsigned d = 1; d < 64u; d <<= 1) {
    const T t = __shfl_up(s, d);
    if (lane >= d) s += t;
  }
  if (lane == 63u) waveSum[threadIdx.x >> 6] = s;
  return s;
}
template <class T> __device__ __forceinline__ ScanRound<T> scan_across_waves(T v, T inclusive, const T *waveSum) {
  const unsigned wave = threadIdx.x >> 6;
  T before = 0, all = 0;
  for (unsigned w = 0; w < 16u; w++) {
    if (w < wave) before += waveSum[w];
    all += waveSum[w];
  }
  return ScanRound<T>{before + inclusive - v, all};
}
}  // namespace detail
template <class T> __device__ __forceinline__ ScanRound<T> scan_round_1024(T v, T *waveSum) {
  const T s = detail::scan_publish_wave(v, waveSum);
  __syncthreads();
  const ScanRound<T> r = detail::scan_across_waves(v, s, waveSum);
  __syncthreads();
  return r;
}
template <class A, class B> __device__ __forceinline__ void scan_round_1024(A a, A *waveA, ScanRound<A> &ra, B b, B *waveB, ScanRound<B> &rb) {
  const A sa = detail::scan_publish_wave(a, waveA);
  const B sb = detail::scan_publish_wave(b, waveB);
  __syncthreads();
  ra = detail::scan_across_waves(a, sa, waveA);
  rb = detail::scan_across_waves(b, sb, waveB);
  __syncthreads();
}

}  // namespace rm
