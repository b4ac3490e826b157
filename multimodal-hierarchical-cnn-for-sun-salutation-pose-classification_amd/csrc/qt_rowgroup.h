// Row-group helpers: LANES lanes of a wave own one row of a [rows][C] matrix, element k sits in lane k % LANES.  These are
// the helpers loss.hip and metrics.hip each keep in their own anonymous namespace (same arithmetic, same order), in one
// place for the stages that come after them: a stage that includes this header and walks a row as metrics.hip's
// metrics_logits_kernel does (per-lane sums over j ascending, then qt_group_sum) forms the softmax with the very bits
// qt_metrics_update writes to probs.
#pragma once
#include "qt_common.h"

// sum over the LANES lanes of a row, every lane receives it: qt_row16_sum inside a DPP row, then two wave shuffles
template <int LANES> __device__ __forceinline__ float qt_group_sum(float v) {
  if (LANES >= 16) v = qt_row16_sum(v);
  if (LANES == 64) {
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
  }
  return v;
}
// the loss head's total order: a NaN beats every number, then the larger value, then the lower index
__device__ __forceinline__ bool qt_arg_beats(float av, int ai, float bv, int bi) {
  const bool an = av != av, bn = bv != bv;
  if (an != bn) return an;
  if (!an && av != bv) return av > bv;
  return ai < bi;
}
// the winner of that order over the LANES lanes, in every lane; the value travels with its index
template <int LANES> __device__ __forceinline__ void qt_group_argmax(float& v, int& i) {
#pragma unroll
  for (int s = 1; s < LANES; s <<= 1) {
    const float ov = __shfl_xor(v, s, 64);
    const int oi = __shfl_xor(i, s, 64);
    if (qt_arg_beats(ov, oi, v, i)) {
      v = ov;
      i = oi;
    }
  }
}
// the value of lane `owner` (0 .. LANES - 1) of the calling lane's group
template <int LANES> __device__ __forceinline__ float qt_group_pick(float v, int owner) {
  if (LANES == 1) return v;
  return __shfl(v, (int)((threadIdx.x & 63u) & ~(unsigned)(LANES - 1)) + owner, 64);
}
// integer sum over the group (any order gives the same integer)
template <int LANES> __device__ __forceinline__ int qt_group_sum_int(int v) {
#pragma unroll
  for (int s = 1; s < LANES; s <<= 1) v += __shfl_xor(v, s, 64);
  return v;
}
// true in every lane of the group when any of its lanes passes true.  Every lane of the wave must call it.
template <int LANES> __device__ __forceinline__ bool qt_group_any(bool v) {
  static_assert(LANES == 1 || LANES == 16 || LANES == 32, "a group is part of a wave");
  if (LANES == 1) return v;
  const unsigned long long b = __ballot(v);
  const unsigned first = (threadIdx.x & 63u) & ~(unsigned)(LANES - 1);
  return ((b >> first) & ((1ull << LANES) - 1ull)) != 0ull;
}
