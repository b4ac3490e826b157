// Row groups: LANES lanes of a wave own one row of a [rows][C] matrix, lane `sub` of the group keeps PER elements in
// registers, element k = j * LANES + sub sits in z[j].  This header is the ONE definition of that walk for loss.hip,
// metrics.hip, scores.hip and timeline.hip: the lane rule, the row load, the argmax in the loss head's total order and the
// softmax.  What the files promise each other (the same class on ties and NaN rows, a softmax with the very bits
// qt_metrics_update writes to probs, one integer confidence) holds because they all call these functions; a kernel that wants
// those bits uses qt_row_load, qt_row_argmax and qt_row_softmax and nothing of its own in their place.
// Every lane of the wave must call the group functions (DPP, shuffles and ballots inside).
#pragma once
#include <math.h>

#include "qt_common.h"

// ---- the lane rule ------------------------------------------------------------------------------------------------------
//     C <= 16    one thread per row, 16 elements per lane
//     C <= 64    one 16-lane DPP row per row, 4 per lane
//     C <= 1024  one wave per row, 16 per lane
static inline int qt_row_lanes(int C) { return C <= 16 ? 1 : C <= 64 ? 16 : 64; }
// f(LANES, PER) for C classes, both as std::integral_constant<int, ..>; a caller whose MAX_C is at most 64 never
// instantiates the wave-per-row arm:
//   qt_by_row_lanes<MAX_C>(C, [&](auto L, auto P) { hipLaunchKernelGGL((k<L(), P()>), ...); });
template <int MAX_C, typename F>
static inline auto qt_by_row_lanes(int C, F&& f) {
  const int lanes = qt_row_lanes(C);
  if (lanes == 1) return f(std::integral_constant<int, 1>{}, std::integral_constant<int, 16>{});
  if constexpr (MAX_C > 64)
    if (lanes == 64) return f(std::integral_constant<int, 64>{}, std::integral_constant<int, 16>{});
  return f(std::integral_constant<int, 16>{}, std::integral_constant<int, 4>{});
}

// ---- over the LANES lanes of a group ------------------------------------------------------------------------------------
// sum, every lane receives it: qt_row16_sum inside a DPP row, then two wave shuffles
template <int LANES> __device__ __forceinline__ float qt_group_sum(float v) {
  if (LANES >= 16) v = qt_row16_sum(v);
  if (LANES == 64) {
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
  }
  return v;
}
// the total order of every argmax here: a NaN beats every number, then the larger value, then the lower index
__device__ __forceinline__ bool qt_arg_beats(float av, int ai, float bv, int bi) {
  const bool an = av != av, bn = bv != bv;
  if (an != bn) return an;
  if (!an && av != bv) return av > bv;
  return ai < bi;
}
template <int CTRL> __device__ __forceinline__ void qt_arg_dpp(float& v, int& i) {
  const float ov = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
  const int oi = __builtin_amdgcn_update_dpp(0, i, CTRL, 0xf, 0xf, false);
  if (qt_arg_beats(ov, oi, v, i)) {
    v = ov;
    i = oi;
  }
}
// the winner of that order, in every lane; the value travels with its index.  The order is total, so any tree gives the
// same pair: the four DPP steps of qt_row16_sum inside a 16-lane row (no LDS crossbar), then two wave shuffles for LANES == 64
template <int LANES> __device__ __forceinline__ void qt_group_argmax(float& v, int& i) {
  static_assert(LANES == 1 || LANES == 16 || LANES == 64, "one lane, one DPP row or one wave");
  if constexpr (LANES >= 16) {
    qt_arg_dpp<0x140>(v, i);   // row_mirror
    qt_arg_dpp<0x141>(v, i);   // row_half_mirror
    qt_arg_dpp<0x1b>(v, i);    // quad_perm [3,2,1,0]
    qt_arg_dpp<0xb1>(v, i);    // quad_perm [1,0,3,2]
  }
  if constexpr (LANES == 64) {
#pragma unroll
    for (int s = 16; s < 64; s <<= 1) {
      const float ov = __shfl_xor(v, s, 64);
      const int oi = __shfl_xor(i, s, 64);
      if (qt_arg_beats(ov, oi, v, i)) {
        v = ov;
        i = oi;
      }
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
// true in every lane of the group when any of its lanes passes true
template <int LANES> __device__ __forceinline__ bool qt_group_any(bool v) {
  static_assert(LANES == 1 || LANES == 16 || LANES == 32, "a group is part of a wave");
  if (LANES == 1) return v;
  const unsigned long long b = __ballot(v);
  const unsigned first = (threadIdx.x & 63u) & ~(unsigned)(LANES - 1);
  return ((b >> first) & ((1ull << LANES) - 1ull)) != 0ull;
}

// ---- the row walk -------------------------------------------------------------------------------------------------------
// this lane's PER elements of the row at zr; elements past C read as 0
template <int LANES, int PER> __device__ __forceinline__ void qt_row_load(const float* __restrict__ zr, int C, int sub, float (&z)[PER]) {
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int k = j * LANES + sub;
    z[j] = k < C ? zr[k] : 0.f;
  }
}
// argmax = torch.max(outputs, 1) in qt_arg_beats' order: first index of the maximum, a NaN wins.  Lanes that own no element
// enter with (-inf, INT32_MAX), which beats nothing.  Every lane receives (z[argmax], argmax).
template <int LANES, int PER> __device__ __forceinline__ void qt_row_argmax(const float (&z)[PER], int C, int sub, float& bv, int& bi) {
  bv = z[0];
  bi = sub;
  if (sub >= C) { bv = -INFINITY; bi = INT32_MAX; }
#pragma unroll
  for (int j = 1; j < PER; ++j) {
    const int k = j * LANES + sub;
    if (k < C && qt_arg_beats(z[j], k, bv, bi)) { bv = z[j]; bi = k; }
  }
  qt_group_argmax<LANES>(bv, bi);
}
// softmax in place, m = z[argmax]: e_k = expf(z_k - m), per-lane sums with j ascending, the group sum, p_k = e_k / s (a true
// division).  Elements past C are left as they are.  A NaN or +inf logit (and a row of -inf) makes m or z_k - m NaN, so the
// whole row is NaN by IEEE rules, which is what torch.softmax gives on the CPU.
template <int LANES, int PER> __device__ __forceinline__ void qt_row_softmax(float (&z)[PER], int C, int sub, float m) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int k = j * LANES + sub;
    if (k < C) {
      z[j] = expf(z[j] - m);
      s += z[j];
    }
  }
  s = qt_group_sum<LANES>(s);
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int k = j * LANES + sub;
    if (k < C) z[j] = z[j] / s;
  }
}

// ---- what the evaluation kernels share beside the walk ------------------------------------------------------------------
// Sum of one double per thread over a workgroup of THREADS, fixed order (thread t adds slot t + s for s = THREADS / 2 .. 1),
// every thread receives it.  `red`: THREADS doubles of LDS.
template <int THREADS> __device__ __forceinline__ double qt_block_sum(double v, double* red) {
  const int t = threadIdx.x;
  __syncthreads();   // the previous call's readers are done
  red[t] = v;
  __syncthreads();
#pragma unroll
  for (int s = THREADS / 2; s >= 1; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  return red[0];
}
// the row counters cnt[0 .. N) in LDS by a row's class `cls` (a lane that counts nothing passes N or more): one ballot and
// one LDS atomic per wave and class
template <int N> __device__ __forceinline__ void qt_count_rows(int cls, unsigned* cnt) {
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const unsigned long long b = __ballot(cls == k);
    if ((threadIdx.x & 63u) == 0 && b) atomicAdd(&cnt[k], (unsigned)__popcll(b));
  }
}
// the integer confidence of the timeline's segments and of the calibration bins: q(x) = rint(clamp(x, 0, 1) * 65536),
// q(NaN) = 0; the product is exact, so is its rounding
__device__ __forceinline__ int qt_conf_q(float x) {
  if (x != x) return 0;
  return (int)rintf(fminf(fmaxf(x, 0.f), 1.f) * 65536.0f);
}

// ---- host: what the entry points ask of rows and classes ----------------------------------------------------------------
static inline int qt_check_class_cap(const char* who, int C, int max_C) {
  if (C > max_C) {
    qt_set_error("%s: C = %d classes; at most %d are handled", who, C, max_C);
    return QT_ERR_UNSUPPORTED;
  }
  return QT_OK;
}
// max_rows == 0: no cap on the rows of one call
static inline int qt_check_rows_classes(const char* who, long long rows, int C, int max_C, long long max_rows) {
  QT_CHECK_ARG(rows >= 1 && C >= 1, "%s: needs rows >= 1 and C >= 1 (got %lld x %d)", who, rows, C);
  if (int rc = qt_check_class_cap(who, C, max_C)) return rc;
  if (max_rows && rows > max_rows) {
    qt_set_error("%s: %lld rows; at most %lld are handled in one call", who, rows, max_rows);
    return QT_ERR_UNSUPPORTED;
  }
  return QT_OK;
}
