// What the kernels of the chain with hold durations share, on top of pose_chain.h (pose_duration.hip: the best path;
// pose_duration_lag.hip: its fixed-lag form; pose_duration_sweep.h: the forward-backward that pose_duration_posterior.hip and
// pose_duration_prior.hip run; pose_duration_lag_posterior.hip: its fixed-lag form): the table's width and the descriptor checks, the chain's inputs with the duration tables as one
// kernel-argument struct, and the walk of one workgroup of PC_DUR_THREADS per stream: the lane map with a state's slices of dur
// and dur_open in registers, the staging of trans, the start scores, a stream's length, the (max, +) step over the
// predecessors, the emissions staged PC_DUR_CHUNK frames at a time, the ring of the last D frames and the loop over a lane's
// own lengths; on the host the seven inputs as a checked list and the launch of a stream kernel with its LDS limit.
#pragma once
#include <limits.h>

#include "pose_chain.h"

constexpr int PC_MAX_D = 128;
constexpr int PC_DUR_THREADS = 256;
constexpr int PC_DUR_CHUNK = 64;                 // frames of emissions staged at a time
template <bool SMALL>
constexpr int PC_DUR_LPS = SMALL ? 16 : 4;       // lanes per state: lane l of a group has the lengths d = 1 + l + k LPS
static_assert(PC_MAX_D == QT_POSE_DUR_MAX, "the header states this");
static_assert(PC_MAX_D <= PC_DUR_THREADS && PC_MAX_D <= 128 && PC_MAX_S <= 64, "a segment's frames go across the lanes; 7 + 6 bits");
static_assert((PC_DUR_CHUNK & (PC_DUR_CHUNK - 1)) == 0 && PC_MAX_D % 16 == 0, "chunk masks; lengths per lane");
static_assert(PC_MAX_S * PC_DUR_LPS<false> <= PC_DUR_THREADS && 16 * PC_DUR_LPS<true> <= PC_DUR_THREADS, "a group per state");

// the chain's inputs with the duration tables: the head of the stream kernels' argument structs (tiles: not read)
struct PcDurChain : PcChain {
  const int* dur;
  const int* dur_open;         // never null: dur where the caller gave none
  const int* lengths;          // null: every stream has T frames (and in the fixed-lag decoder, which has no lengths)
  int D;
};
inline void pc_dur_fill(PcDurChain& a, const float* probs, long long ld, const int* state_class, const int* trans, const int* init,
                        const int* dur, const int* dur_open, const int* lengths, int T, int C, int S, int D) {
  pc_fill(a, probs, ld, state_class, trans, init, T, C, S);
  a.dur = dur;
  a.dur_open = dur_open ? dur_open : dur;
  a.lengths = lengths;
  a.D = D;
}

// a thread's place in the walk: group j of LPS lanes serves state jj, lane l of it the lengths d = 1 + l + k LPS, whose scores
// du[k] (dur) and dop[k] (dur_open) it keeps in registers
template <int LPS>
struct PcDurLane {
  static constexpr int KMAX = PC_MAX_D / LPS;    // lengths per lane
  int j, l, jj;
  bool own;                                      // (groups beyond S compute on state S - 1 and store nothing)
  int du[KMAX], dop[KMAX];
  __device__ __forceinline__ PcDurLane(int tid, int S, int D, const int* __restrict__ dur, const int* __restrict__ dur_open) {
    j = tid / LPS, l = tid - j * LPS, jj = min(j, S - 1);
    own = l == 0 && j < S;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      const int d0 = l + k * LPS;
      du[k] = d0 < D ? pc_clamp_trans(dur[jj * D + d0]) : 0;
      dop[k] = d0 < D ? pc_clamp_trans(dur_open[jj * D + d0]) : 0;
    }
  }
};

// f(k, d) for the lane's own lengths d = 1 + l + k LPS <= dmax, ascending; k indexes its register tables (KMAX of them)
template <int LPS, int KMAX = PC_MAX_D / LPS, typename F>
__device__ __forceinline__ void pc_for_lengths(int dmax, int l, F&& f) {
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    if (k * LPS >= dmax) break;                  // (uniform)
    const int d = 1 + l + k * LPS;
    if (d <= dmax) f(k, d);
  }
}
// the ring [D][S] of the last D frames, row f mod D: the row after and before `row`, the row d <= D behind it, and a row
// index that is off by less than D to either side
__device__ __forceinline__ int pc_ring_next(int row, int D) { return row + 1 == D ? 0 : row + 1; }
__device__ __forceinline__ int pc_ring_prev(int row, int D) { return row == 0 ? D - 1 : row - 1; }
__device__ __forceinline__ int pc_ring_behind(int row, int d, int D) { return row - d + (row - d < 0 ? D : 0); }
__device__ __forceinline__ int pc_ring_wrap(int r, int D) { return r + (r < 0 ? D : (r >= D ? -D : 0)); }

__device__ __forceinline__ void pc_stage_trans(const int* __restrict__ trans, int* tr, int S) {
  for (int idx = threadIdx.x; idx < S * S; idx += PC_DUR_THREADS) tr[idx] = pc_clamp_trans(trans[idx]);
}
__device__ __forceinline__ int pc_init_score(const int* init, int s) { return init ? pc_clamp_trans(init[s]) : 0; }
// the frames of stream b: lengths[b] clamped into 1 .. T
__device__ __forceinline__ int pc_stream_length(const int* lengths, int b, int T) {
  return lengths ? min(max(lengths[b], 1), T) : T;
}

// (value, index) of the maximum over a group of LPS adjacent lanes, the lower index at equal values; every lane receives it
template <int LPS>
__device__ __forceinline__ void pc_group_max(long long& v, int& k) {
#pragma unroll
  for (int s = 1; s < LPS; s <<= 1) {
    const long long ov = __shfl_xor(v, s, QT_WAVE);
    const int ok = __shfl_xor(k, s, QT_WAVE);
    if (ov > v || (ov == v && ok < k)) v = ov, k = ok;
  }
}
// (B) of the Viterbi walks: max_i (alpha[i] + trans[i][jj]) and the lowest i that attains it, over the group's lanes (the
// pair lives in locals until the end: as reference parameters they cost the fixed-lag kernel moves or registers)
template <int LPS>
__device__ __forceinline__ long long pc_dur_step_in(const long long* alpha, const int* tr, int S, int l, int jj, int& from) {
  long long best = LLONG_MIN;
  int at = INT_MAX;
  for (int i = l; i < S; i += LPS) {
    const long long v = alpha[i] + tr[i * S + jj];
    if (v > best) best = v, at = i;
  }
  pc_group_max<LPS>(best, at);
  from = at;
  return best;
}

// the staged emissions of frame g of the call's n frames, [S] shorts of e_l [PC_DUR_CHUNK][S].  fresh: g's chunk is staged
// first, behind a barrier of its own (the chunk before was last read two barriers ago)
__device__ __forceinline__ bool pc_chunk_start(int g) { return (g & (PC_DUR_CHUNK - 1)) == 0; }
__device__ __forceinline__ const short* pc_chunk_row(const PcChain& a, int b, int g, int n, short* e_l, bool fresh) {
  if (fresh) {
    const int g0 = g & ~(PC_DUR_CHUNK - 1);
    pc_stage_emissions(a, b, g0, min(PC_DUR_CHUNK, n - g0), e_l);
    __syncthreads();
  }
  return e_l + (g & (PC_DUR_CHUNK - 1)) * a.S;
}

// ---- host -------------------------------------------------------------------------------------------------------------------
inline int pc_duration_check_desc(const char* who, const qt_pose_duration_desc* d) {
  QT_CHECK_ARG(d != nullptr, "%s: null descriptor", who);
  const qt_pose_order_desc chain = {d->batch, d->frames, d->num_classes, d->num_states};
  if (const int rc = pc_check_desc(who, &chain)) return rc;
  QT_CHECK_ARG(d->max_duration >= 1 && d->max_duration <= PC_MAX_D, "%s: max_duration = %d; 1 .. %d are handled", who,
               d->max_duration, PC_MAX_D);
  return QT_OK;
}

// the fixed-lag decoder with hold durations (pose_duration_lag.hip): the fixed-lag pair's descriptor with the table's width;
// the scores are absolute int64, which bounds the frames of a stream
constexpr long long PC_DUR_LAG_MAX_SEEN = 1LL << 36;
inline qt_pose_lag_desc pc_duration_lag_as_lag(const qt_pose_duration_lag_desc* d) {
  return {d->batch, d->frames, d->num_classes, d->num_states, d->lag, d->flush, d->seen};
}
inline int pc_duration_lag_check_desc(const char* who, const qt_pose_duration_lag_desc* d) {
  QT_CHECK_ARG(d != nullptr, "%s: null descriptor", who);
  const qt_pose_lag_desc lag = pc_duration_lag_as_lag(d);
  const int rc = pc_lag_check_desc(who, &lag);
  if (rc != QT_OK && rc != QT_ERR_UNSUPPORTED) return rc;
  QT_CHECK_ARG(d->max_duration >= 1 && d->max_duration <= PC_MAX_D, "%s: max_duration = %d; 1 .. %d are handled", who,
               d->max_duration, PC_MAX_D);
  if (rc != QT_OK) return rc;
  if (d->seen > PC_DUR_LAG_MAX_SEEN - d->frames) {
    qt_set_error("%s: seen + frames = %lld + %d; a stream of at most %lld frames is handled", who, d->seen, d->frames,
                 PC_DUR_LAG_MAX_SEEN);
    return QT_ERR_UNSUPPORTED;
  }
  return QT_OK;
}

// the seven inputs of a stream entry point: the six tables of `rows` frames and `last` (lengths, or the fixed-lag carry_in).
// probs may be null where there are no frames
struct PcDurInputs {
  PcBuf v[7];
};
inline PcDurInputs pc_dur_inputs(const float* probs, long long rows, long long ld, int C, int S, int D, const int* state_class,
                                 const int* trans, const int* init, const int* dur, const int* dur_open, const PcBuf& last) {
  const size_t sd = (size_t)S * D * 4;
  return {{{probs, rows ? (size_t)((rows - 1) * ld + C) * 4 : 0, "probs", 3, rows != 0},
           {state_class, (size_t)S * 4, "state_class", 3, true},
           {trans, (size_t)S * S * 4, "trans", 3, true},
           {init, (size_t)S * 4, "init", 3},
           {dur, sd, "dur", 3, true},
           {dur_open, sd, "dur_open", 3},
           last}};
}

// the launch of a stream kernel, one workgroup per stream: its S <= 16 or its general instantiation, with the kernel's LDS
// limit raised to lds_max (once per device) where the call needs more than 64 KB
template <auto SMALL_KERNEL, auto LARGE_KERNEL, typename Args>
inline int pc_launch_stream(int S, size_t lds, size_t lds_max, int B, void* stream, const Args& a) {
  static std::atomic<unsigned long long> raised[2] = {{0}, {0}};
  const bool small = S <= 16;
  const auto kernel = small ? SMALL_KERNEL : LARGE_KERNEL;
  if (lds > 64 * 1024)
    if (const int rc = qt_raise_lds_limit(reinterpret_cast<const void*>(kernel), (int)lds_max, raised[small])) return rc;
  hipLaunchKernelGGL(kernel, dim3((unsigned)B), dim3(PC_DUR_THREADS), lds, static_cast<hipStream_t>(stream), a);
  QT_CHECK_LAUNCH();
  return QT_OK;
}
