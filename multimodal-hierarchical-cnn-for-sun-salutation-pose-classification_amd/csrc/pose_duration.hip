// Pose-order decoding with hold durations (qt_pose_duration_decode): the best segmentation of a whole video under an explicit-
// duration (semi-Markov) chain over the steps of the pose sequence, and the run-length counts that fit its duration table
// (qt_pose_duration_count).  include/qtcnn.h states the rule in full; the reference has no such step.  pose_chain.h supplies the
// limits PC_*, the emission rule (pc_q, pc_stage_emissions), the chain's inputs PcChain, the lane-group maximum pc_group_max,
// the overlap check and the S <= 16 switch.
//
// The recurrence has order D in the frame index, so the (max, +) tile products of pose_order.hip do not apply (the semiring
// state would be S * D wide).  One workgroup of 256 per stream walks the frames in order.  With cum[f][j] the prefix sum of the
// emissions and g[f][j] = beta[f][j] - cum[f][j],
//   alpha[f][j] = cum[f][j] + max_d (g[f - d][j] + len(j, d, f)),
// so the last D rows of g, a ring of int64 [D][S] in LDS, are all the history a step needs.  LDS is dynamic: at S = 64, D = 128
// the ring alone is 64 KB, with the tables 90,632 bytes, so the launch raises the kernel's limit (160 KB per CU).  Everything is
// int64 and absolute: no offset, no saturation to reason about (|beta| < 2^20 frames * 2^18 per frame).
// A group of LPS lanes serves a state (16 lanes for S <= 16, 4 above: 256 threads either way) and keeps the state's slices of
// dur and dur_open in registers, lane l the lengths d = 1 + l + k LPS.  A frame is two maxima and two barriers:
//   (A) every lane takes the maximum over its own lengths in ascending d, the group reduces (value, d) by shuffles, the lower d
//       winning a tie; lane 0 leaves alpha[f][j] in LDS;                                                            barrier
//   (B) the group's lanes share the S predecessors i of state j the same way, the lower i winning a tie; lane 0 writes
//       g[f][j] into ring row f mod D (row f - D was last read in (A)) and (dlen - 1) | from << 7 to the workspace;  barrier
// The emissions are staged PD_CHUNK frames at a time.  After the last frame thread 0 takes the end state, and the same workgroup
// walks the segments back through the workspace (its own stores, behind a barrier) and writes a segment's frames across its
// lanes (d <= 128 <= 256).  No workgroup waits for another, no atomics, no host synchronisation; every workspace slot that is
// read has been written in the same call.
// pd_count_kernel: one thread per frame; the thread at the last frame of a run that the video does not cut walks back to the
// run's first frame and adds 1 to counts[j][min(length, D) - 1] with an integer atomic (exact in any order).
#include <limits.h>
#include <stdint.h>

#include "pose_chain.h"

namespace {

constexpr int PD_THREADS = 256;
constexpr int PD_CHUNK = 64;                     // frames of emissions staged at a time
constexpr int PD_MAX_D = 128;
static_assert(PD_MAX_D == PC_MAX_D, "pose_chain.h checks the descriptor against this");
static_assert(PD_MAX_D <= PD_THREADS && PD_MAX_D <= 128 && PC_MAX_S <= 64, "a segment's frames go across the lanes; 7 + 6 bits");

struct PdArgs : PcChain {    // T: the frames of the descriptor (tiles: not read)
  const int* dur;
  const int* dur_open;       // never null: dur where the caller gave none
  const int* lengths;
  long long* path;
  long long* start;
  long long* score;
  unsigned short* bp;        // workspace: [batch][T][S], row f - 1: (dlen[f][j] - 1) | from[f][j] << 7
  int D;
};

inline size_t pd_lds_bytes(int S, int D) { return 8 * ((size_t)D * S + S + 1) + 4 * (size_t)S * S + 2 * (size_t)PD_CHUNK * S; }

template <bool SMALL>
__global__ __launch_bounds__(PD_THREADS) void pd_stream_kernel(PdArgs a) {
  constexpr int LPS = SMALL ? 16 : 4;            // lanes per state
  constexpr int KMAX = PD_MAX_D / LPS;           // lengths per lane
  extern __shared__ __attribute__((aligned(16))) long long pd_lds[];
  const int S = a.S, D = a.D, tid = threadIdx.x, b = blockIdx.x;
  long long* ring = pd_lds;                                  // [D][S]: g of the last D frames, row f mod D
  long long* alpha = ring + D * S;                           // [S], and [S]: the end state
  int* tr = reinterpret_cast<int*>(alpha + S + 1);           // [S][S]
  short* e_l = reinterpret_cast<short*>(tr + S * S);         // [PD_CHUNK][S]
  const int j = tid / LPS, l = tid - j * LPS, jj = min(j, S - 1);
  const bool own = l == 0 && j < S;              // (groups beyond S compute on state S - 1 and store nothing)
  int T = a.T;
  if (a.lengths) T = min(max(a.lengths[b], 1), a.T);

  int du[KMAX], dop[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    const int d0 = l + k * LPS;
    du[k] = d0 < D ? pc_clamp_trans(a.dur[jj * D + d0]) : 0;
    dop[k] = d0 < D ? pc_clamp_trans(a.dur_open[jj * D + d0]) : 0;
  }
  for (int idx = tid; idx < S * S; idx += PD_THREADS) tr[idx] = pc_clamp_trans(a.trans[idx]);
  if (tid < S) alpha[tid] = a.init ? (long long)pc_clamp_trans(a.init[tid]) : 0;
  __syncthreads();

  // (B): max_i (alpha[i] + trans[i][j]) and the lowest i that attains it
  auto step_in = [&](long long& best, int& from) {
    best = LLONG_MIN, from = INT_MAX;
    for (int i = l; i < S; i += LPS) {
      const long long v = alpha[i] + tr[i * S + jj];
      if (v > best) best = v, from = i;
    }
    pc_group_max<LPS>(best, from);
  };

  long long cum = 0, beta;
  int from;
  step_in(beta, from);                           // beta[0]: the scores before the first frame; cum[0] = 0
  if (own) ring[j] = beta;
  unsigned short* __restrict__ bp = a.bp + (long long)b * a.T * S;
  int row = 0;
  for (int f = 1; f <= T; ++f) {
    const int g = f - 1;
    if ((g & (PD_CHUNK - 1)) == 0) {             // (the chunk before was last read two barriers ago)
      pc_stage_emissions(a, b, g, min(PD_CHUNK, T - g), e_l);
      __syncthreads();
    }
    cum += e_l[(g & (PD_CHUNK - 1)) * S + jj];
    row = row + 1 == D ? 0 : row + 1;            // f mod D
    const int dmax = min(D, f);
    const bool cut = f == T;
    long long best = LLONG_MIN;
    int bd = INT_MAX;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      if (k * LPS >= dmax) break;                // (uniform)
      const int d = 1 + l + k * LPS;
      if (d <= dmax) {
        int r = row - d;
        r += r < 0 ? D : 0;
        const long long v = ring[r * S + jj] + ((cut || d == f) ? dop[k] : du[k]);
        if (v > best) best = v, bd = d;
      }
    }
    pc_group_max<LPS>(best, bd);
    if (own) alpha[j] = cum + best;
    __syncthreads();
    if (f < T) {
      step_in(beta, from);
      if (own) {
        ring[row * S + j] = beta - cum;
        bp[(long long)g * S + j] = (unsigned short)((bd - 1) | (from << 7));
      }
    } else {
      if (own) bp[(long long)g * S + j] = (unsigned short)(bd - 1);
      if (tid == 0) {                            // the lowest state at the maximum of alpha[T]
        long long m = alpha[0];
        int last = 0;
        for (int s = 1; s < S; ++s)
          if (alpha[s] > m) m = alpha[s], last = s;
        alpha[S] = last;
        if (a.score) a.score[b] = m;
      }
    }
    __syncthreads();
  }

  // the segments, from the last to the first (every thread walks; a segment's frames go across the lanes)
  long long* __restrict__ path = a.path + (long long)b * a.T;
  long long* __restrict__ start = a.start ? a.start + (long long)b * a.T : nullptr;
  int s = (int)alpha[S];
  for (int f = T; f > 0;) {
    const int d = min((int)(bp[(long long)(f - 1) * S + s] & 127) + 1, f), st = f - d;
    if (tid < d) {
      path[st + tid] = s;
      if (start) start[st + tid] = st;
    }
    f = st;
    if (f > 0) s = min((int)(bp[(long long)(f - 1) * S + s] >> 7), S - 1);
  }
  for (int f = T + tid; f < a.T; f += PD_THREADS) {
    path[f] = -1;
    if (start) start[f] = -1;
  }
}

__global__ __launch_bounds__(PD_THREADS) void pd_count_kernel(const long long* __restrict__ path, long long ld,
                                                              const int* __restrict__ lengths, unsigned long long* counts,
                                                              int batch, int frames, int S, int D) {
  const long long idx = (long long)blockIdx.x * PD_THREADS + threadIdx.x;
  if (idx >= (long long)batch * frames) return;
  const int b = (int)(idx / frames), f = (int)(idx - (long long)b * frames);
  const int T = lengths ? min(max(lengths[b], 1), frames) : frames;
  if (f + 1 >= T) return;                        // the stream's last run is cut by the video
  const long long* __restrict__ p = path + (long long)b * ld;
  const long long v = p[f];
  if (v < 0 || v >= S || p[f + 1] == v) return;  // not a run's last frame
  int s = f;
  while (s > 0 && p[s - 1] == v) --s;
  if (s == 0) return;                            // the stream's first run is cut by the video
  atomicAdd(&counts[(int)v * D + min(f - s + 1, D) - 1], 1ull);
}

inline long long pd_workspace_bytes(const qt_pose_duration_desc* d) {
  return ((long long)d->batch * d->frames * d->num_states * 2 + 7) / 8 * 8;
}

}  // namespace

extern "C" long long qt_pose_duration_workspace_bytes(const qt_pose_duration_desc* desc) {
  if (pc_duration_check_desc("qt_pose_duration_workspace_bytes", desc) != QT_OK) return 0;
  return pd_workspace_bytes(desc);
}

extern "C" int qt_pose_duration_decode(const qt_pose_duration_desc* desc, const float* probs, long long ld,
                                       const int* state_class, const int* trans, const int* init, const int* dur,
                                       const int* dur_open, const int* lengths, long long* path, long long* start,
                                       long long* score, void* workspace, long long workspace_bytes, void* stream) {
  const char* const who = "qt_pose_duration_decode";
  if (const int rc = pc_duration_check_desc(who, desc)) return rc;
  const int B = desc->batch, T = desc->frames, C = desc->num_classes, S = desc->num_states, D = desc->max_duration;
  QT_CHECK_ARG(ld >= C, "%s: row stride ld = %lld < C = %d", who, ld, C);
  QT_CHECK_ARG(probs != nullptr && state_class != nullptr && trans != nullptr && dur != nullptr && path != nullptr,
               "%s: null %s", who, !probs ? "probs" : !state_class ? "state_class" : !trans ? "trans" : !dur ? "dur" : "path");
  QT_CHECK_ARG(!misaligned(probs, 3) && !misaligned(state_class, 3) && !misaligned(trans, 3) && !misaligned(init, 3) &&
                   !misaligned(dur, 3) && !misaligned(dur_open, 3) && !misaligned(lengths, 3) && !misaligned(path, 7) &&
                   !misaligned(start, 7) && !misaligned(score, 7) && !misaligned(workspace, 7),
               "%s: probs, state_class, trans, init, dur, dur_open and lengths must be 4-byte aligned, path, start, score and "
               "the workspace 8-byte", who);
  const long long need = pd_workspace_bytes(desc);
  QT_CHECK_ARG(workspace != nullptr && workspace_bytes >= need,
               "%s: workspace of %lld bytes; qt_pose_duration_workspace_bytes asks for %lld", who,
               workspace ? workspace_bytes : 0LL, need);
  const long long rows = (long long)B * T;
  const PcBuf in[] = {{probs, (size_t)((rows - 1) * ld + C) * 4, "probs"}, {state_class, (size_t)S * 4, "state_class"},
                      {trans, (size_t)S * S * 4, "trans"}, {init, (size_t)S * 4, "init"}, {dur, (size_t)S * D * 4, "dur"},
                      {dur_open, (size_t)S * D * 4, "dur_open"}, {lengths, (size_t)B * 4, "lengths"}};
  const PcBuf out[] = {{path, (size_t)rows * 8, "path"}, {start, (size_t)rows * 8, "start"}, {score, (size_t)B * 8, "score"},
                       {workspace, (size_t)need, "workspace"}};
  if (const int rc = pc_check_disjoint(who, in, out)) return rc;

  PdArgs a;
  pc_fill(a, probs, ld, state_class, trans, init, T, C, S);
  a.dur = dur;
  a.dur_open = dur_open ? dur_open : dur;
  a.lengths = lengths;
  a.path = path;
  a.start = start;
  a.score = score;
  a.bp = static_cast<unsigned short*>(workspace);
  a.D = D;
  const size_t lds = pd_lds_bytes(S, D);
  const bool small = S <= 16;
  static std::atomic<unsigned long long> raised[2] = {{0}, {0}};
  if (lds > 64 * 1024)
    if (const int rc = qt_raise_lds_limit(reinterpret_cast<const void*>(small ? pd_stream_kernel<true> : pd_stream_kernel<false>),
                                          (int)pd_lds_bytes(PC_MAX_S, PD_MAX_D), raised[small]))
      return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  pc_by_small(S, [&](auto sm) {
    hipLaunchKernelGGL(pd_stream_kernel<PC_SMALL(sm)>, dim3((unsigned)B), dim3(PD_THREADS), lds, s, a);
  });
  QT_CHECK_LAUNCH();
  return QT_OK;
}

extern "C" int qt_pose_duration_count(const qt_pose_duration_desc* desc, const long long* path, long long ld_path,
                                      const int* lengths, long long* counts, void* stream) {
  const char* const who = "qt_pose_duration_count";
  if (const int rc = pc_duration_check_desc(who, desc)) return rc;
  const int B = desc->batch, T = desc->frames, S = desc->num_states, D = desc->max_duration;
  QT_CHECK_ARG(ld_path >= T, "%s: row stride ld_path = %lld < frames = %d", who, ld_path, T);
  QT_CHECK_ARG(path != nullptr && counts != nullptr, "%s: null %s", who, !path ? "path" : "counts");
  QT_CHECK_ARG(!misaligned(path, 7) && !misaligned(counts, 7) && !misaligned(lengths, 3),
               "%s: path and counts must be 8-byte aligned, lengths 4-byte", who);
  const PcBuf in[] = {{path, (size_t)((B - 1) * ld_path + T) * 8, "path"}, {lengths, (size_t)B * 4, "lengths"}};
  const PcBuf out[] = {{counts, (size_t)S * D * 8, "counts"}};
  if (const int rc = pc_check_disjoint(who, in, out)) return rc;
  const long long rows = (long long)B * T;
  hipLaunchKernelGGL(pd_count_kernel, dim3((unsigned)qt_cdiv(rows, PD_THREADS)), dim3(PD_THREADS), 0,
                     static_cast<hipStream_t>(stream), path, ld_path, lengths, reinterpret_cast<unsigned long long*>(counts), B, T,
                     S, D);
  QT_CHECK_LAUNCH();
  return QT_OK;
}
