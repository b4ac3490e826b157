// Pose-order decoding with hold durations (qt_pose_duration_decode): the best segmentation of a whole video under an explicit-
// duration (semi-Markov) chain over the steps of the pose sequence, and the run-length counts that fit its duration table
// (qt_pose_duration_count).  include/qtcnn.h states the rule in full; the reference has no such step.  pose_chain.h supplies the
// limits PC_*, the emission rule (pc_q, pc_stage_emissions) and the buffer checks; pose_duration_chain.h the chain's inputs
// PcDurChain, the lane map with its register tables, the pieces of the walk (trans and emission staging, the ring, the loop
// over a lane's lengths, the step over the predecessors), the descriptor check and the stream kernel's launch.
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
// The emissions are staged PC_DUR_CHUNK frames at a time.  After the last frame thread 0 takes the end state, and the same workgroup
// walks the segments back through the workspace (its own stores, behind a barrier) and writes a segment's frames across its
// lanes (d <= 128 <= 256).  No workgroup waits for another, no atomics, no host synchronisation; every workspace slot that is
// read has been written in the same call.
// pd_count_kernel: one thread per frame; the thread at the last frame of a run that the video does not cut walks back to the
// run's first frame and adds 1 to counts[j][min(length, D) - 1] with an integer atomic (exact in any order).
#include <stdint.h>

#include "pose_chain.h"
#include "pose_duration_chain.h"

namespace {

struct PdArgs : PcDurChain {   // T: the frames of the descriptor
  long long* path;
  long long* start;
  long long* score;
  unsigned short* bp;        // workspace: [batch][T][S], row f - 1: (dlen[f][j] - 1) | from[f][j] << 7
};

inline size_t pd_lds_bytes(int S, int D) { return 8 * ((size_t)D * S + S + 1) + 4 * (size_t)S * S + 2 * (size_t)PC_DUR_CHUNK * S; }

template <bool SMALL>
__global__ __launch_bounds__(PC_DUR_THREADS) void pd_stream_kernel(PdArgs a) {
  constexpr int LPS = PC_DUR_LPS<SMALL>;
  extern __shared__ __attribute__((aligned(16))) long long pd_lds[];
  const int S = a.S, D = a.D, tid = threadIdx.x, b = blockIdx.x;
  long long* ring = pd_lds;                                  // [D][S]: g of the last D frames, row f mod D
  long long* alpha = ring + D * S;                           // [S], and [S]: the end state
  int* tr = reinterpret_cast<int*>(alpha + S + 1);           // [S][S]
  short* e_l = reinterpret_cast<short*>(tr + S * S);         // [PC_DUR_CHUNK][S]
  const PcDurLane<LPS> ln(tid, S, D, a.dur, a.dur_open);
  const int j = ln.j, l = ln.l, jj = ln.jj;
  const bool own = ln.own;
  const int T = pc_stream_length(a.lengths, b, a.T);
  pc_stage_trans(a.trans, tr, S);
  if (tid < S) alpha[tid] = pc_init_score(a.init, tid);
  __syncthreads();

  long long cum = 0, beta;
  int from;
  beta = pc_dur_step_in<LPS>(alpha, tr, S, l, jj, from);      // beta[0]: the scores before the first frame; cum[0] = 0
  if (own) ring[j] = beta;
  unsigned short* __restrict__ bp = a.bp + (long long)b * a.T * S;
  int row = 0;
  for (int f = 1; f <= T; ++f) {
    const int g = f - 1;
    cum += pc_chunk_row(a, b, g, T, e_l, pc_chunk_start(g))[jj];
    row = pc_ring_next(row, D);                  // f mod D
    const bool cut = f == T;
    long long best = LLONG_MIN;
    int bd = INT_MAX;
    pc_for_lengths<LPS>(min(D, f), l, [&](int k, int d) {
      const long long v = ring[pc_ring_behind(row, d, D) * S + jj] + ((cut || d == f) ? ln.dop[k] : ln.du[k]);
      if (v > best) best = v, bd = d;
    });
    pc_group_max<LPS>(best, bd);
    if (own) alpha[j] = cum + best;
    __syncthreads();
    if (f < T) {
      beta = pc_dur_step_in<LPS>(alpha, tr, S, l, jj, from);
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
  for (int f = T + tid; f < a.T; f += PC_DUR_THREADS) {
    path[f] = -1;
    if (start) start[f] = -1;
  }
}

__global__ __launch_bounds__(PC_DUR_THREADS) void pd_count_kernel(const long long* __restrict__ path, long long ld,
                                                                  const int* __restrict__ lengths, unsigned long long* counts,
                                                                  int batch, int frames, int S, int D) {
  const long long idx = (long long)blockIdx.x * PC_DUR_THREADS + threadIdx.x;
  if (idx >= (long long)batch * frames) return;
  const int b = (int)(idx / frames), f = (int)(idx - (long long)b * frames);
  const int T = pc_stream_length(lengths, b, frames);
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
  const long long need = pd_workspace_bytes(desc), rows = (long long)B * T;
  const PcDurInputs in =
      pc_dur_inputs(probs, rows, ld, C, S, D, state_class, trans, init, dur, dur_open, {lengths, (size_t)B * 4, "lengths", 3});
  const PcBuf out[] = {{path, (size_t)rows * 8, "path", 7, true}, {start, (size_t)rows * 8, "start", 7},
                       {score, (size_t)B * 8, "score", 7}, {workspace, (size_t)need, "workspace", 7}};
  if (const int rc = pc_check_bufs(who, in.v, out,
                                   {workspace, workspace_bytes, need, "qt_pose_duration_workspace_bytes asks for %lld"}))
    return rc;

  PdArgs a;
  pc_dur_fill(a, probs, ld, state_class, trans, init, dur, dur_open, lengths, T, C, S, D);
  a.path = path;
  a.start = start;
  a.score = score;
  a.bp = static_cast<unsigned short*>(workspace);
  return pc_launch_stream<pd_stream_kernel<true>, pd_stream_kernel<false>>(S, pd_lds_bytes(S, D), pd_lds_bytes(PC_MAX_S, PC_MAX_D),
                                                                          B, stream, a);
}

extern "C" int qt_pose_duration_count(const qt_pose_duration_desc* desc, const long long* path, long long ld_path,
                                      const int* lengths, long long* counts, void* stream) {
  const char* const who = "qt_pose_duration_count";
  if (const int rc = pc_duration_check_desc(who, desc)) return rc;
  const int B = desc->batch, T = desc->frames, S = desc->num_states, D = desc->max_duration;
  QT_CHECK_ARG(ld_path >= T, "%s: row stride ld_path = %lld < frames = %d", who, ld_path, T);
  const PcBuf in[] = {{path, (size_t)((B - 1) * ld_path + T) * 8, "path", 7, true}, {lengths, (size_t)B * 4, "lengths", 3}};
  const PcBuf out[] = {{counts, (size_t)S * D * 8, "counts", 7, true}};
  if (const int rc = pc_check_bufs(who, in, out)) return rc;
  const long long rows = (long long)B * T;
  hipLaunchKernelGGL(pd_count_kernel, dim3((unsigned)qt_cdiv(rows, PC_DUR_THREADS)), dim3(PC_DUR_THREADS), 0,
                     static_cast<hipStream_t>(stream), path, ld_path, lengths, reinterpret_cast<unsigned long long*>(counts), B, T,
                     S, D);
  QT_CHECK_LAUNCH();
  return QT_OK;
}
