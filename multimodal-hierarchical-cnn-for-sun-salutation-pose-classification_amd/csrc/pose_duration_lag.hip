// Fixed-lag pose-order decoding with hold durations (qt_pose_duration_lag_decode): qt_pose_duration_decode's semi-Markov Viterbi
// for a loop that hands over a frame or a few per call.  include/qtcnn.h states the rule in full; the reference has no such
// step.  pose_chain.h supplies the limits PC_*, the emission rule, the emitted span and the buffer checks;
// pose_duration_chain.h the chain's inputs PcDurChain, the lane map with its register tables, the pieces of the walk, the
// lane-group maximum, the descriptor check and the stream kernel's launch.
//
// The frame step is pd_stream_kernel's (pose_duration.hip): one workgroup of 256 per stream, a group of LPS lanes per state
// with the state's slices of dur and dur_open in registers, the ring g[f][j] = beta[f][j] - cum[f][j] of the last D frames in
// LDS (row f mod D), two barriers a frame, emissions staged PC_DUR_CHUNK frames at a time.  What differs:
//   - the ring and cum come from carry_in (beta[0] at seen == 0) and leave through carry_out; f counts from the stream's start;
//   - any frame may be the last one seen so far, so (A) takes two maxima over the same ring reads: the closed one (dur; dur_open
//     only where the segment touches the stream's start), which feeds beta as for f < T of the whole-video decoder, and the
//     open one (dur_open throughout), which is that decoder's alpha[T] on the stream cut after frame f.  With dur_open NULL the
//     two are one and the second is skipped;
//   - (B) also has wave 0 take end[f], the lowest state at the maximum of the open alpha, by shuffles; lane 0 writes filtered,
//     score and the tail word (dlen_open[f][end] - 1) | end << 7, and the state's lane 0 the hist word (dlen - 1) | from << 7,
//     to the workspace.
// Behind the last barrier one thread per emitted frame walks its window back from the tail word of frame w through at most lag
// hist rows, from the workspace (the workgroup's own stores) at f > seen and from carry_in's hist at f <= seen; then the
// workgroup writes carry_out in full.  One launch, one route: no workgroup waits for another, no atomics, no host
// synchronisation; inputs, carry_in included, are never written; every workspace slot that is read is written in the same call.
#include <stdint.h>

#include "pose_chain.h"
#include "pose_duration_chain.h"

namespace {

static_assert(PC_MAX_S <= QT_WAVE, "wave 0 takes the end state, lane = state");

struct PdlArgs : PcDurChain {   // T: the new frames of the call; lengths: null
  const char* carry_in;
  char* carry_out;
  long long* lag_path;
  long long* lag_start;
  long long* filtered;
  long long* score;
  unsigned short* ws_hist;   // workspace: [batch][n][S], row i: the hist word of frame f = seen + i + 1
  unsigned short* ws_tail;   //            [batch][n]: its tail word
  long long seen, g0, g1, carry_stride;
  int lag, row0;             // row0: seen mod D
};

// a stream's carry: { int64 cum[S]; int64 g[D][S]; uint16 hist[lag][S]; uint16 tail }, rounded up to 8 bytes
struct PdlCarry {
  long long* cum;
  long long* g;
  unsigned short* hist;      // slot k: f = seen - lag + 1 + k of the call that reads it
  unsigned short* tail;
};
__host__ __device__ inline long long pdl_carry_body(int S, int D, int lag) { return 8LL * S + 8LL * D * S + 2LL * lag * S + 2; }
inline long long pdl_carry_stride(int S, int D, int lag) { return (pdl_carry_body(S, D, lag) + 7) / 8 * 8; }
__device__ __forceinline__ PdlCarry pdl_carry(const char* base, long long stride, int b, int S, int D, int lag) {
  char* p = const_cast<char*>(base) + (long long)b * stride;
  PdlCarry c;
  c.cum = reinterpret_cast<long long*>(p);
  c.g = c.cum + S;
  c.hist = reinterpret_cast<unsigned short*>(c.g + D * S);
  c.tail = c.hist + lag * S;
  return c;
}

inline size_t pdl_lds_bytes(int S, int D) {
  return 8 * ((size_t)D * S + 2 * S) + 4 * ((size_t)S * S + S) + 2 * (size_t)PC_DUR_CHUNK * S;
}
inline long long pdl_hist_bytes(const qt_pose_duration_lag_desc* d) {
  return ((long long)d->batch * d->frames * d->num_states * 2 + 7) / 8 * 8;
}
inline long long pdl_workspace_bytes(const qt_pose_duration_lag_desc* d) {
  return pdl_hist_bytes(d) + ((long long)d->batch * d->frames * 2 + 7) / 8 * 8;
}

template <bool SMALL>
__global__ __launch_bounds__(PC_DUR_THREADS) void pdl_stream_kernel(PdlArgs a) {
  constexpr int LPS = PC_DUR_LPS<SMALL>;
  extern __shared__ __attribute__((aligned(16))) long long pdl_lds[];
  const int S = a.S, D = a.D, lag = a.lag, n = a.T, tid = threadIdx.x, b = blockIdx.x;
  long long* ring = pdl_lds;                                 // [D][S]: g of the last D frames, row f mod D
  long long* alpha = ring + D * S;                           // [S]: the closed maximum
  long long* alpha_o = alpha + S;                            // [S]: the open one
  int* tr = reinterpret_cast<int*>(alpha_o + S);             // [S][S]
  int* dlo = tr + S * S;                                     // [S]: dlen_open of the frame
  short* e_l = reinterpret_cast<short*>(dlo + S);            // [PC_DUR_CHUNK][S]
  const PcDurLane<LPS> ln(tid, S, D, a.dur, a.dur_open);
  const int j = ln.j, l = ln.l, jj = ln.jj;
  const bool own = ln.own;
  const bool two = a.dur_open != a.dur;          // (uniform)
  const long long seen = a.seen;
  const PdlCarry in = pdl_carry(a.carry_in, a.carry_stride, b, S, D, lag);
  const PdlCarry out = pdl_carry(a.carry_out, a.carry_stride, b, S, D, lag);

  pc_stage_trans(a.trans, tr, S);

  long long cum = 0, beta;
  int from;
  if (seen == 0) {                               // beta[0]: the scores before the first frame; cum[0] = 0; the other rows zero
    for (int idx = tid; idx < D * S; idx += PC_DUR_THREADS) ring[idx] = 0;
    if (tid < S) alpha[tid] = pc_init_score(a.init, tid);
    __syncthreads();
    beta = pc_dur_step_in<LPS>(alpha, tr, S, l, jj, from);
    if (own) ring[j] = beta;
  } else {
    for (int idx = tid; idx < D * S; idx += PC_DUR_THREADS) ring[idx] = in.g[idx];
    cum = in.cum[jj];
  }
  __syncthreads();

  unsigned short* __restrict__ hist = a.ws_hist + (long long)b * n * S;
  unsigned short* __restrict__ tail = a.ws_tail + (long long)b * n;
  int row = a.row0;
  long long f = seen;
  for (int i = 0; i < n; ++i) {
    ++f;
    cum += pc_chunk_row(a, b, i, n, e_l, pc_chunk_start(i))[jj];
    row = pc_ring_next(row, D);                  // f mod D
    long long best = LLONG_MIN, best_o = LLONG_MIN;
    int bd = INT_MAX, bd_o = INT_MAX;
    pc_for_lengths<LPS>((int)min((long long)D, f), l, [&](int k, int d) {
      const long long g = ring[pc_ring_behind(row, d, D) * S + jj];
      const long long v = g + (d == f ? ln.dop[k] : ln.du[k]);
      if (v > best) best = v, bd = d;
      if (two) {
        const long long vo = g + ln.dop[k];
        if (vo > best_o) best_o = vo, bd_o = d;
      }
    });
    pc_group_max<LPS>(best, bd);
    if (two) pc_group_max<LPS>(best_o, bd_o);
    else best_o = best, bd_o = bd;
    if (own) {
      alpha[j] = cum + best;
      alpha_o[j] = cum + best_o;
      dlo[j] = bd_o;
    }
    __syncthreads();
    beta = pc_dur_step_in<LPS>(alpha, tr, S, l, jj, from);
    if (own) {
      ring[row * S + j] = beta - cum;            // (row f - D was last read in (A))
      hist[(long long)i * S + j] = (unsigned short)((bd - 1) | (from << 7));
    }
    if (tid < QT_WAVE) {                         // end[f]: the lowest state at the maximum of the open alpha
      long long m = tid < S ? alpha_o[tid] : LLONG_MIN;
      int e = tid;
      pc_group_max<QT_WAVE>(m, e);
      if (tid == 0) {
        tail[i] = (unsigned short)((dlo[e] - 1) | (e << 7));
        if (a.filtered) a.filtered[(long long)b * n + i] = e;
        if (a.score) a.score[(long long)b * n + i] = m;
      }
    }
    __syncthreads();
  }

  // the windows: thread = emitted frame.  The walk stays at g < f <= w whatever the words hold, and a state is clamped.
  const long long end = seen + n, last = end - 1, count = a.g1 - a.g0;
  for (long long g = a.g0 + tid; g < a.g1; g += PC_DUR_THREADS) {
    const long long w = g + lag < last ? g + lag : last;
    long long ff = w + 1;
    const unsigned t = ff > seen ? tail[ff - seen - 1] : *in.tail;
    int s = min((int)(t >> 7), S - 1), d = (int)(t & 127) + 1;
    while (ff - d > g) {                         // the segment in front: the state that beta[ff][s] came from, and its length
      ff -= d;
      const unsigned short* __restrict__ h = ff > seen ? hist + (ff - seen - 1) * S : in.hist + (ff - (seen - lag + 1)) * S;
      s = min((int)(h[s] >> 7), S - 1);
      d = (int)(h[s] & 127) + 1;
    }
    a.lag_path[(long long)b * count + (g - a.g0)] = s;
    if (a.lag_start) a.lag_start[(long long)b * count + (g - a.g0)] = ff - d;
  }

  // carry_out, in full: cum, the ring as it stands, hist of f = end - lag + 1 .. end (zeros for f <= 0), the tail, the padding
  if (own) out.cum[j] = cum;
  for (int idx = tid; idx < D * S; idx += PC_DUR_THREADS) out.g[idx] = ring[idx];
  for (int idx = tid; idx < lag * S; idx += PC_DUR_THREADS) {
    const int k = (int)fdiv((unsigned)idx, a.div_s);
    const long long fk = end - lag + 1 + k;
    unsigned short v = 0;
    if (fk > seen) v = hist[(fk - seen - 1) * S + (idx - k * S)];
    else if (fk > 0) v = in.hist[(fk - (seen - lag + 1)) * S + (idx - k * S)];
    out.hist[idx] = v;
  }
  if (tid == 0) {
    *out.tail = n > 0 ? tail[n - 1] : (seen > 0 ? *in.tail : (unsigned short)0);
    const int pad = (int)(a.carry_stride - pdl_carry_body(S, D, lag)) / 2;
    for (int k = 1; k <= pad; ++k) out.tail[k] = 0;
  }
}

}  // namespace

extern "C" long long qt_pose_duration_lag_carry_bytes(const qt_pose_duration_lag_desc* desc) {
  if (pc_duration_lag_check_desc("qt_pose_duration_lag_carry_bytes", desc) != QT_OK) return 0;
  return desc->batch * pdl_carry_stride(desc->num_states, desc->max_duration, desc->lag);
}

extern "C" long long qt_pose_duration_lag_workspace_bytes(const qt_pose_duration_lag_desc* desc) {
  if (pc_duration_lag_check_desc("qt_pose_duration_lag_workspace_bytes", desc) != QT_OK) return 0;
  return pdl_workspace_bytes(desc);
}

extern "C" int qt_pose_duration_lag_decode(const qt_pose_duration_lag_desc* desc, const float* probs, long long ld,
                                           const int* state_class, const int* trans, const int* init, const int* dur,
                                           const int* dur_open, const void* carry_in, void* carry_out, long long* lag_path,
                                           long long* lag_start, long long* filtered, long long* score, void* workspace,
                                           long long workspace_bytes, void* stream) {
  const char* const who = "qt_pose_duration_lag_decode";
  if (const int rc = pc_duration_lag_check_desc(who, desc)) return rc;
  const int B = desc->batch, T = desc->frames, C = desc->num_classes, S = desc->num_states, D = desc->max_duration;
  const int lag = desc->lag;
  const qt_pose_lag_desc as_lag = pc_duration_lag_as_lag(desc);
  const PcSpan span = pc_lag_span(&as_lag);
  const long long count = span.count;
  QT_CHECK_ARG(ld >= C, "%s: row stride ld = %lld < C = %d", who, ld, C);
  const long long need = pdl_workspace_bytes(desc), stride = pdl_carry_stride(S, D, lag), rows = (long long)B * T;
  const size_t carry_bytes = (size_t)(B * stride);
  // carry_in is not read at seen == 0: it may be null there and overlaps nothing
  const PcDurInputs in = pc_dur_inputs(probs, rows, ld, C, S, D, state_class, trans, init, dur, dur_open,
                                       {carry_in, desc->seen ? carry_bytes : 0, "carry_in", 7});
  const PcBuf out[] = {{carry_out, carry_bytes, "carry_out", 7, true}, {lag_path, (size_t)(B * count) * 8, "lag_path", 7},
                       {lag_start, (size_t)(B * count) * 8, "lag_start", 7}, {filtered, (size_t)rows * 8, "filtered", 7},
                       {score, (size_t)rows * 8, "score", 7}, {workspace, (size_t)need, "workspace", 7}};
  if (const int rc = pc_check_present(who, in.v, out)) return rc;
  QT_CHECK_ARG(count == 0 || lag_path != nullptr, "%s: null lag_path (the call emits %lld frames)", who, count);
  QT_CHECK_ARG(desc->seen == 0 || carry_in != nullptr, "%s: null carry_in with seen = %lld", who, desc->seen);
  if (const int rc = pc_check_aligned(who, in.v, out)) return rc;
  if (const int rc = pc_check_room(who, {workspace, workspace_bytes, need, "qt_pose_duration_lag_workspace_bytes asks for %lld"}))
    return rc;
  QT_CHECK_ARG(!overlap(carry_in, in.v[6].bytes, carry_out, carry_bytes), "%s: carry_in must not overlap carry_out", who);
  if (const int rc = pc_check_disjoint(who, in.v, out)) return rc;

  PdlArgs a;
  pc_dur_fill(a, probs, ld, state_class, trans, init, dur, dur_open, nullptr, T, C, S, D);
  a.carry_in = desc->seen ? static_cast<const char*>(carry_in) : nullptr;
  a.carry_out = static_cast<char*>(carry_out);
  a.lag_path = lag_path;
  a.lag_start = lag_start;
  a.filtered = filtered;
  a.score = score;
  a.ws_hist = static_cast<unsigned short*>(workspace);
  a.ws_tail = reinterpret_cast<unsigned short*>(static_cast<char*>(workspace) + pdl_hist_bytes(desc));
  a.seen = desc->seen;
  a.g0 = span.g0;
  a.g1 = span.g1;
  a.carry_stride = stride;
  a.lag = lag;
  a.row0 = (int)(desc->seen % D);
  return pc_launch_stream<pdl_stream_kernel<true>, pdl_stream_kernel<false>>(S, pdl_lds_bytes(S, D),
                                                                            pdl_lds_bytes(PC_MAX_S, PC_MAX_D), B, stream, a);
}
