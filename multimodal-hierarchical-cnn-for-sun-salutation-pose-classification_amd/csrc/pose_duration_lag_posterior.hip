// Fixed-lag pose-order posteriors with hold durations (qt_pose_duration_lag_smooth): qt_pose_duration_posterior's marginals for
// a loop that hands over a frame or a few per call.  include/qtcnn.h states the rule in full; the reference has no such step.
// pose_chain.h supplies the limits, the emission rule, the emitted span and the buffer checks; pose_duration_chain.h the chain's
// inputs PcDurChain, the lane map with its register tables, the pieces of the walk, the descriptor check and the stream
// kernel's launch; pose_duration_sweep.h the arithmetic of the two sweeps (pp_group_L, pp_length_L, pp_evidence, pp_owner_step,
// pp_row, pp_class_sum), the very functions the whole-video kernel runs, which is how a window's bits are that kernel's bits
// on the stream's prefix.
//
// Two launches on the caller's stream:
//   pls_forward_kernel, one workgroup of 256 per stream: pp_stream_kernel's forward step with f counted from the stream's
//     start.  The ring g[f][j] = Bt[f][j] - cum[f][j] / 256 of the last D frames and cum come from carry_in (Bt[0] at seen == 0).
//     (A) takes two Ls over the same ring rows: the closed Al[f] (dur_open only where the segment touches the stream's start),
//     which feeds Bt[f], and Al_open[f] (dur_open throughout), the whole-video kernel's Al[T] on the stream cut after frame f;
//     with dur_open NULL the two are one and the second is skipped.  (B) also has wave 0 form Z_f = L_j Al_open[f][j].  Every
//     new frame's g[f - 1], closed Al[f], Al_open[f], cum[f], Z_f and int16 emission row go to the workspace, Z_f to
//     log2_evidence; then the workgroup writes carry_out in full.
//   pls_window_kernel, one workgroup of 256 per (stream, emitted frame) and, with `filtered`, per (stream, new frame): the
//     whole-video kernel's backward sweep on the prefix [0, F) from f = F - 1 down to f = g only, the same lane map, so an L adds
//     in the same order.  h[f][j] = Be[f][j] + cum[f][j] / 256 of its at most lag + 1 frames lies in LDS as rows f - g, cum steps
//     back from cum[F] through the int16 rows; the forward rows come from the workspace for the frames of this call and from
//     carry_in for older ones.  It writes its one row of each output.  Windows share nothing.
// No workgroup waits for another, no atomics, no host synchronisation; inputs, carry_in included, are never written; every
// workspace slot that is read is written in the same call (by the first launch); no index comes from memory.
#include <stdint.h>

#include "pose_chain.h"
#include "pose_duration_chain.h"
#include "pose_duration_sweep.h"

namespace {

// levels are absolute doubles, as in the whole-video kernel: a stream has that kernel's frame limit
constexpr long long PLS_MAX_SEEN = PC_MAX_FRAMES;

struct PlsArgs : PcDurChain {   // T: the new frames of the call; lengths: null
  const char* carry_in;
  char* carry_out;
  float* lagged;
  float* lagged_class;
  float* lagged_begin;
  float* filtered;
  double* evidence;
  double* ws_g;              // workspace [batch][n][S], row i: g[f] of f = seen + i
  double* ws_al;             //           [batch][n][S], row i: the closed Al[f] of f = seen + i + 1
  double* ws_alo;            //           [batch][n][S]: Al_open[f] of the same f
  long long* ws_cum;         //           [batch][n][S]: cum[f] of the same f
  double* ws_z;              //           [batch][n]: Z_f of the same f
  short* ws_e;               //           [batch][n][S], row i: the emissions of frame seen + i
  long long seen, g0, g1, carry_stride;
  int lag, row0, per;        // row0: seen mod D; per: the windows of a stream, count (+ n with filtered)
};

// a stream's carry: { int64 cum[S]; double ring[D][S]; double gh[lag][S]; double al[lag][S]; double al_open[S]; double Z;
// int16 e[lag][S] }, rounded up to 8 bytes
struct PlsCarry {
  long long* cum;            // cum[seen]
  double* ring;              // g[f] at row f mod D, the last D values of f
  double* gh;                // slot k: g[f] of f = seen - lag + k (of the call that reads it)
  double* al;                // slot k: the closed Al[f] of f = seen - lag + 1 + k
  double* alo;               // Al_open[seen]
  double* z;                 // Z_seen
  short* e;                  // slot k: the emissions of frame seen - lag + k
};
__host__ __device__ inline long long pls_carry_body(int S, int D, int lag) {
  return 8LL * S + 8LL * D * S + 16LL * lag * S + 8LL * S + 8 + 2LL * lag * S;
}
inline long long pls_carry_stride(int S, int D, int lag) { return (pls_carry_body(S, D, lag) + 7) / 8 * 8; }
__device__ __forceinline__ PlsCarry pls_carry(const char* base, long long stride, int b, int S, int D, int lag) {
  char* p = const_cast<char*>(base) + (long long)b * stride;
  PlsCarry c;
  c.cum = reinterpret_cast<long long*>(p);
  c.ring = reinterpret_cast<double*>(c.cum + S);
  c.gh = c.ring + D * S;
  c.al = c.gh + lag * S;
  c.alo = c.al + lag * S;
  c.z = c.alo + S;
  c.e = reinterpret_cast<short*>(c.z + 1);
  return c;
}

// the ring, the closed and the open level, trans, the staged emissions
inline size_t pls_forward_lds(int S, int D) {
  return 8 * ((size_t)D * S + 2 * S) + 4 * (size_t)S * S + 2 * (size_t)PC_DUR_CHUNK * S;
}
// the window's rows of h (f - g = 0 .. lag + 1), r = max(occ, 0), Bs, trans, state_class, the posterior row
inline size_t pls_window_lds(int S, int lag) { return 8 * ((size_t)(lag + 2) * S + 2 * S) + 4 * ((size_t)S * S + 2 * S); }
inline long long pls_rows(const qt_pose_duration_lag_desc* d) { return (long long)d->batch * d->frames * d->num_states; }
inline long long pls_workspace_bytes(const qt_pose_duration_lag_desc* d) {
  return 32 * pls_rows(d) + 8LL * d->batch * d->frames + (2 * pls_rows(d) + 7) / 8 * 8;
}

template <bool SMALL>
__global__ __launch_bounds__(PC_DUR_THREADS) void pls_forward_kernel(PlsArgs a) {
  constexpr int LPS = PC_DUR_LPS<SMALL>;
  extern __shared__ __attribute__((aligned(16))) double pls_lds[];
  const int S = a.S, D = a.D, lag = a.lag, n = a.T, tid = threadIdx.x, b = blockIdx.x;
  double* ring = pls_lds;                                    // [D][S]: g of the last D frames, row f mod D
  double* lev = ring + D * S;                                // [S]: start, the closed Al[f]
  double* lev_o = lev + S;                                   // [S]: Al_open[f]
  int* tr = reinterpret_cast<int*>(lev_o + S);               // [S][S]
  short* e_l = reinterpret_cast<short*>(tr + S * S);         // [PC_DUR_CHUNK][S]
  const PcDurLane<LPS> ln(tid, S, D, a.dur, a.dur_open);
  const int j = ln.j, l = ln.l, jj = ln.jj;
  const bool own = ln.own;
  const bool two = a.dur_open != a.dur;          // (uniform)
  const long long seen = a.seen;
  const PlsCarry in = pls_carry(a.carry_in, a.carry_stride, b, S, D, lag);
  const PlsCarry out = pls_carry(a.carry_out, a.carry_stride, b, S, D, lag);

  pc_stage_trans(a.trans, tr, S);
  auto step_in = [&]() { return pp_group_L<LPS>(S, l, [&](int i) { return lev[i] + pp_bits(tr[i * S + jj]); }); };

  long long cum = 0;
  if (seen == 0) {                               // Bt[0]; cum[0] = 0; the other rows zero
    for (int idx = tid; idx < D * S; idx += PC_DUR_THREADS) ring[idx] = 0.0;
    if (tid < S) lev[tid] = pp_bits(pc_init_score(a.init, tid));
    __syncthreads();
    const double bt = step_in();
    if (own) ring[j] = bt;
  } else {
    for (int idx = tid; idx < D * S; idx += PC_DUR_THREADS) ring[idx] = in.ring[idx];
    cum = in.cum[jj];
  }
  __syncthreads();

  const long long base = (long long)b * n * S;
  double* __restrict__ gw = a.ws_g + base;
  double* __restrict__ alw = a.ws_al + base;
  double* __restrict__ alow = a.ws_alo + base;
  long long* __restrict__ cumw = a.ws_cum + base;
  short* __restrict__ ew = a.ws_e + base;
  double* __restrict__ zw = a.ws_z + (long long)b * n;
  int row = a.row0;
  long long f = seen;
  double Z = 0.0;                                // Z_f of the newest frame (wave 0)
  for (int i = 0; i < n; ++i) {
    ++f;
    const short* e_f = pc_chunk_row(a, b, i, n, e_l, pc_chunk_start(i));
    if (own) {
      gw[(long long)i * S + j] = ring[row * S + j];        // g[f - 1]
      ew[(long long)i * S + j] = e_f[j];
    }
    cum += e_f[jj];
    row = pc_ring_next(row, D);                  // f mod D
    const int dmax = (int)min((long long)D, f);
    const double lc = pp_length_L<LPS>(ln, ring, S, D, dmax, row, true, (int)f, false);
    const double lo = two ? pp_length_L<LPS>(ln, ring, S, D, dmax, row, true, (int)f, true) : lc;
    if (own) {
      const double alv = lc + pp_bits(cum), alo = lo + pp_bits(cum);
      lev[j] = alv;
      lev_o[j] = alo;
      alw[(long long)i * S + j] = alv;
      alow[(long long)i * S + j] = alo;
      cumw[(long long)i * S + j] = cum;
    }
    __syncthreads();
    const double bt = step_in();
    if (own) ring[row * S + j] = bt - pp_bits(cum);        // (row f - D was last read in (A))
    if (tid < QT_WAVE) {
      Z = pp_evidence(lev_o, S);
      if (tid == 0) {
        zw[i] = Z;
        if (a.evidence) a.evidence[(long long)b * n + i] = Z;
      }
    }
    __syncthreads();
  }

  // carry_out, in full: cum, the ring as it stands, the rows of the last lag frames (zeros in front of the stream's start),
  // Al_open and Z of the newest f, the padding
  const long long end = seen + n;
  if (own) {
    out.cum[j] = cum;
    out.alo[j] = n > 0 ? lev_o[j] : (seen > 0 ? in.alo[j] : 0.0);
  }
  for (int idx = tid; idx < D * S; idx += PC_DUR_THREADS) out.ring[idx] = ring[idx];
  for (int idx = tid; idx < lag * S; idx += PC_DUR_THREADS) {
    const int k = (int)fdiv((unsigned)idx, a.div_s), s = idx - k * S;
    const long long fg = end - lag + k, fa = fg + 1;       // g[fg], the emissions of frame fg; Al[fa]
    double gv = 0.0, av = 0.0;
    short ev = 0;
    if (fg >= seen) gv = gw[(fg - seen) * S + s], ev = ew[(fg - seen) * S + s];
    else if (fg >= 0) gv = in.gh[(fg - (seen - lag)) * S + s], ev = in.e[(fg - (seen - lag)) * S + s];
    if (fa > seen) av = alw[(fa - seen - 1) * S + s];
    else if (fa > 0) av = in.al[(fa - (seen - lag + 1)) * S + s];
    out.gh[idx] = gv;
    out.al[idx] = av;
    out.e[idx] = ev;
  }
  if (tid == 0) {
    *out.z = n > 0 ? Z : (seen > 0 ? *in.z : 0.0);
    const int pad = (int)(a.carry_stride - pls_carry_body(S, D, lag)) / 2;
    for (int k = 0; k < pad; ++k) out.e[lag * S + k] = 0;
  }
}

template <bool SMALL>
__global__ __launch_bounds__(PC_DUR_THREADS) void pls_window_kernel(PlsArgs a) {
  constexpr int LPS = PC_DUR_LPS<SMALL>;
  extern __shared__ __attribute__((aligned(16))) double pls_lds[];
  const int S = a.S, C = a.C, D = a.D, lag = a.lag, n = a.T, tid = threadIdx.x;
  const int b = (int)(blockIdx.x / (unsigned)a.per), w = (int)(blockIdx.x - (unsigned)b * (unsigned)a.per);
  double* hwin = pls_lds;                                    // [lag + 2][S]: h[f], row f - g
  double* lev = hwin + (lag + 2) * S;                        // [S]: r = max(occ[g], 0)
  double* vec = lev + S;                                     // [S]: Bs[f]
  int* tr = reinterpret_cast<int*>(vec + S);                 // [S][S]
  int* sc = tr + S * S;                                      // [S]
  float* pst = reinterpret_cast<float*>(sc + S);             // [S]: the posterior row
  const PcDurLane<LPS> ln(tid, S, D, a.dur, a.dur_open);
  const int j = ln.j, l = ln.l, jj = ln.jj;
  const bool own = ln.own;
  const long long seen = a.seen, count = a.g1 - a.g0, last = seen + n - 1;
  const bool lagged = w < count;                 // else: the lag-0 window of new frame w - count
  const long long g = lagged ? a.g0 + w : seen + (w - count);
  const long long F = lagged ? (g + lag < last ? g + lag : last) + 1 : g + 1;
  const int steps = (int)(F - g);                // 1 .. lag + 1
  const PlsCarry in = pls_carry(a.carry_in, a.carry_stride, b, S, D, lag);
  const long long base = (long long)b * n * S;
  const double* __restrict__ gw = a.ws_g + base;
  const double* __restrict__ alw = a.ws_al + base;
  const short* __restrict__ ew = a.ws_e + base;
  // the forward rows: the workspace for the frames of this call, carry_in for older ones (g >= seen - lag: its slots cover them)
  auto g_at = [&](long long f, int s) { return f >= seen ? gw[(f - seen) * S + s] : in.gh[(f - (seen - lag)) * S + s]; };
  auto al_at = [&](long long f, int s) { return f > seen ? alw[(f - seen - 1) * S + s] : in.al[(f - (seen - lag + 1)) * S + s]; };
  auto e_at = [&](long long f, int s) { return f >= seen ? ew[(f - seen) * S + s] : in.e[(f - (seen - lag)) * S + s]; };
  const bool fresh = F > seen;                   // (uniform) Al_open[F], cum[F], Z_F are of this call
  const long long at_f = base + (fresh ? (F - seen - 1) * S : 0);
  const double* __restrict__ alo_f = fresh ? a.ws_alo + at_f : in.alo;
  long long cum = fresh ? a.ws_cum[at_f + jj] : in.cum[jj];
  const double Z = fresh ? a.ws_z[(long long)b * n + (F - seen - 1)] : *in.z;

  pc_stage_trans(a.trans, tr, S);
  if (tid < S) sc[tid] = a.state_class[tid];
  if (own) hwin[steps * S + j] = pp_bits(cum);   // h[F] = cum[F] / 256: Be[F] = 0
  double be_next = 0.0, occ = 0.0;               // Be[f + 1][j], occ[f + 1][j]
  float begin_next = 0.0f;                       // begin[f + 1][j]
  __syncthreads();
  for (long long f = F - 1; f >= g; --f) {
    const int r = (int)(f - g);
    cum -= e_at(f, jj);                          // cum[f]
    const double lh = pp_length_L<LPS>(ln, hwin, S, lag + 2, min(D, (int)(F - f)), r, false, (int)(F - f), f == 0);
    if (own) {
      const double al_next = f == F - 1 ? alo_f[j] : al_at(f + 1, j);
      const float bg = pp_owner_step(g_at(f, j), lh, al_next, be_next, Z, f == F - 1, occ, begin_next);
      vec[j] = lh - pp_bits(cum);
      if (f == g) {
        lev[j] = fmax(occ, 0.0);
        if (lagged && a.lagged_begin) a.lagged_begin[((long long)b * count + w) * S + j] = bg;
      }
    }
    __syncthreads();
    if (f > g) {                                 // Be[f] and h[f]; f >= 1 here
      be_next = pp_group_L<LPS>(S, l, [&](int i) { return pp_bits(tr[jj * S + i]) + vec[i]; });
      if (own) hwin[r * S + j] = be_next + pp_bits(cum);
      __syncthreads();
    }
  }
  if (own) {
    const float p = pp_row(lev, S, j);
    pst[j] = p;
    if (lagged) a.lagged[((long long)b * count + w) * S + j] = p;
    else a.filtered[((long long)b * n + (w - count)) * S + j] = p;
  }
  if (lagged && a.lagged_class) {                // (uniform)
    __syncthreads();
    if (tid < C) a.lagged_class[((long long)b * count + w) * C + tid] = pp_class_sum(pst, sc, S, tid);
  }
}

inline int pls_check_desc(const char* who, const qt_pose_duration_lag_desc* d) {
  const int rc = pc_duration_lag_check_desc(who, d);
  if (rc != QT_OK && rc != QT_ERR_UNSUPPORTED) return rc;
  if (d->seen > PLS_MAX_SEEN - d->frames) {
    qt_set_error("%s: seen + frames = %lld + %d; a stream of at most %lld frames is handled", who, d->seen, d->frames,
                 PLS_MAX_SEEN);
    return QT_ERR_UNSUPPORTED;
  }
  return rc;
}

}  // namespace

extern "C" long long qt_pose_duration_lag_smooth_carry_bytes(const qt_pose_duration_lag_desc* desc) {
  if (pls_check_desc("qt_pose_duration_lag_smooth_carry_bytes", desc) != QT_OK) return 0;
  return desc->batch * pls_carry_stride(desc->num_states, desc->max_duration, desc->lag);
}

extern "C" long long qt_pose_duration_lag_smooth_workspace_bytes(const qt_pose_duration_lag_desc* desc) {
  if (pls_check_desc("qt_pose_duration_lag_smooth_workspace_bytes", desc) != QT_OK) return 0;
  return pls_workspace_bytes(desc);
}

extern "C" int qt_pose_duration_lag_smooth(const qt_pose_duration_lag_desc* desc, const float* probs, long long ld,
                                           const int* state_class, const int* trans, const int* init, const int* dur,
                                           const int* dur_open, const void* carry_in, void* carry_out, float* lagged,
                                           float* lagged_class, float* lagged_begin, float* filtered, double* log2_evidence,
                                           void* workspace, long long workspace_bytes, void* stream) {
  const char* const who = "qt_pose_duration_lag_smooth";
  if (const int rc = pls_check_desc(who, desc)) return rc;
  const int B = desc->batch, T = desc->frames, C = desc->num_classes, S = desc->num_states, D = desc->max_duration;
  const int lag = desc->lag;
  const qt_pose_lag_desc as_lag = pc_duration_lag_as_lag(desc);
  const PcSpan span = pc_lag_span(&as_lag);
  const long long count = span.count;
  QT_CHECK_ARG(ld >= C, "%s: row stride ld = %lld < C = %d", who, ld, C);
  const long long need = pls_workspace_bytes(desc), stride = pls_carry_stride(S, D, lag), rows = (long long)B * T;
  const size_t carry_bytes = (size_t)(B * stride);
  // carry_in is not read at seen == 0: it may be null there and overlaps nothing
  const PcDurInputs in = pc_dur_inputs(probs, rows, ld, C, S, D, state_class, trans, init, dur, dur_open,
                                       {carry_in, desc->seen ? carry_bytes : 0, "carry_in", 7});
  const PcBuf out[] = {{carry_out, carry_bytes, "carry_out", 7, true},
                       {lagged, (size_t)(B * count) * S * 4, "lagged", 3},
                       {lagged_class, (size_t)(B * count) * C * 4, "lagged_class", 3},
                       {lagged_begin, (size_t)(B * count) * S * 4, "lagged_begin", 3},
                       {filtered, (size_t)rows * S * 4, "filtered", 3},
                       {log2_evidence, (size_t)rows * 8, "log2_evidence", 7},
                       {workspace, (size_t)need, "workspace", 7}};
  if (const int rc = pc_check_present(who, in.v, out)) return rc;
  QT_CHECK_ARG(count == 0 || lagged != nullptr, "%s: null lagged (the call emits %lld frames)", who, count);
  QT_CHECK_ARG(desc->seen == 0 || carry_in != nullptr, "%s: null carry_in with seen = %lld", who, desc->seen);
  if (const int rc = pc_check_aligned(who, in.v, out)) return rc;
  if (const int rc =
          pc_check_room(who, {workspace, workspace_bytes, need, "qt_pose_duration_lag_smooth_workspace_bytes asks for %lld"}))
    return rc;
  QT_CHECK_ARG(!overlap(carry_in, in.v[6].bytes, carry_out, carry_bytes), "%s: carry_in must not overlap carry_out", who);
  if (const int rc = pc_check_disjoint(who, in.v, out)) return rc;

  PlsArgs a;
  pc_dur_fill(a, probs, ld, state_class, trans, init, dur, dur_open, nullptr, T, C, S, D);
  a.carry_in = desc->seen ? static_cast<const char*>(carry_in) : nullptr;
  a.carry_out = static_cast<char*>(carry_out);
  a.lagged = lagged;
  a.lagged_class = count ? lagged_class : nullptr;
  a.lagged_begin = count ? lagged_begin : nullptr;
  a.filtered = T ? filtered : nullptr;
  a.evidence = T ? log2_evidence : nullptr;
  const long long elems = pls_rows(desc);
  a.ws_g = static_cast<double*>(workspace);
  a.ws_al = a.ws_g + elems;
  a.ws_alo = a.ws_al + elems;
  a.ws_cum = reinterpret_cast<long long*>(a.ws_alo + elems);
  a.ws_z = reinterpret_cast<double*>(a.ws_cum + elems);
  a.ws_e = reinterpret_cast<short*>(a.ws_z + rows);
  a.seen = desc->seen;
  a.g0 = span.g0;
  a.g1 = span.g1;
  a.carry_stride = stride;
  a.lag = lag;
  a.row0 = (int)(desc->seen % D);
  a.per = (int)(count + (a.filtered ? T : 0));
  if (const int rc = pc_launch_stream<pls_forward_kernel<true>, pls_forward_kernel<false>>(
          S, pls_forward_lds(S, D), pls_forward_lds(PC_MAX_S, PC_MAX_D), B, stream, a))
    return rc;
  if (a.per > 0) {
    pc_by_small(S, [&](auto small) {
      hipLaunchKernelGGL(pls_window_kernel<PC_SMALL(small)>, dim3((unsigned)((long long)B * a.per)), dim3(PC_DUR_THREADS),
                         pls_window_lds(S, lag), static_cast<hipStream_t>(stream), a);
    });
    QT_CHECK_LAUNCH();
  }
  return QT_OK;
}
