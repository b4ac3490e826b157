// Learning the chain with hold durations on the device (semi-Markov Baum-Welch): the expected transition, start and duration
// counts under the chain's own posterior (qt_pose_duration_prior_expect), the hard counts of given segmentations
// (qt_pose_duration_prior_count_paths) and the new tables from the counts (qt_pose_duration_prior_update).  include/qtcnn.h
// states the rules in full; the reference has no such step.
// expect, two launches: (a) pose_duration_sweep.h's stream kernel in its LEARN mode, the very sweeps of
// qt_pose_duration_posterior, so that Z and the duration counts are that function's bits; every (i, j) and (j, d) slot is owned
// by one lane, a stream's terms are added in descending f into double registers and go to the workspace as the stream's
// partials; (b) pq_reduce_kernel, one thread per slot, adds the streams' partials in ascending stream order from zero and adds
// that sum onto the accumulator.  pose_chain.h supplies the buffer checks, pose_duration_chain.h the descriptor check, the
// seven inputs as a list, a stream's length and the stream kernel's launch.  No float atomics, no zero fill of caller memory, no host synchronisation.
// count_paths, two launches: (a) a workgroup of 256 per (stream, chunk of PQ_CHUNK frames) counts the boundaries and the uncut
// segments that END in its chunk into int histograms [S][S] and [S][D] in LDS (integer atomics on LDS: the result does not
// depend on their order) and writes them to the workspace; (b) one thread per slot adds the chunks of every stream in int64 and
// adds the sum, an exact integer, onto the double accumulator; start counts and frames are read off path and lengths there.
// update, one launch of one workgroup: thread i < S row i of trans, thread S the new init (both pose_chain.h's pc_update_row:
// qt_pose_prior_update's bits), thread S + 1 + j row j of dur and of dur_open.
#include "pose_duration_sweep.h"

namespace {

constexpr int PQ_THREADS = 256;
constexpr int PQ_CHUNK = 1024;                   // frames per workgroup of count (a); a histogram entry stays below 2^10

inline long long pq_part_elems(const qt_pose_duration_desc* d) {   // a stream's partials: xi, start, dur counts, Z
  const long long S = d->num_states, D = d->max_duration;
  return S * S + S + S * D + 1;
}
inline long long pq_workspace_bytes(const qt_pose_duration_desc* d) {
  return 8 * (2 * pp_level_elems(d) + (long long)d->batch * pq_part_elems(d));
}
inline long long pq_count_workspace_bytes(const qt_pose_duration_desc* d) {   // int32 [batch][chunks][S * S + S * D]
  const long long S = d->num_states, D = d->max_duration;
  return ((long long)d->batch * qt_cdiv(d->frames, PQ_CHUNK) * (S * S + S * D) * 4 + 7) / 8 * 8;
}

// accumulator[slot] += the streams' partials in ascending stream order, from zero; totals[0] += the sum of Z, totals[1] += the
// sum of T_b
__global__ __launch_bounds__(PQ_THREADS) void pq_reduce_kernel(const double* __restrict__ xi_part, const double* __restrict__ start_part,
                                                               const double* __restrict__ dur_part, const double* __restrict__ z_part,
                                                               const int* __restrict__ lengths, double* trans_counts,
                                                               double* start_counts, double* dur_counts, double* totals, int batch,
                                                               int frames, int S, int D) {
  const int SS = S * S, SD = S * D, idx = blockIdx.x * PQ_THREADS + threadIdx.x;
  double s = 0.0;
  if (idx < SS) {
    for (int b = 0; b < batch; ++b) s += xi_part[(long long)b * SS + idx];
    trans_counts[idx] += s;
  } else if (idx < SS + SD) {
    const int k = idx - SS;
    for (int b = 0; b < batch; ++b) s += dur_part[(long long)b * SD + k];
    dur_counts[k] += s;
  } else if (idx < SS + SD + S) {
    if (!start_counts) return;
    const int k = idx - SS - SD;
    for (int b = 0; b < batch; ++b) s += start_part[(long long)b * S + k];
    start_counts[k] += s;
  } else if (idx == SS + SD + S) {
    for (int b = 0; b < batch; ++b) s += z_part[b];
    totals[0] += s;
  } else if (idx == SS + SD + S + 1) {
    long long n = 0;
    for (int b = 0; b < batch; ++b) n += pc_stream_length(lengths, b, frames);
    totals[1] += (double)n;
  }
}

// true where a segment begins at frame f of p (1 <= f < T)
__device__ __forceinline__ bool pq_boundary(const long long* __restrict__ p, const long long* __restrict__ st, int f) {
  return st ? st[f] == f : p[f] != p[f - 1];
}

__global__ __launch_bounds__(PQ_THREADS) void pq_count_kernel(const long long* __restrict__ path, const long long* __restrict__ start,
                                                              long long ld, const int* __restrict__ lengths, int* __restrict__ partial,
                                                              int frames, int chunks, int S, int D) {
  extern __shared__ int pq_hist[];               // [S][S] transitions, then [S][D] durations
  const int n = S * S + S * D, tid = threadIdx.x;
  const int b = blockIdx.x / chunks, chunk = blockIdx.x - b * chunks;
  const int T = pc_stream_length(lengths, b, frames);
  const int f0 = max(chunk * PQ_CHUNK, 1), f1 = min((chunk + 1) * PQ_CHUNK, T);
  for (int idx = tid; idx < n; idx += PQ_THREADS) pq_hist[idx] = 0;
  __syncthreads();
  const long long* __restrict__ p = path + (long long)b * ld;
  const long long* __restrict__ st = start ? start + (long long)b * ld : nullptr;
  for (int f = f0 + tid; f < f1; f += PQ_THREADS) {      // f: a boundary in 1 .. T - 1, the end of the segment in front of it
    if (!pq_boundary(p, st, f)) continue;
    const long long from = p[f - 1], to = p[f];
    if (from >= 0 && from < S && to >= 0 && to < S) atomicAdd(&pq_hist[(int)from * S + (int)to], 1);
    int s = f - 1;                               // the segment [s, f): back to its own boundary
    while (s > 0 && !pq_boundary(p, st, s)) --s;
    const long long v = p[s];
    if (s > 0 && v >= 0 && v < S) atomicAdd(&pq_hist[S * S + (int)v * D + min(f - s, D) - 1], 1);
  }
  __syncthreads();
  int* __restrict__ out = partial + (long long)blockIdx.x * n;
  for (int idx = tid; idx < n; idx += PQ_THREADS) out[idx] = pq_hist[idx];
}

__global__ __launch_bounds__(PQ_THREADS) void pq_count_reduce_kernel(const long long* __restrict__ path, long long ld,
                                                                     const int* __restrict__ lengths, const int* __restrict__ partial,
                                                                     double* trans_counts, double* start_counts, double* dur_counts,
                                                                     double* totals, int batch, int frames, int chunks, int S, int D) {
  const int SS = S * S, n = SS + S * D, idx = blockIdx.x * PQ_THREADS + threadIdx.x;
  long long s = 0;
  if (idx < n) {
    for (long long k = 0; k < (long long)batch * chunks; ++k) s += partial[k * n + idx];
    if (idx < SS) trans_counts[idx] += (double)s;
    else dur_counts[idx - SS] += (double)s;
  } else if (idx < n + S) {
    if (!start_counts) return;
    for (int b = 0; b < batch; ++b) s += path[(long long)b * ld] == idx - n;
    start_counts[idx - n] += (double)s;
  } else if (idx == n + S) {
    for (int b = 0; b < batch; ++b) s += pc_stream_length(lengths, b, frames);
    totals[1] += (double)s;
  }
}

// row j of dur: r[d] = allowed ? count + pseudo : 0, R = sum in ascending d; R > 0: q((float)(r / R)) where allowed and -65536
// elsewhere; otherwise dur_in's values; dur_open, where asked for, is the row's suffix maximum
__device__ void pq_dur_row(const double* __restrict__ src, const int* __restrict__ allowed, double pseudo, const int* old, int* dst,
                           int* open, int D) {
  double R = 0.0;
  for (int d = 0; d < D; ++d) R += allowed[d] ? src[d] + pseudo : 0.0;
  int best = PC_TRANS_FLOOR;
  for (int d = D - 1; d >= 0; --d) {             // (a slot is read before it is written: dst may be old)
    int v = old[d];
    if (R > 0.0) v = allowed[d] ? pc_q((float)((src[d] + pseudo) / R)) : PC_TRANS_FLOOR;
    dst[d] = v;
    best = max(best, v);
    if (open) open[d] = best;
  }
}

__global__ __launch_bounds__(PQ_THREADS) void pq_update_kernel(const double* __restrict__ trans_counts,
                                                               const double* __restrict__ start_counts,
                                                               const double* __restrict__ dur_counts, const int* __restrict__ allowed,
                                                               const int* __restrict__ dur_allowed, double pseudo, double dur_pseudo,
                                                               const int* trans_in, const int* init_in, const int* dur_in,
                                                               int* trans_out, int* init_out, int* dur_out, int* dur_open_out, int S,
                                                               int D) {
  const int i = threadIdx.x;   // (a row is read and written by its own thread alone: an out may be its in)
  if (i < S) {
    pc_update_row(trans_counts + i * S, allowed + i * S, pseudo, trans_in + i * S, trans_out + i * S, S);
  } else if (i == S) {
    if (init_out) pc_update_row(start_counts, nullptr, pseudo, init_in, init_out, S);
  } else if (i <= 2 * S) {
    const int j = i - S - 1;
    pq_dur_row(dur_counts + j * D, dur_allowed + j * D, dur_pseudo, dur_in + j * D, dur_out + j * D,
               dur_open_out ? dur_open_out + j * D : nullptr, D);
  }
}
static_assert(2 * PC_MAX_S + 1 <= PQ_THREADS, "a thread per row");

inline bool pq_finite_nonneg(double v) { return v >= 0.0 && v <= 1.7976931348623157e308; }

}  // namespace

extern "C" long long qt_pose_duration_prior_workspace_bytes(const qt_pose_duration_desc* desc) {
  if (pc_duration_check_desc("qt_pose_duration_prior_workspace_bytes", desc) != QT_OK) return 0;
  return pq_workspace_bytes(desc);
}

extern "C" int qt_pose_duration_prior_expect(const qt_pose_duration_desc* desc, const float* probs, long long ld,
                                             const int* state_class, const int* trans, const int* init, const int* dur,
                                             const int* dur_open, const int* lengths, double* trans_counts, double* start_counts,
                                             double* dur_counts, double* totals, void* workspace, long long workspace_bytes,
                                             void* stream) {
  const char* const who = "qt_pose_duration_prior_expect";
  if (const int rc = pc_duration_check_desc(who, desc)) return rc;
  const int B = desc->batch, T = desc->frames, C = desc->num_classes, S = desc->num_states, D = desc->max_duration;
  QT_CHECK_ARG(ld >= C, "%s: row stride ld = %lld < C = %d", who, ld, C);
  const long long need = pq_workspace_bytes(desc), rows = (long long)B * T;
  const PcDurInputs in =
      pc_dur_inputs(probs, rows, ld, C, S, D, state_class, trans, init, dur, dur_open, {lengths, (size_t)B * 4, "lengths", 3});
  const PcBuf out[] = {{trans_counts, (size_t)S * S * 8, "trans_counts", 7, true}, {start_counts, (size_t)S * 8, "start_counts", 7},
                       {dur_counts, (size_t)S * D * 8, "dur_counts", 7, true}, {totals, 16, "totals", 7, true},
                       {workspace, (size_t)need, "workspace", 7}};
  if (const int rc = pc_check_bufs(who, in.v, out,
                                   {workspace, workspace_bytes, need, "qt_pose_duration_prior_workspace_bytes asks for %lld"}))
    return rc;

  PpArgs a;
  pc_dur_fill(a, probs, ld, state_class, trans, init, dur, dur_open, lengths, T, C, S, D);
  a.posterior = a.class_posterior = a.begin = nullptr;
  a.evidence = nullptr;
  a.g = static_cast<double*>(workspace);
  a.al = a.g + pp_level_elems(desc);
  a.part = a.al + pp_level_elems(desc);
  a.xi_part = a.part + (long long)B * S * D;
  a.start_part = a.xi_part + (long long)B * S * S;
  a.z_part = a.start_part + (long long)B * S;
  double* const start_part = a.start_part;
  if (!start_counts) a.start_part = nullptr;
  if (const int rc = pc_launch_stream<pp_stream_kernel<true, true>, pp_stream_kernel<false, true>>(
          S, pp_lds_bytes(S, D), pp_lds_bytes(PC_MAX_S, PC_MAX_D), B, stream, a))
    return rc;
  hipLaunchKernelGGL(pq_reduce_kernel, dim3((unsigned)qt_cdiv(pq_part_elems(desc) + 1, PQ_THREADS)), dim3(PQ_THREADS), 0,
                     static_cast<hipStream_t>(stream), (const double*)a.xi_part, (const double*)start_part, (const double*)a.part,
                     (const double*)a.z_part, lengths, trans_counts, start_counts, dur_counts, totals, B, T, S, D);
  QT_CHECK_LAUNCH();
  return QT_OK;
}

extern "C" int qt_pose_duration_prior_count_paths(const qt_pose_duration_desc* desc, const long long* path, const long long* start,
                                                  long long ld_path, const int* lengths, double* trans_counts,
                                                  double* start_counts, double* dur_counts, double* totals, void* workspace,
                                                  long long workspace_bytes, void* stream) {
  const char* const who = "qt_pose_duration_prior_count_paths";
  if (const int rc = pc_duration_check_desc(who, desc)) return rc;
  const int B = desc->batch, T = desc->frames, S = desc->num_states, D = desc->max_duration, chunks = qt_cdiv(T, PQ_CHUNK);
  QT_CHECK_ARG(ld_path >= T, "%s: row stride ld_path = %lld < frames = %d", who, ld_path, T);
  const long long need = pq_count_workspace_bytes(desc);
  const size_t pb = (size_t)((B - 1) * ld_path + T) * 8;
  const PcBuf in[] = {{path, pb, "path", 7, true}, {start, pb, "start", 7}, {lengths, (size_t)B * 4, "lengths", 3}};
  const PcBuf out[] = {{trans_counts, (size_t)S * S * 8, "trans_counts", 7, true}, {start_counts, (size_t)S * 8, "start_counts", 7},
                       {dur_counts, (size_t)S * D * 8, "dur_counts", 7, true}, {totals, 16, "totals", 7, true},
                       {workspace, (size_t)need, "workspace", 7}};
  if (const int rc = pc_check_bufs(who, in, out,
                                   {workspace, workspace_bytes, need,
                                    "%lld are needed (qt_pose_duration_prior_workspace_bytes asks for no less)"}))
    return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  int* partial = static_cast<int*>(workspace);
  const int n = S * S + S * D;
  hipLaunchKernelGGL(pq_count_kernel, dim3((unsigned)(B * chunks)), dim3(PQ_THREADS), (size_t)n * 4, s, path, start, ld_path,
                     lengths, partial, T, chunks, S, D);
  QT_CHECK_LAUNCH();
  hipLaunchKernelGGL(pq_count_reduce_kernel, dim3((unsigned)qt_cdiv(n + S + 1, PQ_THREADS)), dim3(PQ_THREADS), 0, s, path, ld_path,
                     lengths, (const int*)partial, trans_counts, start_counts, dur_counts, totals, B, T, chunks, S, D);
  QT_CHECK_LAUNCH();
  return QT_OK;
}

extern "C" int qt_pose_duration_prior_update(int num_states, int max_duration, const double* trans_counts,
                                             const double* start_counts, const double* dur_counts, const int* allowed,
                                             const int* dur_allowed, double pseudo_count, double dur_pseudo_count,
                                             const int* trans_in, const int* init_in, const int* dur_in, int* trans_out,
                                             int* init_out, int* dur_out, int* dur_open_out, void* stream) {
  const char* const who = "qt_pose_duration_prior_update";
  const int S = num_states, D = max_duration;
  QT_CHECK_ARG(S >= 1 && S <= PC_MAX_S, "%s: num_states = %d; 1 .. %d are handled", who, S, PC_MAX_S);
  QT_CHECK_ARG(D >= 1 && D <= PC_MAX_D, "%s: max_duration = %d; 1 .. %d are handled", who, D, PC_MAX_D);
  QT_CHECK_ARG(pq_finite_nonneg(pseudo_count), "%s: pseudo_count must be a finite number that is not negative (got %g)", who,
               pseudo_count);
  QT_CHECK_ARG(pq_finite_nonneg(dur_pseudo_count), "%s: dur_pseudo_count must be a finite number that is not negative (got %g)",
               who, dur_pseudo_count);
  QT_CHECK_ARG(trans_counts != nullptr && allowed != nullptr && trans_in != nullptr && trans_out != nullptr, "%s: null %s", who,
               !trans_counts ? "trans_counts" : !allowed ? "allowed" : !trans_in ? "trans_in" : "trans_out");
  QT_CHECK_ARG(dur_counts != nullptr && dur_allowed != nullptr && dur_in != nullptr && dur_out != nullptr, "%s: null %s", who,
               !dur_counts ? "dur_counts" : !dur_allowed ? "dur_allowed" : !dur_in ? "dur_in" : "dur_out");
  QT_CHECK_ARG(init_out == nullptr || start_counts != nullptr, "%s: null start_counts with an init_out", who);
  QT_CHECK_ARG(!misaligned(trans_counts, 7) && !misaligned(start_counts, 7) && !misaligned(dur_counts, 7) &&
                   !misaligned(allowed, 3) && !misaligned(dur_allowed, 3) && !misaligned(trans_in, 3) && !misaligned(init_in, 3) &&
                   !misaligned(dur_in, 3) && !misaligned(trans_out, 3) && !misaligned(init_out, 3) && !misaligned(dur_out, 3) &&
                   !misaligned(dur_open_out, 3),
               "%s: trans_counts, start_counts and dur_counts must be 8-byte aligned, allowed, dur_allowed, trans_in, init_in, "
               "dur_in, trans_out, init_out, dur_out and dur_open_out 4-byte", who);
  const size_t tb = (size_t)S * S * 4, ib = (size_t)S * 4, db = (size_t)S * D * 4;
  const PcBuf in[] = {{trans_counts, 2 * tb, "trans_counts"}, {start_counts, 2 * ib, "start_counts"},
                      {dur_counts, 2 * db, "dur_counts"}, {allowed, tb, "allowed"}, {dur_allowed, db, "dur_allowed"},
                      {trans_in, tb, "trans_in"}, {init_in, ib, "init_in"}, {dur_in, db, "dur_in"}},
              out[] = {{trans_out, tb, "trans_out"}, {init_out, ib, "init_out"}, {dur_out, db, "dur_out"},
                       {dur_open_out, db, "dur_open_out"}};
  for (const PcBuf& o : out) {
    for (const PcBuf& i : in) {
      const bool in_place = (o.p == trans_out && i.p == trans_in && trans_out == trans_in) ||
                            (o.p == init_out && i.p == init_in && init_out == init_in) ||
                            (o.p == dur_out && i.p == dur_in && dur_out == dur_in);
      QT_CHECK_ARG(in_place || !overlap(o.p, o.bytes, i.p, i.bytes),
                   "%s: %s must not overlap %s (trans_out may be trans_in itself, init_out init_in itself, dur_out dur_in itself)",
                   who, o.name, i.name);
    }
    for (const PcBuf& o2 : out)
      QT_CHECK_ARG(&o == &o2 || !overlap(o.p, o.bytes, o2.p, o2.bytes), "%s: %s must not overlap %s", who, o.name, o2.name);
  }
  hipLaunchKernelGGL(pq_update_kernel, dim3(1), dim3(PQ_THREADS), 0, static_cast<hipStream_t>(stream), trans_counts, start_counts,
                     dur_counts, allowed, dur_allowed, pseudo_count, dur_pseudo_count, trans_in, init_in, dur_in, trans_out,
                     init_out, dur_out, dur_open_out, S, D);
  QT_CHECK_LAUNCH();
  return QT_OK;
}
