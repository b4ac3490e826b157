// Score-based evaluation on the device (qt_scores_update / qt_scores_finalize): top-k accuracy, one-vs-rest ROC / AUC,
// average precision and calibration from the scores themselves, where metrics.hip counts hard decisions.  The state is
// additive integer counts that stay in device memory for a whole evaluation (include/qtcnn.h states the layout and every
// formula):
//     hist[C][2][K]   counted rows by q(p_k), side 1 = rows whose label is k      rank[C]   counted rows by the true class's rank
//     cal[M][3]       rows / hits / integer confidence sum per confidence bin     five counters
//
// Update, one launch per batch.  Rows map to lanes by qt_rowgroup.h's rule (one thread per row for C <= 16, a 16-lane DPP
// row above) and the softmax of QT_SCORES_LOGITS is metrics_logits_kernel's because both are qt_row_load, qt_row_argmax and
// qt_row_softmax, so p has the bits qt_metrics_update writes to probs.  Two routes to the same integers:
//   direct      a workgroup walks row tiles with a grid stride; each lane adds its (k, side, q) cell with one 64-bit global
//               atomic, the writer lane of a row its rank and calibration cells; the counters go through ballots into LDS
//               and leave once per workgroup.
//   privatised  workgroup (x, k) owns rows [x SC_SLICE, (x + 1) SC_SLICE) and class k: it re-reads the rows (48 bytes at
//               C = 12), keeps hist[k][2][K] as u32 in LDS (8 K bytes: 32 KB at K = 4096, 128 KB at K = 16384) and leaves with
//               one 64-bit global atomic per non-zero cell.  Positives pile up in bin K - 1 and negatives in bin 0, so the
//               direct route's atomics serialise on a few addresses of a large batch; here they meet in LDS.  The workgroups
//               of class 0 also tally ranks, calibration and the counters (in LDS, u32: SC_SLICE x 65536 < 2^32).
// Neither route has a workspace, a zero fill or a host synchronisation.
//
// Finalize, two launches: C + 1 workgroups (one per class: a block scan over the K bins, a thread owning K / 256 consecutive
// bins; one for ranks, calibration and the counters), then one wave for the macro / weighted averages, which need every
// class's value: the stream's order makes them wait, no workgroup waits for another.
#include <math.h>
#include <stdint.h>

#include <atomic>

#include "qt_common.h"
#include "qt_rowgroup.h"

namespace {

constexpr int SC_THREADS = 256;
constexpr int SC_MAX_C = QT_SCORES_MAX_CLASSES;
constexpr int SC_MAX_M = QT_SCORES_MAX_CAL_BINS;
constexpr int SC_MIN_BITS = QT_SCORES_MIN_BITS, SC_MAX_BITS = QT_SCORES_MAX_BITS;
constexpr long long SC_MAX_ROWS = 1ll << 22;
constexpr int SC_MAX_BLOCKS = 2048;            // direct route: grid-stride cap, 8 workgroups per CU
constexpr int SC_SLICE = QT_SCORES_SLICE_ROWS; // privatised route: rows per workgroup
constexpr int SC_COUNTERS = 5;
constexpr int SC_SCALARS = 12;
constexpr int SC_TALLY_WORDS = SC_MAX_C + 3 * SC_MAX_M + 4;   // privatised route: rank, cal and four counters behind the histogram
static_assert(SC_MAX_C <= 64, "rows map to one thread or one 16-lane DPP row");
static_assert((long long)SC_SLICE * 65536 < (1ll << 32), "a slice's confidence sum fits u32");
static_assert((2 * (1 << SC_MAX_BITS) + SC_TALLY_WORDS) * 4 <= 160 * 1024, "LDS of the privatised route");

struct ScArgs {
  const float* s;                 // [rows][ld]
  const long long* y;             // [rows]
  long long rows, ld;
  int C, K, M;
  long long ignore_index;
  unsigned long long* state;
};

enum { ROW_COUNTED = 0, ROW_IGNORED = 1, ROW_INVALID = 2, ROW_NAN = 3, ROW_NONE = 4 };

__host__ __device__ inline size_t sc_hist_cells(int C, int K) { return 2 * (size_t)C * (size_t)K; }

// q(p) = min(K - 1, (int)(p K)): a multiplication by a power of two and a truncation, both exact
__device__ __forceinline__ int sc_q(float p, int K) { return min(K - 1, (int)(p * (float)K)); }
// the calibration bin of a confidence in [0, 1]: the product is rounded to f32 once
__device__ __forceinline__ int sc_bin(float conf, int M) { return min(M - 1, (int)(conf * (float)M)); }

template <int PER> struct RowEval {
  int cls;          // ROW_*, the same in every lane of the row
  int y;            // the label of a counted row, 0 otherwise
  float p[PER];     // this lane's probabilities (k = j * LANES + sub)
  int rank, pred;   // only with tally
  float conf;
};

// One row per group of LANES lanes.  Every lane of the wave must call it (shuffles and ballots inside).
template <int LANES, int PER, bool LOGITS>
__device__ __forceinline__ void eval_row(const ScArgs& a, long long row, int sub, bool tally, RowEval<PER>& r) {
  const int C = a.C;
  const float* __restrict__ zr = a.s + row * a.ld;
  float z[PER];
  qt_row_load<LANES, PER>(zr, C, sub, z);
#pragma unroll
  for (int j = 0; j < PER; ++j) r.p[j] = z[j];   // (0 in the lanes past C, and the softmax leaves them so)
  if (LOGITS) {
    float m;
    int at;
    qt_row_argmax<LANES, PER>(z, C, sub, m, at);
    qt_row_softmax<LANES, PER>(r.p, C, sub, m);
  }
  bool bad = false;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int k = j * LANES + sub;
    if (k < C) bad |= LOGITS ? (r.p[j] != r.p[j]) : !(r.p[j] >= 0.f && r.p[j] <= 1.f);   // (a NaN fails both comparisons)
  }
  bad = qt_group_any<LANES>(bad);
  const long long yl = a.y[row];
  r.cls = yl == a.ignore_index ? ROW_IGNORED : (yl < 0 || yl >= (long long)C) ? ROW_INVALID : bad ? ROW_NAN : ROW_COUNTED;
  r.y = r.cls == ROW_COUNTED ? (int)yl : 0;
  r.rank = 0;
  r.pred = 0;
  r.conf = 0.f;
  if (!tally) return;   // (the workgroup's: no lane is left behind)

  // rank of the true class among the scores as given: #{k : s_k > s_y, or s_k == s_y and k < y}
  float sy_l = 0.f;
#pragma unroll
  for (int j = 0; j < PER; ++j)
    if (j * LANES + sub == r.y) sy_l = z[j];
  const float sy = qt_group_pick<LANES>(sy_l, r.y & (LANES - 1));
  int above = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int k = j * LANES + sub;
    if (k < C && (z[j] > sy || (z[j] == sy && k < r.y))) ++above;
  }
  r.rank = qt_group_sum_int<LANES>(above);
  // pred = argmax of p in the loss head's order, conf = p[pred]
  qt_row_argmax<LANES, PER>(r.p, C, sub, r.conf, r.pred);
}

template <int LANES, int PER, bool LOGITS>
__global__ __launch_bounds__(SC_THREADS) void scores_direct_kernel(ScArgs a) {
  constexpr int RPB = SC_THREADS / LANES;
  __shared__ unsigned cnt[4];
  if (threadIdx.x < 4) cnt[threadIdx.x] = 0u;
  __syncthreads();
  const int sub = threadIdx.x & (LANES - 1);
  const int C = a.C, K = a.K;
  unsigned long long* __restrict__ rank = a.state + sc_hist_cells(C, K);
  unsigned long long* __restrict__ cal = rank + C;
  const long long tiles = (a.rows + RPB - 1) / RPB;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {   // uniform per workgroup
    const long long row0 = tile * RPB + threadIdx.x / LANES;
    const bool live = row0 < a.rows;
    const long long row = live ? row0 : a.rows - 1;   // idle lanes repeat the last row and add nothing
    RowEval<PER> r;
    eval_row<LANES, PER, LOGITS>(a, row, sub, true, r);
    const bool counted = live && r.cls == ROW_COUNTED;
    if (counted) {
#pragma unroll
      for (int j = 0; j < PER; ++j) {
        const int k = j * LANES + sub;   // k < C, side < 2, q < K: inside hist
        if (k < C) atomicAdd(&a.state[((size_t)k * 2 + (k == r.y ? 1 : 0)) * (size_t)K + (size_t)sc_q(r.p[j], K)], 1ull);
      }
      if (sub == 0) {   // rank < C, bin < M
        atomicAdd(&rank[r.rank], 1ull);
        unsigned long long* __restrict__ cb = cal + 3 * sc_bin(r.conf, a.M);
        atomicAdd(&cb[0], 1ull);
        if (r.pred == r.y) atomicAdd(&cb[1], 1ull);
        atomicAdd(&cb[2], (unsigned long long)qt_conf_q(r.conf));
      }
    }
    qt_count_rows<4>(live && sub == 0 ? r.cls : ROW_NONE, cnt);
  }
  __syncthreads();
  unsigned long long* __restrict__ ctr = cal + 3 * a.M;
  if (threadIdx.x < 4 && cnt[threadIdx.x]) atomicAdd(&ctr[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
  if (threadIdx.x == 4 && blockIdx.x == 0) atomicAdd(&ctr[4], 1ull);
}

template <int LANES, int PER, bool LOGITS>
__global__ __launch_bounds__(SC_THREADS) void scores_private_kernel(ScArgs a) {
  constexpr int RPB = SC_THREADS / LANES;
  extern __shared__ unsigned sc_lds[];   // hist[2][K], then rank[SC_MAX_C], cal[SC_MAX_M][3], cnt[4]
  const int C = a.C, K = a.K, kc = blockIdx.y;
  const bool tally = kc == 0;
  unsigned* hist = sc_lds;
  unsigned* rank_l = hist + 2 * K;
  unsigned* cal_l = rank_l + SC_MAX_C;
  unsigned* cnt = cal_l + 3 * SC_MAX_M;
  for (int i = threadIdx.x; i < 2 * K + SC_TALLY_WORDS; i += SC_THREADS) sc_lds[i] = 0u;
  __syncthreads();

  const int sub = threadIdx.x & (LANES - 1);
  const long long r0 = (long long)blockIdx.x * SC_SLICE;
  const long long rend = min(a.rows, r0 + SC_SLICE);   // r0 < rows by the grid's size
  for (long long base = r0; base < rend; base += RPB) {   // uniform per workgroup
    const long long row0 = base + threadIdx.x / LANES;
    const bool live = row0 < rend;
    const long long row = live ? row0 : rend - 1;
    RowEval<PER> r;
    eval_row<LANES, PER, LOGITS>(a, row, sub, tally, r);
    const bool counted = live && r.cls == ROW_COUNTED;
    if (counted && (LANES == 1 || sub == (kc & (LANES - 1)))) {   // the lane that holds p[kc]
      float pk = 0.f;
#pragma unroll
      for (int j = 0; j < PER; ++j)
        if (j * LANES + sub == kc) pk = r.p[j];
      atomicAdd(&hist[(kc == r.y ? K : 0) + sc_q(pk, K)], 1u);
    }
    if (tally) {
      if (counted && sub == 0) {
        atomicAdd(&rank_l[r.rank], 1u);
        unsigned* cb = cal_l + 3 * sc_bin(r.conf, a.M);
        atomicAdd(&cb[0], 1u);
        if (r.pred == r.y) atomicAdd(&cb[1], 1u);
        atomicAdd(&cb[2], (unsigned)qt_conf_q(r.conf));
      }
      qt_count_rows<4>(live && sub == 0 ? r.cls : ROW_NONE, cnt);
    }
  }
  __syncthreads();

  unsigned long long* __restrict__ gh = a.state + (size_t)kc * 2 * (size_t)K;
  for (int i = threadIdx.x; i < 2 * K; i += SC_THREADS) {
    const unsigned v = hist[i];
    if (v) atomicAdd(&gh[i], (unsigned long long)v);
  }
  if (tally) {
    unsigned long long* __restrict__ rank = a.state + sc_hist_cells(C, K);
    unsigned long long* __restrict__ cal = rank + C;
    unsigned long long* __restrict__ ctr = cal + 3 * a.M;
    for (int i = threadIdx.x; i < C; i += SC_THREADS)
      if (rank_l[i]) atomicAdd(&rank[i], (unsigned long long)rank_l[i]);
    for (int i = threadIdx.x; i < 3 * a.M; i += SC_THREADS)
      if (cal_l[i]) atomicAdd(&cal[i], (unsigned long long)cal_l[i]);
    if (threadIdx.x < 4 && cnt[threadIdx.x]) atomicAdd(&ctr[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
    if (threadIdx.x == 4 && blockIdx.x == 0) atomicAdd(&ctr[4], 1ull);
  }
}

// ---- finalize -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long shfl_up_u64(unsigned long long v, int d) {
  const unsigned lo = __shfl_up((unsigned)v, d, 64), hi = __shfl_up((unsigned)(v >> 32), d, 64);
  return ((unsigned long long)hi << 32) | lo;
}
// Exclusive prefix sum of one u64 per thread over the workgroup, and the total in every thread: an inclusive scan inside
// each wave, then the four wave totals through LDS.  Integers: any order gives these values.
__device__ __forceinline__ unsigned long long block_excl_scan(unsigned long long v, unsigned long long* wtot, unsigned long long& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long o = shfl_up_u64(inc, d);
    if (lane >= d) inc += o;
  }
  __syncthreads();   // the previous call's readers are done
  if (lane == 63) wtot[wave] = inc;
  __syncthreads();
  unsigned long long before = 0ull;
  total = 0ull;
#pragma unroll
  for (int w = 0; w < SC_THREADS / 64; ++w) {
    if (w < wave) before += wtot[w];
    total += wtot[w];
  }
  return before + inc - v;
}
__device__ __forceinline__ double sc_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// report: [0, C) auc, [C, 2C) average precision, [2C, 3C) support, [3C, 4C) top-k, [4C, 4C + 3M) calibration count /
// accuracy / confidence, then the twelve scalars
__global__ __launch_bounds__(SC_THREADS) void scores_finalize_kernel(const unsigned long long* __restrict__ state, int C, int K, int M,
                                                                     double* __restrict__ report, long long* __restrict__ curves) {
  __shared__ unsigned long long wtot[SC_THREADS / 64];
  __shared__ double red[SC_THREADS];
  const int t = threadIdx.x;
  const unsigned long long* __restrict__ rank = state + sc_hist_cells(C, K);
  const unsigned long long* __restrict__ cal = rank + C;
  const unsigned long long* __restrict__ ctr = cal + 3 * M;
  double* __restrict__ scal = report + 4 * (size_t)C + 3 * (size_t)M;

  if ((int)blockIdx.x == C) {   // ranks, calibration, counters
    __shared__ unsigned long long rk[SC_MAX_C];
    __shared__ double gap[SC_MAX_M], wgt[SC_MAX_M];
    const unsigned long long counted = ctr[0];
    if (t < C) rk[t] = rank[t];
    if (t < M) {
      const unsigned long long n = cal[3 * t], hit = cal[3 * t + 1], cs = cal[3 * t + 2];
      const double acc = n ? (double)hit / (double)n : 0.0;
      const double conf = n ? (double)cs / (65536.0 * (double)n) : 0.0;
      report[4 * C + t] = (double)n;
      report[4 * C + M + t] = acc;
      report[4 * C + 2 * M + t] = conf;
      gap[t] = fabs(acc - conf);
      wgt[t] = (double)n;
    }
    __syncthreads();
    if (t == 0) {
      unsigned long long cum = 0ull;
      for (int k = 0; k < C; ++k) {
        cum += rk[k];
        report[3 * C + k] = counted ? (double)cum / (double)counted : sc_nan();
      }
      double n = 0.0, ece = 0.0, mce = 0.0;
      for (int b = 0; b < M; ++b) n += wgt[b];   // integers below 2^53: exact
      for (int b = 0; b < M; ++b)                // bins in ascending order
        if (wgt[b] > 0.0) {
          ece += (wgt[b] / n) * gap[b];
          mce = fmax(mce, gap[b]);
        }
      scal[4] = n > 0.0 ? ece : sc_nan();
      scal[5] = n > 0.0 ? mce : sc_nan();
      scal[6] = (double)counted;
      scal[7] = (double)ctr[1];
      scal[8] = (double)ctr[2];
      scal[9] = (double)ctr[3];
      scal[11] = (double)ctr[4];
    }
    return;
  }

  // class k: thread t owns bins [t per, (t + 1) per)
  const int k = blockIdx.x;
  const unsigned long long* __restrict__ neg = state + (size_t)k * 2 * (size_t)K;
  const unsigned long long* __restrict__ pos = neg + K;
  const int per = K >= SC_THREADS ? K / SC_THREADS : 1;
  const int b0 = t * per, b1 = b0 < K ? b0 + per : b0;   // threads past the last bin own nothing
  unsigned long long sp = 0ull, sn = 0ull;
  for (int b = b0; b < b1; ++b) {
    sp += pos[b];
    sn += neg[b];
  }
  unsigned long long P, N;
  const unsigned long long pb = block_excl_scan(sp, wtot, P);   // positives / negatives in the bins below b0
  const unsigned long long nb = block_excl_scan(sn, wtot, N);

  // A2 = sum_b pos_b (2 negbelow_b + neg_b), and the cumulative curves tp_b = P - posbelow_b, fp_b = N - negbelow_b
  unsigned long long a2 = 0ull, pbelow = pb, nbelow = nb;
  long long* __restrict__ cv = curves ? curves + (size_t)k * 2 * (size_t)K : nullptr;
  for (int b = b0; b < b1; ++b) {
    const unsigned long long p = pos[b], n = neg[b];
    a2 += p * (2ull * nbelow + n);
    if (cv) {
      cv[b] = (long long)(P - pbelow);
      cv[K + b] = (long long)(N - nbelow);
    }
    pbelow += p;
    nbelow += n;
  }
  unsigned long long A2;
  block_excl_scan(a2, wtot, A2);
  // average precision: this thread's bins from the top down, then the tree over the threads
  double ap = 0.0;
  for (int b = b1 - 1; b >= b0; --b) {
    const unsigned long long p = pos[b];
    pbelow -= p;
    nbelow -= neg[b];
    if (p) {
      const double tp = (double)(P - pbelow), fp = (double)(N - nbelow);
      ap += ((double)p / (double)P) * (tp / (tp + fp));
    }
  }
  ap = qt_block_sum<SC_THREADS>(ap, red);
  if (t == 0) {
    report[k] = P && N ? (double)A2 / (double)(2ull * P * N) : sc_nan();
    report[C + k] = P ? ap : sc_nan();
    report[2 * C + k] = (double)P;
  }
}

// macro and support-weighted averages over the classes whose value is defined, classes in ascending order
__global__ __launch_bounds__(64) void scores_average_kernel(int C, int M, double* __restrict__ report) {
  if (threadIdx.x != 0) return;
  double* __restrict__ scal = report + 4 * (size_t)C + 3 * (size_t)M;
  double ma = 0.0, wa = 0.0, sa = 0.0, na = 0.0, mp = 0.0, wp = 0.0, sp = 0.0, np = 0.0;
  for (int k = 0; k < C; ++k) {
    const double auc = report[k], ap = report[C + k], s = report[2 * C + k];
    if (auc == auc) {
      ma += auc;
      wa += s * auc;
      sa += s;
      na += 1.0;
    }
    if (ap == ap) {
      mp += ap;
      wp += s * ap;
      sp += s;
      np += 1.0;
    }
  }
  scal[0] = na > 0.0 ? ma / na : sc_nan();
  scal[1] = na > 0.0 ? wa / sa : sc_nan();
  scal[2] = np > 0.0 ? mp / np : sc_nan();
  scal[3] = np > 0.0 ? wp / sp : sc_nan();
  scal[10] = na;
}

inline bool sizes_ok(int C, int bits, int M) {
  return C >= 1 && C <= SC_MAX_C && bits >= SC_MIN_BITS && bits <= SC_MAX_BITS && M >= 1 && M <= SC_MAX_M;
}

template <int LANES, int PER, bool LOGITS>
int launch_update(const ScArgs& a, bool privatised, hipStream_t s) {
  if (privatised) {
    const int lds = (2 * a.K + SC_TALLY_WORDS) * (int)sizeof(unsigned);
    static std::atomic<unsigned long long> raised{0};
    if (lds > 48 * 1024)
      if (int rc = qt_raise_lds_limit((const void*)scores_private_kernel<LANES, PER, LOGITS>, lds, raised)) return rc;
    const dim3 grid((unsigned)((a.rows + SC_SLICE - 1) / SC_SLICE), (unsigned)a.C);
    hipLaunchKernelGGL((scores_private_kernel<LANES, PER, LOGITS>), grid, dim3(SC_THREADS), lds, s, a);
  } else {
    const dim3 grid((unsigned)qt_grid_for(a.rows, SC_THREADS / LANES, SC_MAX_BLOCKS));
    hipLaunchKernelGGL((scores_direct_kernel<LANES, PER, LOGITS>), grid, dim3(SC_THREADS), 0, s, a);
  }
  QT_CHECK_LAUNCH();
  return QT_OK;
}

}  // namespace

extern "C" size_t qt_scores_state_bytes(int C, int bits, int cal_bins) {
  if (!sizes_ok(C, bits, cal_bins)) return 0;
  return sizeof(unsigned long long) * (sc_hist_cells(C, 1 << bits) + (size_t)C + 3 * (size_t)cal_bins + SC_COUNTERS);
}

extern "C" size_t qt_scores_report_bytes(int C, int cal_bins) {
  if (!sizes_ok(C, SC_MIN_BITS, cal_bins)) return 0;
  return sizeof(double) * (4 * (size_t)C + 3 * (size_t)cal_bins + SC_SCALARS);
}

extern "C" int qt_scores_update(const qt_scores_desc* desc, const float* scores, long long ld, const long long* labels,
                                long long rows, int C, unsigned long long* state, void* stream) {
  QT_CHECK_ARG(desc, "qt_scores_update: null descriptor");
  if (desc->dtype != QT_F32) {
    qt_set_error("qt_scores_update: f32 scores only (dtype %d)", desc->dtype);
    return QT_ERR_UNSUPPORTED;
  }
  QT_CHECK_ARG(desc->kind == QT_SCORES_LOGITS || desc->kind == QT_SCORES_PROBS, "qt_scores_update: kind %d is neither logits nor probs",
               desc->kind);
  QT_CHECK_ARG(desc->bits >= SC_MIN_BITS && desc->bits <= SC_MAX_BITS, "qt_scores_update: bits = %d outside %d .. %d", desc->bits,
               SC_MIN_BITS, SC_MAX_BITS);
  QT_CHECK_ARG(desc->cal_bins >= 1 && desc->cal_bins <= SC_MAX_M, "qt_scores_update: cal_bins = %d outside 1 .. %d", desc->cal_bins,
               SC_MAX_M);
  QT_CHECK_ARG(desc->route >= QT_SCORES_ROUTE_AUTO && desc->route <= QT_SCORES_ROUTE_PRIVATE, "qt_scores_update: route %d outside 0 .. 2",
               desc->route);
  QT_CHECK_ARG(scores && labels && state, "qt_scores_update: null scores / labels / state");
  if (int rc = qt_check_rows_classes("qt_scores_update", rows, C, SC_MAX_C, SC_MAX_ROWS)) return rc;
  QT_CHECK_ARG(ld >= C, "qt_scores_update: row stride %lld < C = %d", ld, C);
  QT_CHECK_ARG(!misaligned(scores, 3) && !misaligned(labels, 7) && !misaligned(state, 7),
               "qt_scores_update: scores must be 4-byte aligned, labels and state 8-byte");

  ScArgs a;
  a.s = scores;
  a.y = labels;
  a.rows = rows;
  a.ld = ld;
  a.C = C;
  a.K = 1 << desc->bits;
  a.M = desc->cal_bins;
  a.ignore_index = desc->ignore_index;
  a.state = state;
  const bool privatised = desc->route == QT_SCORES_ROUTE_AUTO ? rows >= QT_SCORES_AUTO_PRIVATE_ROWS : desc->route == QT_SCORES_ROUTE_PRIVATE;
  const bool logits = desc->kind == QT_SCORES_LOGITS;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return qt_by_row_lanes<SC_MAX_C>(C, [&](auto L, auto P) {
    constexpr int LANES = decltype(L)::value, PER = decltype(P)::value;
    return logits ? launch_update<LANES, PER, true>(a, privatised, s) : launch_update<LANES, PER, false>(a, privatised, s);
  });
}

extern "C" int qt_scores_finalize(const unsigned long long* state, int C, int bits, int cal_bins, double* report, long long* curves,
                                  void* stream) {
  QT_CHECK_ARG(state && report, "qt_scores_finalize: null state / report");
  QT_CHECK_ARG(C >= 1, "qt_scores_finalize: needs C >= 1 (got %d)", C);
  if (int rc = qt_check_class_cap("qt_scores_finalize", C, SC_MAX_C)) return rc;
  QT_CHECK_ARG(bits >= SC_MIN_BITS && bits <= SC_MAX_BITS, "qt_scores_finalize: bits = %d outside %d .. %d", bits, SC_MIN_BITS, SC_MAX_BITS);
  QT_CHECK_ARG(cal_bins >= 1 && cal_bins <= SC_MAX_M, "qt_scores_finalize: cal_bins = %d outside 1 .. %d", cal_bins, SC_MAX_M);
  QT_CHECK_ARG(!misaligned(state, 7) && !misaligned(report, 7) && !misaligned(curves, 7),
               "qt_scores_finalize: state, report and curves must be 8-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(scores_finalize_kernel, dim3((unsigned)C + 1), dim3(SC_THREADS), 0, s, state, C, 1 << bits, cal_bins, report, curves);
  QT_CHECK_LAUNCH();
  hipLaunchKernelGGL(scores_average_kernel, dim3(1), dim3(64), 0, s, C, cal_bins, report);
  QT_CHECK_LAUNCH();
  return QT_OK;
}
