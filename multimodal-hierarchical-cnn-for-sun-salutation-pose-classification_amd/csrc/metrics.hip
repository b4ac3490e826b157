// Evaluation report on the device (qt_metrics_update / qt_metrics_finalize): the confusion matrix and the per-frame
// softmax confidence the reference's scripts build on the host (comparative analysis/analysis.py:60-109 copies labels and
// predictions to the CPU every batch and calls scikit-learn; experiment/test_on_video_cnn.py:274-278 reads softmax, its
// maximum and .item() per frame).  The state is additive integer counts that stay in device memory for a whole evaluation:
//     state[C*C + 4] u64 = { cm[label][pred] ..., rows counted, rows ignored, rows invalid, update calls }
// and one finalize launch turns it into the report (precision / recall / F1 / support per class, accuracy, weighted and
// macro averages, R^2 of label index against predicted index) in double.
//
// Update, one launch per batch.  Rows map to lanes by qt_rowgroup.h's rule (LANES lanes own one row, element k sits in lane
// k % LANES): one thread per row for C <= 16, a 16-lane DPP row for C <= 64, a wave above; the argmax is qt_row_argmax (a NaN
// beats every number, then the larger value, then the lower index), loss.hip's too, so pred is what qt_loss_forward writes.
// A workgroup walks row tiles with a grid stride.  Counting is exact in any order of execution because every add is an
// integer atomic:
//     C <= 64   the workgroup's own u32 histogram of C*C cells in LDS (16 KiB), LDS atomics per row, then one 64-bit global
//               atomic per non-zero cell when the workgroup is done;
//     C  > 64   one 64-bit global atomic per counted row.
// The three row counters go through ballots (one LDS atomic per wave and tile) and leave with the flush.
// Probabilities (all f32): m = z[argmax], e_k = expf(z_k - m), s = sum_k e_k, p_k = e_k / s; confidence is the p_k of the
// lane that owns the argmax, i.e. the very value stored to probs[pred].  A NaN or +inf logit (and a row of -inf) makes m or
// z_k - m NaN, so the whole row is NaN by IEEE rules, which is what torch.softmax gives on the CPU.
#include <math.h>
#include <stdint.h>

#include "qt_common.h"
#include "qt_rowgroup.h"

namespace {

constexpr int MET_THREADS = 256;
constexpr int MET_MAX_C = QT_METRICS_MAX_CLASSES;
constexpr int MET_LDS_C = 64;                  // largest C whose C*C u32 histogram is kept in LDS
constexpr long long MET_MAX_ROWS = 1ll << 22;
constexpr int MET_MAX_BLOCKS = 2048;           // grid-stride cap: 8 workgroups per CU
constexpr int MET_SCALARS = 12;

struct MetArgs {
  const float* z;                 // [rows][ld] or NULL
  const long long* pred_in;       // [rows] or NULL
  const long long* y;             // [rows] or NULL
  long long rows, ld, ld_p;
  int C;
  long long ignore_index;
  unsigned long long* state;      // [C*C + 4] or NULL
  float* probs;                   // [rows][ld_p] or NULL
  float* conf;                    // [rows] or NULL
  long long* pred_out;            // [rows] or NULL
};

// ---- counting ---------------------------------------------------------------------------------------------------------
enum { ROW_COUNTED = 0, ROW_IGNORED = 1, ROW_INVALID = 2, ROW_NONE = 3 };

// One row per calling lane (`active` lanes only).  Every lane of the wave must call it: the counters use ballots.
template <bool LDS_HIST>
__device__ __forceinline__ void tally(bool active, long long y, long long p, const MetArgs& a, unsigned* hist, unsigned* cnt) {
  int cls = ROW_NONE;
  if (active) {
    if (y == a.ignore_index) cls = ROW_IGNORED;
    else if (y < 0 || y >= (long long)a.C || p < 0 || p >= (long long)a.C) cls = ROW_INVALID;
    else cls = ROW_COUNTED;
  }
  if (cls == ROW_COUNTED) {   // both indices are inside [0, C) here and nowhere else
    if (LDS_HIST) atomicAdd(&hist[(int)y * a.C + (int)p], 1u);
    else atomicAdd(&a.state[(unsigned long long)y * (unsigned)a.C + (unsigned long long)p], 1ull);
  }
  qt_count_rows<3>(cls, cnt);
}

template <bool LDS_HIST> __device__ __forceinline__ void tally_begin(const MetArgs& a, unsigned* hist, unsigned* cnt) {
  if (LDS_HIST)
    for (int i = threadIdx.x; i < a.C * a.C; i += MET_THREADS) hist[i] = 0u;
  if (threadIdx.x < 3) cnt[threadIdx.x] = 0u;
  __syncthreads();
}
template <bool LDS_HIST> __device__ __forceinline__ void tally_end(const MetArgs& a, const unsigned* hist, const unsigned* cnt) {
  __syncthreads();
  const int cells = a.C * a.C;
  if (LDS_HIST)
    for (int i = threadIdx.x; i < cells; i += MET_THREADS) {
      const unsigned v = hist[i];
      if (v) atomicAdd(&a.state[i], (unsigned long long)v);
    }
  if (threadIdx.x < 3 && cnt[threadIdx.x]) atomicAdd(&a.state[cells + threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
  if (threadIdx.x == 3 && blockIdx.x == 0) atomicAdd(&a.state[cells + 3], 1ull);
}

template <int LANES, int PER>
__global__ __launch_bounds__(MET_THREADS) void metrics_logits_kernel(MetArgs a) {
  constexpr int RPB = MET_THREADS / LANES;
  constexpr bool LDS_HIST = LANES < 64;
  __shared__ unsigned hist[LDS_HIST ? MET_LDS_C * MET_LDS_C : 1];
  __shared__ unsigned cnt[3];
  const bool counting = a.state != nullptr;
  if (counting) tally_begin<LDS_HIST>(a, hist, cnt);

  const int sub = threadIdx.x & (LANES - 1);
  const int C = a.C;
  const bool want_p = a.probs != nullptr || a.conf != nullptr;
  const long long tiles = (a.rows + RPB - 1) / RPB;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {   // uniform per workgroup: no divergence around shuffles
    const long long row0 = tile * RPB + threadIdx.x / LANES;
    const bool live = row0 < a.rows;
    const long long row = live ? row0 : a.rows - 1;   // idle lanes repeat the last row and store nothing
    const float* __restrict__ zr = a.z + row * a.ld;

    float z[PER];
    qt_row_load<LANES, PER>(zr, C, sub, z);
    float bv;   // argmax = torch.max(outputs, 1): first index of the maximum, a NaN wins
    int bi;
    qt_row_argmax<LANES, PER>(z, C, sub, bv, bi);
    const bool writer = live && sub == 0;

    if (want_p) {
      qt_row_softmax<LANES, PER>(z, C, sub, bv);
      float conf_l = 0.f;
      float* __restrict__ pr = a.probs ? a.probs + row * a.ld_p : nullptr;
#pragma unroll
      for (int j = 0; j < PER; ++j) {
        const int k = j * LANES + sub;
        if (k < C) {
          if (pr && live) pr[k] = z[j];
          if (k == bi) conf_l = z[j];
        }
      }
      const float conf = qt_group_pick<LANES>(conf_l, bi & (LANES - 1));
      if (writer && a.conf) a.conf[row] = conf;
    }
    if (writer && a.pred_out) a.pred_out[row] = (long long)bi;
    if (counting) tally<LDS_HIST>(writer, a.y[row], (long long)bi, a, hist, cnt);
  }
  if (counting) tally_end<LDS_HIST>(a, hist, cnt);
}

// Counting from given predictions: one thread per row.
template <bool LDS_HIST>
__global__ __launch_bounds__(MET_THREADS) void metrics_pred_kernel(MetArgs a) {
  __shared__ unsigned hist[LDS_HIST ? MET_LDS_C * MET_LDS_C : 1];
  __shared__ unsigned cnt[3];
  tally_begin<LDS_HIST>(a, hist, cnt);
  for (long long r0 = (long long)blockIdx.x * MET_THREADS; r0 < a.rows; r0 += (long long)gridDim.x * MET_THREADS) {
    const long long row = r0 + threadIdx.x;
    const bool live = row < a.rows;
    const long long y = live ? a.y[row] : 0;
    const long long p = live ? a.pred_in[row] : 0;
    tally<LDS_HIST>(live, y, p, a, hist, cnt);
  }
  tally_end<LDS_HIST>(a, hist, cnt);
}

// ---- finalize: one workgroup, counts added as integers (exact), everything else in double --------------------------------
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const unsigned lo = __shfl_xor((unsigned)v, s, 64);
    const unsigned hi = __shfl_xor((unsigned)(v >> 32), s, 64);
    v += ((unsigned long long)hi << 32) | lo;
  }
  return v;
}

__global__ __launch_bounds__(MET_THREADS) void metrics_finalize_kernel(const unsigned long long* __restrict__ state, int C,
                                                                       double* __restrict__ report) {
  __shared__ unsigned long long sup[MET_MAX_C];    // row sums: samples whose label is i
  __shared__ unsigned long long prd[MET_MAX_C];    // column sums: samples predicted as j
  __shared__ unsigned long long dia[MET_MAX_C];
  __shared__ double red[MET_THREADS];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  constexpr int PER = MET_MAX_C / 64;
  for (int k = t; k < C; k += MET_THREADS) prd[k] = 0ull;
  __syncthreads();

  // one wave per matrix row: lanes stride over the columns
  unsigned long long col[PER];
#pragma unroll
  for (int q = 0; q < PER; ++q) col[q] = 0ull;
  double ss_res = 0.0;
  for (int i = wave; i < C; i += MET_THREADS / 64) {
    const unsigned long long* __restrict__ r = state + (size_t)i * C;
    unsigned long long rs = 0ull;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int j = q * 64 + lane;
      if (j < C) {
        const unsigned long long v = r[j];
        rs += v;
        col[q] += v;
        const double d = (double)(i - j);
        ss_res += (double)v * (d * d);
        if (j == i) dia[i] = v;
      }
    }
    rs = wave_sum_u64(rs);
    if (lane == 0) sup[i] = rs;
  }
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    const int j = q * 64 + lane;
    if (j < C && col[q]) atomicAdd(&prd[j], col[q]);
  }
  __syncthreads();

  // per class (thread t owns classes t, t + 256, ..)
  double wp = 0.0, wr = 0.0, wf = 0.0, mp = 0.0, mr = 0.0, mf = 0.0, present = 0.0, correct = 0.0, n = 0.0, isum = 0.0;
  for (int k = t; k < C; k += MET_THREADS) {
    const double tp = (double)dia[k], s = (double)sup[k], p = (double)prd[k];
    const double pk = p > 0.0 ? tp / p : 0.0;
    const double rk = s > 0.0 ? tp / s : 0.0;
    const double fk = s + p > 0.0 ? 2.0 * tp / (s + p) : 0.0;
    report[k] = pk;
    report[C + k] = rk;
    report[2 * C + k] = fk;
    report[3 * C + k] = s;
    wp += s * pk;
    wr += s * rk;
    wf += s * fk;
    if (s + p > 0.0) {
      mp += pk;
      mr += rk;
      mf += fk;
      present += 1.0;
    }
    correct += tp;
    n += s;
    isum += s * (double)k;
  }
  wp = qt_block_sum<MET_THREADS>(wp, red);
  wr = qt_block_sum<MET_THREADS>(wr, red);
  wf = qt_block_sum<MET_THREADS>(wf, red);
  mp = qt_block_sum<MET_THREADS>(mp, red);
  mr = qt_block_sum<MET_THREADS>(mr, red);
  mf = qt_block_sum<MET_THREADS>(mf, red);
  present = qt_block_sum<MET_THREADS>(present, red);
  correct = qt_block_sum<MET_THREADS>(correct, red);
  n = qt_block_sum<MET_THREADS>(n, red);
  isum = qt_block_sum<MET_THREADS>(isum, red);
  ss_res = qt_block_sum<MET_THREADS>(ss_res, red);
  const double mean = n > 0.0 ? isum / n : 0.0;
  double ss_tot = 0.0;
  for (int k = t; k < C; k += MET_THREADS) {
    const double d = (double)k - mean;
    ss_tot += (double)sup[k] * (d * d);
  }
  ss_tot = qt_block_sum<MET_THREADS>(ss_tot, red);
  if (t == 0) {
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double* __restrict__ o = report + 4 * (size_t)C;
    const bool any = n > 0.0;
    o[0] = any ? correct / n : nan;
    o[1] = any ? wp / n : nan;
    o[2] = any ? wr / n : nan;
    o[3] = any ? wf / n : nan;
    o[4] = any ? mp / present : nan;
    o[5] = any ? mr / present : nan;
    o[6] = any ? mf / present : nan;
    double r2 = nan;
    if (n >= 2.0) r2 = ss_tot != 0.0 ? 1.0 - ss_res / ss_tot : (ss_res == 0.0 ? 1.0 : 0.0);
    o[7] = r2;
    o[8] = n;
    o[9] = (double)state[(size_t)C * C + 1];
    o[10] = (double)state[(size_t)C * C + 2];
    o[11] = present;
  }
}

}  // namespace

extern "C" size_t qt_metrics_state_bytes(int C) {
  if (C < 1 || C > MET_MAX_C) return 0;
  return sizeof(unsigned long long) * ((size_t)C * C + 4);
}

extern "C" size_t qt_metrics_report_bytes(int C) {
  if (C < 1 || C > MET_MAX_C) return 0;
  return sizeof(double) * (4 * (size_t)C + MET_SCALARS);
}

extern "C" int qt_metrics_update(const qt_metrics_desc* desc, const float* logits, long long ld, const long long* pred_in,
                                 const long long* labels, long long rows, int C, unsigned long long* state, float* probs,
                                 long long ld_probs, float* confidence, long long* pred_out, void* stream) {
  QT_CHECK_ARG(desc, "qt_metrics_update: null descriptor");
  if (desc->dtype != QT_F32) {
    qt_set_error("qt_metrics_update: f32 logits only (dtype %d)", desc->dtype);
    return QT_ERR_UNSUPPORTED;
  }
  QT_CHECK_ARG((logits != nullptr) != (pred_in != nullptr), "qt_metrics_update: exactly one of logits and pred_in must be given");
  QT_CHECK_ARG(logits || (!probs && !confidence && !pred_out),
               "qt_metrics_update: probs / confidence / pred_out need logits (predictions are only counted)");
  QT_CHECK_ARG((labels != nullptr) == (state != nullptr), "qt_metrics_update: labels and state go together (got %s only)",
               labels ? "labels" : "a state");
  QT_CHECK_ARG(state || probs || confidence || pred_out, "qt_metrics_update: nothing to produce (no state and no output)");
  if (int rc = qt_check_rows_classes("qt_metrics_update", rows, C, MET_MAX_C, MET_MAX_ROWS)) return rc;
  QT_CHECK_ARG(!logits || ld >= C, "qt_metrics_update: row stride %lld < C = %d", ld, C);
  QT_CHECK_ARG(!probs || ld_probs >= C, "qt_metrics_update: probs row stride %lld < C = %d", ld_probs, C);
  QT_CHECK_ARG(!misaligned(logits, 3) && !misaligned(probs, 3) && !misaligned(confidence, 3) && !misaligned(pred_in, 7) &&
                   !misaligned(labels, 7) && !misaligned(state, 7) && !misaligned(pred_out, 7),
               "qt_metrics_update: f32 buffers must be 4-byte aligned, pred_in / labels / state / pred_out 8-byte");

  hipStream_t s = static_cast<hipStream_t>(stream);
  MetArgs a;
  a.z = logits;
  a.pred_in = pred_in;
  a.y = labels;
  a.rows = rows;
  a.ld = ld;
  a.ld_p = ld_probs;
  a.C = C;
  a.ignore_index = desc->ignore_index;
  a.state = state;
  a.probs = probs;
  a.conf = confidence;
  a.pred_out = pred_out;
  if (logits) {
    const dim3 grid((unsigned)qt_grid_for(rows, MET_THREADS / qt_row_lanes(C), MET_MAX_BLOCKS));
    qt_by_row_lanes<MET_MAX_C>(C, [&](auto L, auto P) {
      hipLaunchKernelGGL((metrics_logits_kernel<decltype(L)::value, decltype(P)::value>), grid, dim3(MET_THREADS), 0, s, a);
    });
  } else {
    const dim3 grid((unsigned)qt_grid_for(rows, MET_THREADS, MET_MAX_BLOCKS));
    if (C <= MET_LDS_C) hipLaunchKernelGGL(metrics_pred_kernel<true>, grid, dim3(MET_THREADS), 0, s, a);
    else hipLaunchKernelGGL(metrics_pred_kernel<false>, grid, dim3(MET_THREADS), 0, s, a);
  }
  QT_CHECK_LAUNCH();
  return QT_OK;
}

extern "C" int qt_metrics_finalize(const unsigned long long* state, int C, double* report, void* stream) {
  QT_CHECK_ARG(state && report, "qt_metrics_finalize: null state / report");
  QT_CHECK_ARG(C >= 1, "qt_metrics_finalize: needs C >= 1 (got %d)", C);
  if (int rc = qt_check_class_cap("qt_metrics_finalize", C, MET_MAX_C)) return rc;
  QT_CHECK_ARG(!misaligned(state, 7) && !misaligned(report, 7), "qt_metrics_finalize: state and report must be 8-byte aligned");
  hipLaunchKernelGGL(metrics_finalize_kernel, dim3(1), dim3(MET_THREADS), 0, static_cast<hipStream_t>(stream), state, C, report);
  QT_CHECK_LAUNCH();
  return QT_OK;
}
