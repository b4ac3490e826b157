// Loss head on the device (qt_loss_forward / qt_loss_backward): cross-entropy with torch.nn.functional.cross_entropy
// semantics (class weights, label smoothing, ignore_index, mean / sum / none) and the focal loss of the reference
// (3dcnn/models.py:8-47), plus the trainers' per-step bookkeeping (argmax, correct count, running epoch meter), so a train
// step needs no torch kernel between the forward and the backward and no device-to-host read
// (3dcnn/train_3D_Quadtree_cnn_model.py:127-137 reads loss.item() and (predicted == labels).sum().item() every step).
//
// A latency problem (256 x 12 floats), so: one launch per direction whenever the batch fits one workgroup; no atomics, no
// zero fill, every summation order fixed -> the same bits on every run; nothing allocated, nothing synchronised.
//
// Row-to-lane mapping by class count C (qt_rowgroup.h: LANES lanes own one row, each keeps PER logits in registers, element
// k of the row sits in lane k % LANES):
//     C <= 16    one thread per row           256 rows per workgroup
//     C <= 64    one 16-lane DPP row per row    16 rows per workgroup
//     C <= 1024  one wave per row                4 rows per workgroup
// Above one workgroup's reach every workgroup writes {numerator, denominator, correct} as doubles to its own workspace slot
// and a one-workgroup finalize adds the slots in a fixed order; it also owns the meter update.
//
// Per row (all f32):  a = argmax (first index wins a tie, a NaN wins the row), m = z[a], d_k = z_k - m,
//   l = log1pf(sum_{k != a} expf(d_k))              -- log-sum-exp minus m; the maximum's own exp(0) = 1 is never added, so
//   -log p_y = l - d_y                                 a saturated row keeps its digits; m + l is never formed, so a common
//   1 - p_y  = -expm1f(d_y - l)                        shift of the logits costs nothing
// The row state the backward reads is {m, l}.  Cross-row sums are added in double.
#include <math.h>
#include <stdint.h>

#include "qt_common.h"
#include "qt_rowgroup.h"

namespace {

constexpr int LOSS_THREADS = 256;
constexpr int LOSS_MAX_C = 1024;

struct LossArgs {
  const float* z;            // [rows][ld]
  const long long* y;        // [rows]
  const float* w;            // [C] or NULL
  long long rows, ld;
  int C, kind, reduction;
  long long ignore_index;
  float eps, gamma;
};

__device__ __forceinline__ float loss_nan() { return __uint_as_float(0x7fc00000u); }

// Sum of one double per thread over the workgroup, fixed order: thread t adds slot t + s for s = 128, 64, .. 1.
// Thread 0 holds the result.
__device__ __forceinline__ void block_sum3(double& a, double& b, double& c) {
  __shared__ double red[3][LOSS_THREADS];
  const int t = threadIdx.x;
  red[0][t] = a;
  red[1][t] = b;
  red[2][t] = c;
  __syncthreads();
#pragma unroll
  for (int s = LOSS_THREADS / 2; s >= 1; s >>= 1) {
    if (t < s) {
      red[0][t] += red[0][t + s];
      red[1][t] += red[1][t + s];
      red[2][t] += red[2][t + s];
    }
    __syncthreads();
  }
  a = red[0][0];
  b = red[1][0];
  c = red[2][0];
}

// (1 - p)^(gamma - 1) for gamma >= 1; gamma = 1 and 2 need no powf
__device__ __forceinline__ float focal_pow_m1(float om, float gamma) {
  if (gamma == 1.f) return 1.f;
  if (gamma == 2.f) return om;
  return powf(om, gamma - 1.f);
}

// What one thread does after the cross-row sums are known: the reduced loss, the stats block, the meter.
__device__ __forceinline__ void loss_finish(double num, double den, double correct, long long rows, int kind, int reduction,
                                            float* __restrict__ loss, double* __restrict__ stats, double* __restrict__ meter) {
  if (reduction != QT_LOSS_REDUCE_MEAN) den = 1.0;
  else if (kind == QT_LOSS_FOCAL) den = (double)rows;
  const float reduced = (float)(num / den);     // mean over nothing: 0 / 0 = NaN, as torch
  if (reduction != QT_LOSS_REDUCE_NONE) loss[0] = reduced;
  stats[0] = num;
  stats[1] = den;
  stats[2] = correct;
  if (meter) {
    const double add = reduction == QT_LOSS_REDUCE_MEAN ? (double)reduced * (double)rows : (double)reduced;
    if (isfinite(reduced)) {
      meter[0] += add;
      meter[1] += (double)rows;
      meter[2] += correct;
    } else {
      meter[3] += 1.0;
    }
  }
}

template <int LANES, int PER>
__global__ __launch_bounds__(LOSS_THREADS) void loss_fwd_kernel(LossArgs a, float* __restrict__ loss, float2* __restrict__ row_state,
                                                                double* __restrict__ stats, long long* __restrict__ pred,
                                                                double* __restrict__ meter, double* __restrict__ partial) {
  constexpr int RPB = LOSS_THREADS / LANES;
  const int sub = threadIdx.x & (LANES - 1);
  const long long row0 = (long long)blockIdx.x * RPB + threadIdx.x / LANES;
  const bool live = row0 < a.rows;
  const long long row = live ? row0 : a.rows - 1;   // idle lanes repeat the last row and store nothing: no divergence around shuffles
  const float* __restrict__ zr = a.z + row * a.ld;
  const int C = a.C;
  const long long y = a.y[row];

  float z[PER];
  qt_row_load<LANES, PER>(zr, C, sub, z);
  const bool ce = a.kind == QT_LOSS_CROSS_ENTROPY;
  const bool ignored = ce && y == a.ignore_index;
  const bool in_range = y >= 0 && y < (long long)C;
  const bool bad = !ignored && !in_range;           // error row: NaN loss, no indexing with y anywhere

  float m;   // argmax = torch.max(outputs, 1): first index of the maximum, a NaN wins
  int bi;
  qt_row_argmax<LANES, PER>(z, C, sub, m, bi);

  // d_k = z_k - m (kept in z), s1 = sum over k != argmax of exp(d_k), and the label's own d_y / w_y by selection
  float s1 = 0.f, dy_l = 0.f, wy_l = 1.f;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int k = j * LANES + sub;
    if (k < C) {
      z[j] -= m;
      if (k != bi) s1 += expf(z[j]);
      if ((long long)k == y) dy_l = z[j];
    }
  }
  if (a.w) {
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int k = j * LANES + sub;
      if (k < C && (long long)k == y) wy_l = a.w[k];
    }
  }
  s1 = qt_group_sum<LANES>(s1);
  const float l = log1pf(s1);
  const int owner = in_range ? (int)(y & (LANES - 1)) : 0;
  float dy = qt_group_pick<LANES>(dy_l, owner);
  float wy = qt_group_pick<LANES>(wy_l, owner);
  if (bad) dy = wy = loss_nan();

  float li, deni = 0.f;
  if (ce) {
    const float nll = l - dy;
    li = wy * nll;
    deni = wy;
    if (a.eps > 0.f) {
      float sm = 0.f;
#pragma unroll
      for (int j = 0; j < PER; ++j) {
        const int k = j * LANES + sub;
        if (k < C) sm += (a.w ? a.w[k] : 1.f) * (l - z[j]);
      }
      sm = qt_group_sum<LANES>(sm);
      li = (1.f - a.eps) * li + (a.eps / (float)C) * sm;
    }
    if (ignored) li = deni = 0.f;
  } else {
    const float logp = dy - l;
    const float om = fmaxf(-expm1f(logp), 0.f);
    const float mod = a.gamma == 0.f ? 1.f : focal_pow_m1(om, a.gamma) * om;
    li = -wy * mod * logp;
  }
  const bool writer = live && sub == 0;
  if (writer) {
    if (a.reduction == QT_LOSS_REDUCE_NONE) loss[row] = li;
    if (row_state) row_state[row] = make_float2(m, l);
    if (pred) pred[row] = (long long)bi;
  }
  double num = writer ? (double)li : 0.0;
  double den = writer ? (double)deni : 0.0;
  double cor = writer && (long long)bi == y ? 1.0 : 0.0;
  block_sum3(num, den, cor);
  if (threadIdx.x == 0) {
    if (partial) {
      partial[3 * (long long)blockIdx.x + 0] = num;
      partial[3 * (long long)blockIdx.x + 1] = den;
      partial[3 * (long long)blockIdx.x + 2] = cor;
    } else {
      loss_finish(num, den, cor, a.rows, a.kind, a.reduction, loss, stats, meter);
    }
  }
}

__global__ __launch_bounds__(LOSS_THREADS) void loss_finalize_kernel(const double* __restrict__ partial, int count, long long rows,
                                                                     int kind, int reduction, float* __restrict__ loss,
                                                                     double* __restrict__ stats, double* __restrict__ meter) {
  double num = 0.0, den = 0.0, cor = 0.0;
  for (int i = threadIdx.x; i < count; i += LOSS_THREADS) {
    num += partial[3 * (long long)i + 0];
    den += partial[3 * (long long)i + 1];
    cor += partial[3 * (long long)i + 2];
  }
  block_sum3(num, den, cor);
  if (threadIdx.x == 0) loss_finish(num, den, cor, rows, kind, reduction, loss, stats, meter);
}

// dL/dz.  p_k = exp(d_k - l);  p_y - 1 is taken as expm1f(d_y - l).
//   cross-entropy: [(1-eps) w_y (p_k - delta_ky) + (eps/C) (p_k sum_c w_c - w_k)] * grad_out / denominator, 0 for an ignored row
//   focal:         alpha_y [(1-p_y)^gamma - gamma p_y (1-p_y)^(gamma-1) log p_y] (p_k - delta_ky) * grad_out / denominator
template <int LANES, int PER>
__global__ __launch_bounds__(LOSS_THREADS) void loss_bwd_kernel(LossArgs a, const float2* __restrict__ row_state,
                                                                const double* __restrict__ stats, const float* __restrict__ grad_out,
                                                                float* __restrict__ dz, long long ld_d) {
  constexpr int RPB = LOSS_THREADS / LANES;
  const int sub = threadIdx.x & (LANES - 1);
  const long long row0 = (long long)blockIdx.x * RPB + threadIdx.x / LANES;
  const bool live = row0 < a.rows;
  const long long row = live ? row0 : a.rows - 1;
  const float* __restrict__ zr = a.z + row * a.ld;
  const int C = a.C;
  const long long y = a.y[row];
  const float2 st = row_state[row];
  const float g = a.reduction == QT_LOSS_REDUCE_NONE ? grad_out[row] : grad_out[0];
  const float scale = g / (float)stats[1];

  float z[PER];
  qt_row_load<LANES, PER>(zr, C, sub, z);
  const bool ce = a.kind == QT_LOSS_CROSS_ENTROPY;
  const bool ignored = ce && y == a.ignore_index;
  const bool in_range = y >= 0 && y < (long long)C;
  const bool bad = !ignored && !in_range;

  float ly_l = 0.f, wy_l = 1.f, wsum = 0.f;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int k = j * LANES + sub;
    if (k < C) {
      z[j] = (z[j] - st.x) - st.y;                      // log p_k
      if ((long long)k == y) ly_l = z[j];
      if (a.w) {
        const float wk = a.w[k];
        wsum += wk;
        if ((long long)k == y) wy_l = wk;
      }
    }
  }
  const int owner = in_range ? (int)(y & (LANES - 1)) : 0;
  float logp = qt_group_pick<LANES>(ly_l, owner);
  float wy = qt_group_pick<LANES>(wy_l, owner);
  if (bad) logp = wy = loss_nan();
  const float pm1 = expm1f(logp);                       // p_y - 1

  float c1, c2 = 0.f, W = 0.f;
  if (ce) {
    c1 = wy;
    if (a.eps > 0.f) {
      W = a.w ? qt_group_sum<LANES>(wsum) : (float)C;
      c1 = (1.f - a.eps) * wy;
      c2 = a.eps / (float)C;
    }
  } else {
    const float om = fmaxf(-pm1, 0.f);
    if (a.gamma == 0.f) {
      c1 = wy;
    } else {
      const float q = focal_pow_m1(om, a.gamma);
      c1 = wy * (q * om - a.gamma * expf(logp) * q * logp);
    }
  }
  if (!live) return;
  float* __restrict__ dr = dz + row * ld_d;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int k = j * LANES + sub;
    if (k < C) {
      const float p = expf(z[j]);
      float v = c1 * ((long long)k == y ? pm1 : p);
      if (c2 != 0.f) v += c2 * (p * W - (a.w ? a.w[k] : 1.f));
      dr[k] = ignored ? 0.f : v * scale;
    }
  }
}

int check_desc(const qt_loss_desc* d, long long rows, int C, const char* who) {
  QT_CHECK_ARG(d, "%s: null descriptor", who);
  if (d->dtype != QT_F32) {
    qt_set_error("%s: f32 logits only (dtype %d)", who, d->dtype);
    return QT_ERR_UNSUPPORTED;
  }
  QT_CHECK_ARG(d->kind == QT_LOSS_CROSS_ENTROPY || d->kind == QT_LOSS_FOCAL, "%s: unknown loss kind %d", who, d->kind);
  QT_CHECK_ARG(d->reduction == QT_LOSS_REDUCE_MEAN || d->reduction == QT_LOSS_REDUCE_SUM || d->reduction == QT_LOSS_REDUCE_NONE,
               "%s: unknown reduction %d", who, d->reduction);
  if (int rc = qt_check_rows_classes(who, rows, C, LOSS_MAX_C, 0)) return rc;
  QT_CHECK_ARG(!misaligned(d->class_weight, 3), "%s: class_weight must be 4-byte aligned", who);
  if (d->kind == QT_LOSS_CROSS_ENTROPY) {
    QT_CHECK_ARG(d->label_smoothing >= 0.f && d->label_smoothing <= 1.f, "%s: label_smoothing must be in [0, 1] (got %g)", who,
                 (double)d->label_smoothing);
  } else {
    QT_CHECK_ARG(d->gamma >= 0.f && isfinite(d->gamma), "%s: gamma must be a finite number >= 0 (got %g)", who, (double)d->gamma);
    if (d->gamma > 0.f && d->gamma < 1.f) {
      qt_set_error("%s: gamma = %g: only 0 and gamma >= 1 are handled (the derivative at p = 1 is infinite in between)", who,
                   (double)d->gamma);
      return QT_ERR_UNSUPPORTED;
    }
  }
  return QT_OK;
}

inline long long loss_blocks(long long rows, int C) {
  const int rpb = LOSS_THREADS / qt_row_lanes(C);
  return (rows + rpb - 1) / rpb;
}

LossArgs make_args(const qt_loss_desc* d, const float* logits, long long ld, const long long* labels, long long rows, int C) {
  LossArgs a;
  a.z = logits;
  a.y = labels;
  a.w = d->class_weight;
  a.rows = rows;
  a.ld = ld;
  a.C = C;
  a.kind = d->kind;
  a.reduction = d->reduction;
  a.ignore_index = d->ignore_index;
  a.eps = d->kind == QT_LOSS_CROSS_ENTROPY ? d->label_smoothing : 0.f;
  a.gamma = d->gamma;
  return a;
}

}  // namespace

extern "C" size_t qt_loss_workspace_bytes(long long rows, int C) {
  if (rows < 1 || C < 1 || C > LOSS_MAX_C) return 0;
  const long long blocks = loss_blocks(rows, C);
  return blocks > 1 ? (size_t)blocks * 3 * sizeof(double) : 0;
}

extern "C" int qt_loss_forward(const qt_loss_desc* desc, const float* logits, long long ld, const long long* labels, long long rows,
                               int C, float* loss, float* row_state, double* stats, long long* pred, double* meter,
                               void* workspace, size_t workspace_bytes, void* stream) {
  if (int st = check_desc(desc, rows, C, "qt_loss_forward")) return st;
  QT_CHECK_ARG(logits && labels && loss && stats, "qt_loss_forward: null logits / labels / loss / stats");
  QT_CHECK_ARG(ld >= C, "qt_loss_forward: row stride %lld < C = %d", ld, C);
  QT_CHECK_ARG(!misaligned(logits, 3) && !misaligned(loss, 3) && !misaligned(labels, 7) && !misaligned(stats, 7) &&
                   !misaligned(row_state, 7) && !misaligned(pred, 7) && !misaligned(meter, 7) && !misaligned(workspace, 7),
               "qt_loss_forward: f32 buffers must be 4-byte aligned, labels / row_state / stats / pred / meter / workspace 8-byte");
  const long long blocks = loss_blocks(rows, C);
  QT_CHECK_ARG(blocks <= (long long)INT32_MAX, "qt_loss_forward: too many rows for one call");
  const size_t need = qt_loss_workspace_bytes(rows, C);
  QT_CHECK_ARG(need == 0 || (workspace && workspace_bytes >= need),
               "qt_loss_forward: workspace of %zu bytes, %zu needed (qt_loss_workspace_bytes)", workspace ? workspace_bytes : (size_t)0,
               need);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const LossArgs a = make_args(desc, logits, ld, labels, rows, C);
  double* partial = blocks > 1 ? static_cast<double*>(workspace) : nullptr;
  float2* rs = reinterpret_cast<float2*>(row_state);
  qt_by_row_lanes<LOSS_MAX_C>(C, [&](auto L, auto P) {
    hipLaunchKernelGGL((loss_fwd_kernel<decltype(L)::value, decltype(P)::value>), dim3((unsigned)blocks), dim3(LOSS_THREADS), 0, s, a,
                       loss, rs, stats, pred, meter, partial);
  });
  QT_CHECK_LAUNCH();
  if (partial) {
    hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(LOSS_THREADS), 0, s, partial, (int)blocks, rows, desc->kind,
                       desc->reduction, loss, stats, meter);
    QT_CHECK_LAUNCH();
  }
  return QT_OK;
}

extern "C" int qt_loss_backward(const qt_loss_desc* desc, const float* logits, long long ld, const long long* labels, long long rows,
                                int C, const float* row_state, const double* stats, const float* grad_out, float* dlogits,
                                long long ld_d, void* stream) {
  if (int st = check_desc(desc, rows, C, "qt_loss_backward")) return st;
  QT_CHECK_ARG(logits && labels && row_state && stats && grad_out && dlogits,
               "qt_loss_backward: null logits / labels / row_state / stats / grad_out / dlogits");
  QT_CHECK_ARG(ld >= C && ld_d >= C, "qt_loss_backward: row strides %lld / %lld < C = %d", ld, ld_d, C);
  QT_CHECK_ARG(!misaligned(logits, 3) && !misaligned(grad_out, 3) && !misaligned(dlogits, 3) && !misaligned(labels, 7) &&
                   !misaligned(row_state, 7) && !misaligned(stats, 7),
               "qt_loss_backward: f32 buffers must be 4-byte aligned, labels / row_state / stats 8-byte");
  const long long blocks = loss_blocks(rows, C);
  QT_CHECK_ARG(blocks <= (long long)INT32_MAX, "qt_loss_backward: too many rows for one call");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const LossArgs a = make_args(desc, logits, ld, labels, rows, C);
  const float2* rs = reinterpret_cast<const float2*>(row_state);
  qt_by_row_lanes<LOSS_MAX_C>(C, [&](auto L, auto P) {
    hipLaunchKernelGGL((loss_bwd_kernel<decltype(L)::value, decltype(P)::value>), dim3((unsigned)blocks), dim3(LOSS_THREADS), 0, s, a,
                       rs, stats, grad_out, dlogits, ld_d);
  });
  QT_CHECK_LAUNCH();
  return QT_OK;
}
