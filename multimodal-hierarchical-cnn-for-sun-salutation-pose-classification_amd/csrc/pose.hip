// The 47-float pose vector on the device (qt_pose_features): 33 MediaPipe landmarks to the reference's features
// (experiment/test_on_video_cnn.py:126-202), or the stored raw vectors, followed by the loaders' NaN imputation
// (Quadtree_from scratch/dataloader.py:84-88, 3dcnn/dataloaders.py:119-139), in one launch.  include/qtcnn.h states the
// rule in full.
//
// From landmarks, a workgroup of 256 threads owns PF_ROWS = 32 consecutive rows:
//   1. the rows' 32 x 528 bytes are contiguous: 16-byte loads, lane after lane, into LDS;
//   2. thread = (task, row): a row's 14 computed features (8 joint angles, the two torso angles, the three normalised
//      distances, the variance ratio) go to 14 lanes, two passes of 16 rows.  The task is the slow index, tid / 16, so the
//      64 lanes of a wave hold four tasks for 16 rows: the first two waves are joint angles only and do not diverge, the
//      other two take two or three branches, and 16 rows 528 bytes apart read their float4 landmarks from LDS without a bank
//      conflict.  Each lane leaves its feature in LDS;
//   3. the tile's 32 x 47 outputs are contiguous too, and 32 x 188 bytes is a multiple of 16: every tile starts at the
//      same address modulo 16 as `out`.  Up to three single floats to the first 16-byte boundary, float4 stores, up to
//      three single floats behind them.  An element is its row's visibility (from the staged landmarks) or a feature,
//      imputed as it is stored.
// From stored vectors there is nothing to stage: the same head / float4 / tail walk over the flat [rows x 47] array, each
// element read and written by the same thread (out == raw is fine), 16-byte loads when raw and out agree modulo 16.
// No atomics, no zero fill, no workspace, no host synchronisation; a row's bits do not depend on its neighbours.
#include <math.h>
#include <stdint.h>

#include "qt_common.h"

namespace {

constexpr int PF_THREADS = 256;
constexpr int PF_ROWS = 32;            // rows per workgroup (landmark source); PF_ROWS * 188 bytes is a multiple of 16
constexpr int PF_F = QT_POSE_FEATURES;
constexpr int PF_LM = QT_POSE_LANDMARKS;
constexpr int PF_TASKS = 14;           // computed features per row, columns 33 .. 46
constexpr int PF_PASS = 16;            // rows per pass of step 2: PF_THREADS / PF_PASS = 16 task slots, 14 used
constexpr long long PF_MAX_ROWS = 1LL << 22;
static_assert((PF_ROWS * PF_F * 4) % 16 == 0, "a tile of output rows must keep the alignment of `out`");
static_assert(PF_F - PF_LM == PF_TASKS && PF_THREADS / PF_PASS >= PF_TASKS && PF_ROWS % PF_PASS == 0, "task layout");

struct PoseArgs {
  const float4* landmarks;      // source A
  const unsigned char* detected;
  const float* raw;             // source B
  const long long* labels;
  const float* means;
  const float* stds;
  float* out;
  long long rows;
  int rows_per_label, K, mode;
  int raw_vec;                  // source B: raw and out agree modulo 16
};

__device__ __forceinline__ float pf_nan() { return __builtin_nanf(""); }

struct P3 {
  float x, y, z;
};
__device__ __forceinline__ P3 pt(const float4* lm, int j) {
  const float4 v = lm[j];
  return P3{v.x, v.y, v.z};
}
__device__ __forceinline__ P3 sub(const P3& a, const P3& b) { return P3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ float dot(const P3& a, const P3& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ float dist(const P3& a, const P3& b) {
  const P3 d = sub(a, b);
  return sqrtf(dot(d, d));
}
constexpr float PF_DEG = 57.29577951308232f;       // 180 / pi
constexpr float PF_HALF_PI = 1.5707963267948966f;

// angle at b of (a, b, c) in degrees: atan2(|ba x bc|, ba . bc); NaN when a limb has no length
__device__ __forceinline__ float joint_angle(const P3& a, const P3& b, const P3& c) {
  const P3 ba = sub(a, b), bc = sub(c, b);
  if ((ba.x == 0.f && ba.y == 0.f && ba.z == 0.f) || (bc.x == 0.f && bc.y == 0.f && bc.z == 0.f)) return pf_nan();
  const P3 cr = P3{ba.y * bc.z - ba.z * bc.y, ba.z * bc.x - ba.x * bc.z, ba.x * bc.y - ba.y * bc.x};
  return atan2f(sqrtf(dot(cr, cr)), dot(ba, bc)) * PF_DEG;
}
__device__ __forceinline__ float fold180(float d) {
  d = fabsf(d);
  return d > 180.f ? 360.f - d : d;
}

// feature 33 + task of one detected row; lm: its 33 landmarks in LDS
__device__ float pose_task(const float4* lm, int task) {
  if (task < 8) {
    // (a, b, c): elbows, shoulders, knees, hips, left then right
    constexpr int T[8][3] = {{11, 13, 15}, {12, 14, 16}, {23, 11, 13}, {24, 12, 14},
                             {23, 25, 27}, {24, 26, 28}, {11, 23, 25}, {12, 24, 26}};
    return joint_angle(pt(lm, T[task][0]), pt(lm, T[task][1]), pt(lm, T[task][2]));
  }
  const float4 ls = lm[11], rs = lm[12], lh = lm[23], rh = lm[24];
  if (task == 8) {   // torso against the vertical
    const float tx = (ls.x + rs.x) * 0.5f - (lh.x + rh.x) * 0.5f;
    const float ty = (ls.y + rs.y) * 0.5f - (lh.y + rh.y) * 0.5f;
    return fold180((PF_HALF_PI - atan2f(ty, tx)) * PF_DEG);
  }
  if (task == 9) {   // shoulder line against hip line
    const float sa = atan2f(rs.y - ls.y, rs.x - ls.x) * PF_DEG;
    const float ha = atan2f(rh.y - lh.y, rh.x - lh.x) * PF_DEG;
    return fold180(sa - ha);
  }
  if (task < 13) {   // distances over the body scale
    const float sw = dist(P3{ls.x, ls.y, ls.z}, P3{rs.x, rs.y, rs.z});
    const float hw = dist(P3{lh.x, lh.y, lh.z}, P3{rh.x, rh.y, rh.z});
    float s = (sw > 0.f && hw > 0.f) ? (sw + hw) * 0.5f : 1.f;
    if (s == 0.f) s = 1.f;
    if (!(s > 0.05f)) return pf_nan();
    constexpr int D[3][2] = {{15, 16}, {27, 28}, {15, 23}};
    return dist(pt(lm, D[task - 10][0]), pt(lm, D[task - 10][1])) / s;
  }
  // var(x) / var(y) over the visible torso landmarks, two passes
  const float xs[4] = {ls.x, rs.x, lh.x, rh.x}, ys[4] = {ls.y, rs.y, lh.y, rh.y};
  const bool vis[4] = {ls.w > 0.65f, rs.w > 0.65f, lh.w > 0.65f, rh.w > 0.65f};
  int n = 0;
  float sx = 0.f, sy = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (vis[k]) {
      ++n;
      sx += xs[k];
      sy += ys[k];
    }
  if (n < 2) return pf_nan();
  const float fn = (float)n, mx = sx / fn, my = sy / fn;
  float qx = 0.f, qy = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (vis[k]) {
      const float dx = xs[k] - mx, dy = ys[k] - my;
      qx += dx * dx;
      qy += dy * dy;
    }
  const float vx = qx / fn, vy = qy / fn;
  return vy != 0.f ? vx / vy : pf_nan();   // (a NaN var(y) gives NaN either way)
}

// the imputation of element (row, col); rows < 2^22: 32-bit arithmetic
__device__ __forceinline__ float impute(const PoseArgs& a, float v, int row, int col) {
  if (a.mode == QT_POSE_RAW) return v;
  if (a.mode == QT_POSE_ZERO) return v != v ? 0.f : v;
  const long long label = a.labels[row / a.rows_per_label];
  if (label < 0 || label >= a.K) return pf_nan();   // nothing is indexed with it
  const float m = a.means[label * PF_F + col];
  if (v != v) v = m;
  if (a.mode == QT_POSE_CLASS_MEAN) return v;
  const float sd = a.stds[label * PF_F + col];
  return sd < 1e-6f ? 0.f : (v - m) / sd;
}

// dst[t] = value(t) for 0 <= t < n: singles to the first 16-byte boundary, float4 stores, singles behind; value4(t, v) fills
// four consecutive elements
template <typename F1, typename F4>
__device__ __forceinline__ void store_span(float* dst, int n, int first, int step, F1 value, F4 value4) {
  int head = (int)((16u - (unsigned)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u) >> 2;
  if (head > n) head = n;
  const int nvec = (n - head) >> 2;
  const int tail = n - head - 4 * nvec;
  for (int i = first; i < nvec; i += step) {
    float v[4];
    value4(head + 4 * i, v);
    *reinterpret_cast<float4*>(dst + head + 4 * i) = make_float4(v[0], v[1], v[2], v[3]);
  }
  if (first < head + tail) {
    const int o = first < head ? first : 4 * nvec + first;   // (head + 4 nvec + (first - head))
    dst[o] = value(o);
  }
}

__global__ __launch_bounds__(PF_THREADS) void pose_landmarks_kernel(PoseArgs a) {
  __shared__ float4 lm[PF_ROWS * PF_LM];
  __shared__ float feat[PF_ROWS * PF_TASKS];
  const int tid = threadIdx.x;
  const long long row0 = (long long)blockIdx.x * PF_ROWS;
  const int nrows = (int)min((long long)PF_ROWS, a.rows - row0);

  const float4* __restrict__ src = a.landmarks + row0 * PF_LM;
  for (int i = tid; i < nrows * PF_LM; i += PF_THREADS) lm[i] = src[i];
  __syncthreads();

  const int task = tid / PF_PASS;
  for (int r = tid & (PF_PASS - 1); r < nrows; r += PF_PASS)
    if (task < PF_TASKS) {
      const bool found = a.detected == nullptr || a.detected[row0 + r] != 0;
      feat[r * PF_TASKS + task] = found ? pose_task(lm + r * PF_LM, task) : pf_nan();
    }
  __syncthreads();

  auto value = [&](int t) -> float {   // t: index into the tile's nrows x 47 outputs
    const int r = t / PF_F, c = t - r * PF_F;
    float v;
    if (c < PF_LM)
      v = (a.detected == nullptr || a.detected[row0 + r] != 0) ? lm[r * PF_LM + c].w : 0.f;
    else
      v = feat[r * PF_TASKS + (c - PF_LM)];
    return impute(a, v, (int)row0 + r, c);
  };
  auto value4 = [&](int t, float (&v)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = value(t + k);
  };
  store_span(a.out + row0 * PF_F, nrows * PF_F, tid, PF_THREADS, value, value4);
}

__global__ __launch_bounds__(PF_THREADS) void pose_impute_kernel(PoseArgs a) {
  // a workgroup takes PF_ROWS rows here too, so that its span starts at out's address modulo 16
  const long long row0 = (long long)blockIdx.x * PF_ROWS;
  const int nrows = (int)min((long long)PF_ROWS, a.rows - row0);
  const float* raw = a.raw + row0 * PF_F;   // may be `out` itself
  auto value = [&](int t) -> float {        // t: index into the tile's nrows x 47 elements
    const int r = t / PF_F;
    return impute(a, raw[t], (int)row0 + r, t - r * PF_F);
  };
  auto value4 = [&](int t, float (&v)[4]) {
    float in[4];
    if (a.raw_vec) {
      const float4 u = *reinterpret_cast<const float4*>(raw + t);
      in[0] = u.x; in[1] = u.y; in[2] = u.z; in[3] = u.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) in[k] = raw[t + k];
    }
    int r = t / PF_F;
    int c = t - r * PF_F;
    r += (int)row0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[k] = impute(a, in[k], r, c);
      if (++c == PF_F) {
        c = 0;
        ++r;
      }
    }
  };
  store_span(a.out + row0 * PF_F, nrows * PF_F, (int)threadIdx.x, PF_THREADS, value, value4);
}

}  // namespace

extern "C" int qt_pose_features(const qt_pose_desc* desc, const float* landmarks, const unsigned char* detected, const float* raw,
                                const long long* labels, const float* means, const float* stds, float* out, void* stream) {
  QT_CHECK_ARG(desc != nullptr, "qt_pose_features: null descriptor");
  QT_CHECK_ARG(desc->rows >= 1, "qt_pose_features: rows must be positive (got %lld)", desc->rows);
  QT_CHECK_ARG(desc->mode == QT_POSE_RAW || desc->mode == QT_POSE_ZERO || desc->mode == QT_POSE_CLASS_MEAN ||
                   desc->mode == QT_POSE_STANDARDIZE,
               "qt_pose_features: unknown mode %d", desc->mode);
  if (desc->rows > PF_MAX_ROWS) {
    qt_set_error("qt_pose_features: %lld rows in one call; at most %lld are handled", desc->rows, PF_MAX_ROWS);
    return QT_ERR_UNSUPPORTED;
  }
  QT_CHECK_ARG((landmarks != nullptr) != (raw != nullptr),
               "qt_pose_features: exactly one source, landmarks or raw vectors, must be given");
  QT_CHECK_ARG(out != nullptr, "qt_pose_features: null output");
  QT_CHECK_ARG(raw != nullptr ? detected == nullptr : true, "qt_pose_features: `detected` belongs to the landmark source");
  QT_CHECK_ARG((reinterpret_cast<uintptr_t>(landmarks) & 15) == 0, "qt_pose_features: landmarks must be 16-byte aligned");
  QT_CHECK_ARG(((reinterpret_cast<uintptr_t>(raw) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(means) |
                 reinterpret_cast<uintptr_t>(stds)) & 3) == 0 && (reinterpret_cast<uintptr_t>(labels) & 7) == 0,
               "qt_pose_features: raw vectors, output, means and stds must be 4-byte aligned, labels 8-byte aligned");
  const bool by_class = desc->mode == QT_POSE_CLASS_MEAN || desc->mode == QT_POSE_STANDARDIZE;
  if (by_class) {
    QT_CHECK_ARG(labels != nullptr && means != nullptr && desc->num_classes >= 1,
                 "qt_pose_features: mode %d needs labels, class means and num_classes >= 1 (got %d)", desc->mode, desc->num_classes);
    QT_CHECK_ARG(desc->mode != QT_POSE_STANDARDIZE || stds != nullptr, "qt_pose_features: QT_POSE_STANDARDIZE needs class stds");
    QT_CHECK_ARG(desc->rows_per_label >= 1 && desc->rows % desc->rows_per_label == 0,
                 "qt_pose_features: rows_per_label must be >= 1 and divide rows (got %d for %lld rows)", desc->rows_per_label,
                 desc->rows);
  }
  PoseArgs a;
  a.landmarks = reinterpret_cast<const float4*>(landmarks);
  a.detected = detected;
  a.raw = raw;
  a.labels = labels;
  a.means = means;
  a.stds = stds;
  a.out = out;
  a.rows = desc->rows;
  a.rows_per_label = by_class ? desc->rows_per_label : 1;
  a.K = by_class ? desc->num_classes : 0;
  a.mode = desc->mode;
  a.raw_vec = ((reinterpret_cast<uintptr_t>(raw) ^ reinterpret_cast<uintptr_t>(out)) & 15u) == 0;
  const unsigned blocks = (unsigned)qt_cdiv(desc->rows, PF_ROWS);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (landmarks)
    hipLaunchKernelGGL(pose_landmarks_kernel, dim3(blocks), dim3(PF_THREADS), 0, st, a);
  else
    hipLaunchKernelGGL(pose_impute_kernel, dim3(blocks), dim3(PF_THREADS), 0, st, a);
  QT_CHECK_LAUNCH();
  return QT_OK;
}
