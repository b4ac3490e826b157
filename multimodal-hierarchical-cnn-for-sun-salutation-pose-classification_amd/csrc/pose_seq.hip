// Sequence pose features on the device (qt_pose_sequence_features): 33 MediaPipe landmarks per frame to the 443 columns of
// sqn process/processing_image_sequence.py:96-247, the per-clip history of its loop (:374-441) included, and the CNN+LSTM
// loader's NaN -> 0, in one launch.  include/qtcnn.h states the rule in full.
//
// A workgroup of 256 threads owns a tile of PS_ROWS = 16 consecutive frames of ONE clip (a clip's last tile may be short):
//   1. predecessors.  The velocity and acceleration of a frame read the two most recent DETECTED frames before it.  Inside
//      the tile those are earlier frames of the tile; for its first frames they lie before it, arbitrarily far back, or in
//      the caller's history.  Wave 0 walks `detected` backwards from the tile's first frame, 64 flags per step, one ballot per
//      step, taking the highest set bits, until it has two frames or reaches the clip's first frame (no read outside the
//      clip); what is still missing comes from hist_in.  With the usual few undetected frames that is one step.  Everything
//      is wave-uniform and depends on the clip's flags alone: the same frames whatever the batch or the split into calls;
//   2. the tile's PS_ROWS x 528 bytes are contiguous: 16-byte loads, lane after lane, into LDS slots 2 ..; the two
//      predecessor frames go to slots 0 (most recent) and 1.  One thread runs over the tile's flags and leaves, per frame,
//      the LDS slots of its two predecessors (or none) -- 16 steps, beside the loads;
//   3. a frame's 14 computed scalars (ten angles, three distances, the variance ratio) go to 14 lanes, thread = (task, frame)
//      with the task the slow index as in pose.hip; then thread = (frame, landmark) for the three relative coordinates and
//      the six motion columns of a landmark.  Columns 132 .. 442 of every frame are left in LDS (311 floats per frame, an
//      odd stride: the 16 frames of a task do not share a bank); columns 0 .. 131 are the staged landmarks themselves;
//   4. the tile's rows are contiguous in `out`: 1772 bytes per row, a multiple of 4 but not of 16, and a clip may start at
//      any address modulo 16, so the span is walked by address: up to three single floats to the first 16-byte boundary,
//      float4 stores, up to three single floats behind them.  An element is NaN (frame not detected), a staged landmark
//      value or a feature from LDS, imputed as it is stored.  Each row is written exactly once: 528 bytes in, 1772 out;
//   5. the workgroup that owns a clip's last frame writes hist_out / hist_count_out from its LDS slots.
// No atomics, no zero fill, no workspace, no host synchronisation.
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "qt_common.h"

namespace {

constexpr int PS_THREADS = 256;
constexpr int PS_ROWS = 16;                     // frames per workgroup
constexpr int PS_LM = QT_POSE_LANDMARKS;
constexpr int PS_F = QT_POSE_SEQ_FEATURES;
constexpr int PS_RAW = 4 * PS_LM;               // columns 0 .. 131: the landmarks as given
constexpr int PS_FEAT = PS_F - PS_RAW;          // columns 132 .. 442, kept in LDS
constexpr int PS_TASKS = 14;                    // scalar tasks per frame: 10 angles, 3 distances, the variance ratio
constexpr int PS_COL_REL = 145 - PS_RAW, PS_COL_DYN = 244 - PS_RAW, PS_COL_VAR = 442 - PS_RAW;
constexpr int PS_NONE = INT_MIN;                // "no such predecessor"
constexpr long long PS_MAX_FRAMES = 1LL << 22;
constexpr float PS_VIS = 0.65f;
constexpr float PS_DEG = 57.29577951308232f;    // 180 / pi
static_assert(PS_THREADS / PS_ROWS >= PS_TASKS && 2 * PS_LM <= PS_THREADS, "task layout");
static_assert(PS_FEAT == 311 && (PS_FEAT & 1) == 1 && PS_COL_DYN + 6 * PS_LM == PS_COL_VAR, "column layout");

struct SeqArgs {
  const float4* landmarks;
  const unsigned char* detected;
  const int* sizes;
  const float4* hist_in;
  const unsigned char* hist_count_in;
  float4* hist_out;
  unsigned char* hist_count_out;
  float* out;
  int T, tiles, W, H, mode;
};

__device__ __forceinline__ float ps_nan() { return __builtin_nanf(""); }

struct P3 {
  float x, y, z;
};
__device__ __forceinline__ P3 sub(const P3& a, const P3& b) { return P3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ float dot(const P3& a, const P3& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ float dist(const P3& a, const P3& b) {
  const P3 d = sub(a, b);
  return sqrtf(dot(d, d));
}
// A product as an f32 of its own.  The library is built with -ffp-contract=fast, which would fuse x W into the subtraction
// that follows it, q_a - q_b = fma(x_a, W, -q_b): a landmark that did not move would get the rounding error of q_b as its
// velocity, and two landmarks at one place (wrist on elbow) a limb of that length instead of the zero vector.
__device__ __forceinline__ float rounded(float v) {
  asm("" : "+v"(v));
  return v;
}
// pixel position of a landmark
__device__ __forceinline__ P3 pixel(const float4& v, float W, float H) {
  return P3{rounded(v.x * W), rounded(v.y * H), rounded(v.z * W)};
}
__device__ __forceinline__ bool visible(const float4& v) { return v.w > PS_VIS; }   // false for a NaN

// column 132 + task (task < 13) or column 442 (task 13) of one detected frame; f: its 33 landmarks in LDS
__device__ float seq_task(const float4* f, int task, float W, float H) {
  if (task < 10) {
    constexpr int T[10][3] = {{11, 13, 15}, {12, 14, 16}, {13, 11, 23}, {14, 12, 24}, {23, 25, 27},
                              {24, 26, 28}, {11, 23, 25}, {12, 24, 26}, {0, 11, 23},  {11, 12, 23}};
    const float4 a = f[T[task][0]], b = f[T[task][1]], c = f[T[task][2]];
    if (!(visible(a) && visible(b) && visible(c))) return ps_nan();
    const P3 qb = pixel(b, W, H);
    const P3 ba = sub(pixel(a, W, H), qb), bc = sub(pixel(c, W, H), qb);
    if ((ba.x == 0.f && ba.y == 0.f && ba.z == 0.f) || (bc.x == 0.f && bc.y == 0.f && bc.z == 0.f)) return 0.f;
    const P3 cr = P3{ba.y * bc.z - ba.z * bc.y, ba.z * bc.x - ba.x * bc.z, ba.x * bc.y - ba.y * bc.x};
    return atan2f(sqrtf(dot(cr, cr)), dot(ba, bc)) * PS_DEG;
  }
  const float4 ls = f[11], rs = f[12], lh = f[23], rh = f[24];
  if (task < 13) {   // distances over the body scale
    constexpr int D[3][2] = {{15, 16}, {27, 28}, {15, 23}};
    const float4 a = f[D[task - 10][0]], b = f[D[task - 10][1]];
    if (!(visible(a) && visible(b))) return ps_nan();
    const float sw = visible(ls) && visible(rs) ? dist(pixel(ls, W, H), pixel(rs, W, H)) : 0.f;
    const float hw = visible(lh) && visible(rh) ? dist(pixel(lh, W, H), pixel(rh, W, H)) : 0.f;
    const float least = 0.05f * W;
    const float s = sw > least ? sw : (hw > least ? hw : H / 3.f);
    return dist(pixel(a, W, H), pixel(b, W, H)) / s;
  }
  // (var(x) + 1e-6) / (var(y) + 1e-6) over the visible torso landmarks, two passes
  const float xs[4] = {ls.x, rs.x, lh.x, rh.x}, ys[4] = {ls.y, rs.y, lh.y, rh.y};
  const bool vis[4] = {visible(ls), visible(rs), visible(lh), visible(rh)};
  int n = 0;
  float sx = 0.f, sy = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (vis[k]) {
      ++n;
      sx += xs[k];
      sy += ys[k];
    }
  if (n < 2) return ps_nan();
  const float fn = (float)n, mx = sx / fn, my = sy / fn;
  float qx = 0.f, qy = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (vis[k]) {
      const float dx = xs[k] - mx, dy = ys[k] - my;
      qx += dx * dx;
      qy += dy * dy;
    }
  return (qx / fn + 1e-6f) / (qy / fn + 1e-6f);
}

// dst[t] = value(t) for 0 <= t < n: singles to the first 16-byte boundary, float4 stores, singles behind
template <typename F1>
__device__ __forceinline__ void store_span(float* dst, int n, int first, int step, F1 value) {
  int head = (int)((16u - (unsigned)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u) >> 2;
  if (head > n) head = n;
  const int nvec = (n - head) >> 2;
  const int tail = n - head - 4 * nvec;
  for (int i = first; i < nvec; i += step) {
    const int t = head + 4 * i;
    *reinterpret_cast<float4*>(dst + t) = make_float4(value(t), value(t + 1), value(t + 2), value(t + 3));
  }
  if (first < head + tail) {
    const int o = first < head ? first : 4 * nvec + first;   // (head + 4 nvec + (first - head))
    dst[o] = value(o);
  }
}

__global__ __launch_bounds__(PS_THREADS) void pose_sequence_kernel(SeqArgs a) {
  __shared__ float4 lm[(PS_ROWS + 2) * PS_LM];   // slot 0, 1: the predecessors of the tile's first frame; slot 2 + r: frame r
  __shared__ float feat[PS_ROWS * PS_FEAT];
  __shared__ int pred[2];                        // slot 0, 1: frame index in the clip, -1 - k for hist_in slot k, or PS_NONE
  __shared__ int last[2];                        // LDS slots of the two most recent detected frames after the tile, or -1
  __shared__ signed char prev1[PS_ROWS], prev2[PS_ROWS];   // per frame: LDS slots of its predecessors, or -1
  __shared__ unsigned char live[PS_ROWS];        // per frame: detected, in a clip with a positive frame size
  const int tid = threadIdx.x;
  const int b = blockIdx.x / a.tiles;
  const int t0 = (blockIdx.x - b * a.tiles) * PS_ROWS;
  const int nrows = min(PS_ROWS, a.T - t0);
  const long long clip = (long long)b * a.T;     // first frame of the clip, in frames
  const unsigned char* det = a.detected ? a.detected + clip : nullptr;

  if (tid < QT_WAVE) {   // 1. the backward walk (wave 0, uniform)
    int found = 0, n1 = PS_NONE, n2 = PS_NONE;
    for (int base = t0 - QT_WAVE; found < 2 && base > -QT_WAVE; base -= QT_WAVE) {
      const int t = base + tid;                  // t < t0
      unsigned long long m = __ballot(t >= 0 && (det == nullptr || det[t] != 0));
      while (m != 0 && found < 2) {
        const int hi = 63 - __clzll((long long)m);
        (found == 0 ? n1 : n2) = base + hi;
        ++found;
        m &= ~(1ull << hi);
      }
    }
    const int held = a.hist_in ? min((int)a.hist_count_in[b], 2) : 0;
    for (int k = 0; found < 2 && k < held; ++k, ++found) (found == 0 ? n1 : n2) = -1 - k;
    if (tid == 0) {
      pred[0] = n1;
      pred[1] = n2;
    }
  }
  // 2. stage the tile
  const float4* __restrict__ src = a.landmarks + (clip + t0) * PS_LM;
  for (int i = tid; i < nrows * PS_LM; i += PS_THREADS) lm[2 * PS_LM + i] = src[i];
  float W = (float)a.W, H = (float)a.H;
  bool sized = true;
  if (a.sizes) {
    const int w = a.sizes[2 * b], h = a.sizes[2 * b + 1];
    sized = w > 0 && h > 0;
    W = (float)w;
    H = (float)h;
  }
  __syncthreads();
  if (tid < 2 * PS_LM) {
    const int s = tid >= PS_LM, j = tid - s * PS_LM, at = pred[s];
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (at >= 0)
      v = a.landmarks[(clip + at) * PS_LM + j];
    else if (at != PS_NONE)
      v = a.hist_in[((long long)b * 2 + (-1 - at)) * PS_LM + j];
    lm[tid] = v;
  } else if (tid == PS_THREADS - 1) {
    int p = pred[0] != PS_NONE ? 0 : -1, pp = pred[1] != PS_NONE ? 1 : -1;
    for (int r = 0; r < nrows; ++r) {
      const bool d = det == nullptr || det[t0 + r] != 0;
      prev1[r] = (signed char)p;
      prev2[r] = (signed char)pp;
      live[r] = d && sized;
      if (d) {
        pp = p;
        p = r + 2;
      }
    }
    last[0] = p;
    last[1] = pp;
  }
  __syncthreads();

  // 3. the scalar tasks, then the per-landmark columns
  {
    const int task = tid / PS_ROWS, r = tid & (PS_ROWS - 1);
    if (task < PS_TASKS && r < nrows && live[r])
      feat[r * PS_FEAT + (task < 13 ? task : PS_COL_VAR)] = seq_task(lm + (r + 2) * PS_LM, task, W, H);
  }
  for (int i = tid; i < nrows * PS_LM; i += PS_THREADS) {
    const int r = i / PS_LM, j = i - r * PS_LM;
    if (!live[r]) continue;
    const float4* f = lm + (r + 2) * PS_LM;
    const float4 cur = f[j], lh = f[23], rh = f[24];
    const bool vis = visible(cur);
    float* row = feat + r * PS_FEAT;
    const bool hips = visible(lh) && visible(rh);
    const float mx = hips ? (lh.x + rh.x) * 0.5f : 0.5f, my = hips ? (lh.y + rh.y) * 0.5f : 0.5f,
                mz = hips ? (lh.z + rh.z) * 0.5f : 0.f;
    row[PS_COL_REL + 3 * j + 0] = vis ? cur.x - mx : ps_nan();
    row[PS_COL_REL + 3 * j + 1] = vis ? cur.y - my : ps_nan();
    row[PS_COL_REL + 3 * j + 2] = vis ? cur.z - mz : ps_nan();
    float d[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) d[k] = ps_nan();
    const int s1 = prev1[r], s2 = prev2[r];
    if (vis && s1 >= 0 && s2 >= 0) {
      const float4 one = lm[s1 * PS_LM + j], two = lm[s2 * PS_LM + j];
      if (visible(one) && visible(two)) {
        const P3 q1 = pixel(one, W, H);
        const P3 v = sub(pixel(cur, W, H), q1);
        const P3 acc = sub(v, sub(q1, pixel(two, W, H)));
        d[0] = v.x; d[1] = v.y; d[2] = v.z;
        d[3] = acc.x; d[4] = acc.y; d[5] = acc.z;
      }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) row[PS_COL_DYN + 6 * j + k] = d[k];
  }
  __syncthreads();

  // 4. the rows
  const float* lmf = reinterpret_cast<const float*>(lm + 2 * PS_LM);
  const bool zero = a.mode == QT_POSE_ZERO;
  auto value = [&](int t) -> float {   // t: index into the tile's nrows x 443 outputs
    const int r = t / PS_F, c = t - r * PS_F;
    float v = ps_nan();
    if (live[r]) v = c < PS_RAW ? lmf[r * PS_RAW + c] : feat[r * PS_FEAT + (c - PS_RAW)];
    return zero && v != v ? 0.f : v;
  };
  store_span(a.out + (clip + t0) * PS_F, nrows * PS_F, tid, PS_THREADS, value);

  // 5. the history after the clip's last frame
  if (a.hist_out && t0 + nrows == a.T) {
    if (tid < 2 * PS_LM) {
      const int s = tid >= PS_LM, j = tid - s * PS_LM, slot = last[s];
      a.hist_out[((long long)b * 2 + s) * PS_LM + j] = slot >= 0 ? lm[slot * PS_LM + j] : make_float4(0.f, 0.f, 0.f, 0.f);
    } else if (tid == PS_THREADS - 1) {
      a.hist_count_out[b] = (unsigned char)((last[0] >= 0) + (last[1] >= 0));
    }
  }
}

bool overlap(const void* p, const void* q, size_t bytes) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return a < b + bytes && b < a + bytes;
}

}  // namespace

extern "C" int qt_pose_sequence_features(const qt_pose_seq_desc* desc, const float* landmarks, const unsigned char* detected,
                                         const int* sizes, const float* hist_in, const unsigned char* hist_count_in,
                                         float* hist_out, unsigned char* hist_count_out, float* out, void* stream) {
  const char* const who = "qt_pose_sequence_features";
  QT_CHECK_ARG(desc != nullptr, "%s: null descriptor", who);
  QT_CHECK_ARG(desc->batch >= 1 && desc->frames >= 1, "%s: batch and frames must be positive (got %d, %d)", who, desc->batch,
               desc->frames);
  QT_CHECK_ARG(desc->mode == QT_POSE_RAW || desc->mode == QT_POSE_ZERO,
               "%s: unknown mode %d (QT_POSE_RAW or QT_POSE_ZERO; there are no class tables for these columns)", who, desc->mode);
  const long long frames = (long long)desc->batch * desc->frames;
  if (frames > PS_MAX_FRAMES) {
    qt_set_error("%s: %lld frames in one call; at most %lld are handled", who, frames, PS_MAX_FRAMES);
    return QT_ERR_UNSUPPORTED;
  }
  QT_CHECK_ARG(landmarks != nullptr && out != nullptr, "%s: null landmarks or output", who);
  QT_CHECK_ARG(((reinterpret_cast<uintptr_t>(landmarks) | reinterpret_cast<uintptr_t>(hist_in) |
                 reinterpret_cast<uintptr_t>(hist_out)) & 15) == 0,
               "%s: landmarks and the histories must be 16-byte aligned", who);
  QT_CHECK_ARG(((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(sizes)) & 3) == 0,
               "%s: output and sizes must be 4-byte aligned", who);
  QT_CHECK_ARG(sizes != nullptr || (desc->width >= 1 && desc->height >= 1),
               "%s: without `sizes` the descriptor's frame size must be positive (got %d x %d)", who, desc->width, desc->height);
  QT_CHECK_ARG((hist_in != nullptr) == (hist_count_in != nullptr) && (hist_out != nullptr) == (hist_count_out != nullptr),
               "%s: a history and its counts come together (half a history pair)", who);
  if (hist_in && hist_out)
    QT_CHECK_ARG(!overlap(hist_in, hist_out, (size_t)desc->batch * 2 * PS_LM * 16) &&
                     !overlap(hist_count_in, hist_count_out, (size_t)desc->batch),
                 "%s: hist_out / hist_count_out must not overlap hist_in / hist_count_in (swap two buffers)", who);
  SeqArgs a;
  a.landmarks = reinterpret_cast<const float4*>(landmarks);
  a.detected = detected;
  a.sizes = sizes;
  a.hist_in = reinterpret_cast<const float4*>(hist_in);
  a.hist_count_in = hist_count_in;
  a.hist_out = reinterpret_cast<float4*>(hist_out);
  a.hist_count_out = hist_count_out;
  a.out = out;
  a.T = desc->frames;
  a.tiles = qt_cdiv(desc->frames, PS_ROWS);
  a.W = sizes ? 0 : desc->width;
  a.H = sizes ? 0 : desc->height;
  a.mode = desc->mode;
  const unsigned blocks = (unsigned)((long long)desc->batch * a.tiles);
  hipLaunchKernelGGL(pose_sequence_kernel, dim3(blocks), dim3(PS_THREADS), 0, static_cast<hipStream_t>(stream), a);
  QT_CHECK_LAUNCH();
  return QT_OK;
}
