// Pose timeline on the device (qt_timeline_smooth / qt_timeline_decode): between the per-frame probabilities of the video
// loop and what is shown or told: a trailing-window mean with its argmax and confidence, then a debounced label per frame
// and the list of segments "which pose from when to when".  The reference has no such step (experiment/
// test_on_video_cnn.py:274-292 writes each frame's raw argmax).  include/qtcnn.h states both rules in full.
//
// Smooth.  A workgroup of 256 threads owns a tile of TL_TILE = 64 consecutive frames of ONE stream (a stream's last tile may
// be short):
//   1. it stages the tile's rows and the W - 1 rows in front of them in LDS, slot s = row t0 - (W - 1) + s of the stream: from
//      probs, or, before the stream's first frame, from hist_in (slot -1 - row), or zeros where the history holds nothing.
//      16-byte loads where C, ld and the addresses are multiples of four floats, single floats otherwise.  (64 + 63) rows x 64
//      classes are 32 KB;
//   2. thread = (frame, class), LANES = 16 (C <= 16: a frame is one DPP row) or 64 (a frame is one wave) lanes per frame.  A
//      thread adds its class's n = min(W, seen + f + 1) values from the oldest row to the newest, afresh for every frame, and
//      divides once: adds and one IEEE division, nothing for -ffp-contract to fuse.  W C adds per frame are nothing beside
//      the forward pass, and a running sum would drift, keep a NaN for ever and depend on where a call starts;
//   3. the argmax runs across the class lanes in qt_rowgroup.h's total order (qt_group_argmax: the loss head's and the
//      meters'); the value that travels with the index is the confidence;
//   4. the workgroup that owns the stream's last frame copies the last W - 1 LDS rows to hist_out (rows in front of an empty
//      stream are the zeros staged in 1).
// Decode.  One workgroup of one wave per stream walks its frames in trips of TL_TRIP = 64, lane = frame, the pred /
// confidence of the next four trips loaded while these four are worked on.  Inside a trip both recurrences are "last
// qualifying lane" scans over a ballot: the run length ending at a lane is its distance to the last lane whose c differs from its predecessor's, the
// stable label is c at the last lane whose run reached min_run; a segment starts at the last lane whose stable label differs
// from its predecessor's; confidence sums are an integer prefix sum, record slots a ballot rank added to segments_total.
// The neighbour's value and the prefix sum are DPP shifts (wave_shr, row_shr, row_bcast), so a trip's chain of dependent steps
// holds two LDS-crossbar permutes (c at a lane, the prefix sum at a lane) and no barrier.  What crosses a trip (and a call) is
// the eight values of the state, read from the trip's last lane into scalars.  No workgroup waits for another: streams are
// independent, and a single offline video is one wave by design.
// No atomics, no zero fill, no workspace, no host synchronisation in either.
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "qt_common.h"
#include "qt_rowgroup.h"

namespace {

constexpr int TL_THREADS = 256;
constexpr int TL_TILE = 64;                      // frames per workgroup (smooth)
constexpr int TL_TRIP = 64;                      // frames per trip (decode): one per lane
constexpr int TL_AHEAD = 4;                     // decode: trips whose pred / confidence are in registers before their turn (a
                                                 // load's latency is several trips): the loop's period is TL_AHEAD * TL_TRIP frames
constexpr int TL_MAX_W = 64;
constexpr int TL_MAX_C = 64;
constexpr int TL_STATE = QT_TIMELINE_STATE;
constexpr long long TL_MAX_FRAMES = 1LL << 22;
static_assert(TL_TILE == QT_TIMELINE_TILE && TL_TRIP == QT_TIMELINE_TRIP && TL_MAX_W == QT_TIMELINE_MAX_WINDOW &&
                  TL_MAX_C == QT_TIMELINE_MAX_CLASSES, "the header states these");
static_assert(TL_TRIP == QT_WAVE && TL_STATE == 8, "decode: one lane per frame of a trip");
static_assert((TL_TILE + TL_MAX_W - 1) * TL_MAX_C * 4 <= 32 * 1024, "LDS of the smooth kernel");

struct SmoothArgs {
  const float* probs;
  const float* hist_in;
  const int* hist_count_in;
  float* hist_out;
  int* hist_count_out;
  float* smoothed;
  long long* pred;
  float* conf;
  long long ld, ld_s;
  int T, tiles, C, W, vec;
};

struct DecodeArgs {
  const long long* pred;
  const float* conf;
  long long* state;
  long long* stable;
  long long* segments;
  int T, C, min_run, capacity, flush;
  float min_conf;
};

template <int LANES>
__global__ __launch_bounds__(TL_THREADS) void timeline_smooth_kernel(SmoothArgs a) {
  __shared__ __attribute__((aligned(16))) float rows[(TL_TILE + TL_MAX_W - 1) * TL_MAX_C];   // [slot][C], dense
  const int tid = threadIdx.x;
  const int b = blockIdx.x / a.tiles;
  const int t0 = (blockIdx.x - b * a.tiles) * TL_TILE;
  const int nrows = min(TL_TILE, a.T - t0);
  const int C = a.C, back = a.W - 1;
  const int seen = a.hist_in ? min(max(a.hist_count_in[b], 0), back) : 0;
  const float* __restrict__ p = a.probs + (long long)b * a.T * a.ld;
  const float* __restrict__ h = a.hist_in ? a.hist_in + (long long)b * back * C : nullptr;

  // 1. slot s = row t0 - back + s of the stream
  const int slots = back + nrows, first = t0 - back;
  if (a.vec) {
    const int C4 = C >> 2;
    for (int i = tid; i < slots * C4; i += TL_THREADS) {
      const int s = i / C4, k = (i - s * C4) << 2, g = first + s;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (g >= 0)
        v = *reinterpret_cast<const float4*>(p + (long long)g * a.ld + k);
      else if (-1 - g < seen)
        v = *reinterpret_cast<const float4*>(h + (-1 - g) * C + k);
      *reinterpret_cast<float4*>(rows + s * C + k) = v;
    }
  } else {
    for (int i = tid; i < slots * C; i += TL_THREADS) {
      const int s = i / C, k = i - s * C, g = first + s;
      float v = 0.f;
      if (g >= 0)
        v = p[(long long)g * a.ld + k];
      else if (-1 - g < seen)
        v = h[(-1 - g) * C + k];
      rows[i] = v;
    }
  }
  __syncthreads();

  // 2, 3. sums, mean, argmax; the trip count is the workgroup's, so every lane reaches the DPP steps
  constexpr int PER_PASS = TL_THREADS / LANES;
  const int sub = tid & (LANES - 1);
  for (int f0 = 0; f0 < nrows; f0 += PER_PASS) {
    const int fl = f0 + tid / LANES;
    const bool live = fl < nrows;
    const int f = live ? fl : nrows - 1;           // idle lanes repeat the last frame and store nothing
    const int n = min(a.W, seen + t0 + f + 1);
    float m = -INFINITY;
    int idx = INT_MAX;
    if (sub < C) {
      const float* r = rows + (back + f - (n - 1)) * C + sub;
      float s = r[0];
      for (int j = 1; j < n; ++j) s = s + r[j * C];
      m = s / (float)n;
      if (m != m) m = __int_as_float(0x7fc00000);
      idx = sub;
    }
    float bv = m;
    int bi = idx;
    qt_group_argmax<LANES>(bv, bi);
    if (live) {
      const long long at = (long long)b * a.T + t0 + f;
      if (a.smoothed && sub < C) a.smoothed[at * a.ld_s + sub] = m;
      if (sub == 0) {
        a.pred[at] = (long long)bi;
        a.conf[at] = bv;
      }
    }
  }

  // 4. the history after the stream's last frame: slot s is row T - 1 - s
  if (a.hist_out && t0 + nrows == a.T) {
    float* __restrict__ ho = a.hist_out + (long long)b * back * C;
    for (int i = tid; i < back * C; i += TL_THREADS) {
      const int s = i / C, k = i - s * C;
      ho[i] = rows[(slots - 1 - s) * C + k];
    }
    if (tid == 0) a.hist_count_out[b] = min(back, seen + a.T);
  }
}

__device__ __forceinline__ void put_segment(const DecodeArgs& a, int b, long long slot, long long start, long long len,
                                            long long label, long long conf) {
  if ((unsigned long long)slot >= (unsigned long long)a.capacity) return;   // (a negative slot of a corrupt state too)
  long long* __restrict__ r = a.segments + ((long long)b * a.capacity + slot) * 4;
  r[0] = start;
  r[1] = len;
  r[2] = label;
  r[3] = conf;
}

// a lane's value from the lane in front of it; lane 0 receives `first` (DPP wave_shr:1: no LDS crossbar)
__device__ __forceinline__ int from_lane_before(int v, int first) { return __builtin_amdgcn_update_dpp(first, v, 0x138, 0xf, 0xf, false); }
template <int CTRL, int ROWS> __device__ __forceinline__ int scan_step(int v) {
  return v + __builtin_amdgcn_update_dpp(0, v, CTRL, ROWS, 0xf, false);   // lanes without a source add 0
}
// inclusive prefix sum over the wave: four shifts inside each 16-lane row, then lane 15 of rows 0 and 2 into rows 1 and 3,
// then lane 31 into rows 2 and 3
__device__ __forceinline__ int wave_prefix_sum(int v) {
  v = scan_step<0x111, 0xf>(v);   // row_shr:1
  v = scan_step<0x112, 0xf>(v);   // row_shr:2
  v = scan_step<0x114, 0xf>(v);   // row_shr:4
  v = scan_step<0x118, 0xf>(v);   // row_shr:8
  v = scan_step<0x142, 0xa>(v);   // row_bcast:15
  v = scan_step<0x143, 0xc>(v);   // row_bcast:31
  return v;
}
// the value of one lane (a wave-uniform index) for every lane
__device__ __forceinline__ int of_lane(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }
__device__ __forceinline__ long long of_lane(long long v, int lane) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)v, lane), hi = (unsigned)__builtin_amdgcn_readlane((int)(v >> 32), lane);
  return (long long)(((unsigned long long)hi << 32) | lo);
}

__global__ __launch_bounds__(TL_TRIP) void timeline_decode_kernel(DecodeArgs a) {
  const int lane = threadIdx.x, b = blockIdx.x;
  long long* __restrict__ st = a.state + (long long)b * TL_STATE;
  // the carry between trips (and calls): the state, the same in every lane
  const long long seen0 = st[0];
  int stable_in = (int)st[1] - 1, cand_in = (int)st[2] - 1;
  long long run_in = st[3], start_in = st[4], len_in = st[5], conf_in = st[6], total_in = st[7];
  const long long* __restrict__ pr = a.pred + (long long)b * a.T;
  const float* __restrict__ cf = a.conf + (long long)b * a.T;
  const unsigned long long upto = (2ull << lane) - 1ull;     // lanes 0 .. lane (lane 63: the shift gives 0, minus one all)
  const unsigned long long before = (1ull << lane) - 1ull;   // lanes 0 .. lane - 1

  long long next_p[TL_AHEAD];
  float next_c[TL_AHEAD];
  auto fetch = [&](int base) {
#pragma unroll
    for (int g = 0; g < TL_AHEAD; ++g) {
      const int f = base + g * TL_TRIP + lane;
      next_p[g] = 0;
      next_c[g] = 0.f;
      if (f < a.T) {
        next_p[g] = pr[f];
        next_c[g] = cf[f];
      }
    }
  };
  fetch(0);
  for (int base0 = 0; base0 < a.T; base0 += TL_AHEAD * TL_TRIP) {
    long long now_p[TL_AHEAD];
    float now_c[TL_AHEAD];
#pragma unroll
    for (int g = 0; g < TL_AHEAD; ++g) {
      now_p[g] = next_p[g];
      now_c[g] = next_c[g];
    }
    fetch(base0 + TL_AHEAD * TL_TRIP);
#pragma unroll
    for (int g = 0; g < TL_AHEAD; ++g) {
      const int base = base0 + g * TL_TRIP;
      if (base >= a.T) break;   // (the workgroup's: no lane is left behind)
      const long long p = now_p[g];
      const float conf = now_c[g];
      const int f = base + lane;
      const bool act = f < a.T;
      const int last = min(a.T - base, TL_TRIP) - 1;   // the trip's last frame's lane

      // the frame's class, or -1
      int c = -1;
      if (act && conf >= a.min_conf && p >= 0 && p < (long long)a.C) c = (int)p;
      // run length ending here: the distance to the last lane whose class differs from its predecessor's
      const int c_prev = from_lane_before(c, cand_in);
      unsigned long long m = __ballot(act && c != c_prev) & upto;
      long long run = m ? (long long)(lane - top_bit(m) + 1) : run_in + lane + 1;
      if (run > INT_MAX) run = INT_MAX;
      // stable label: the class at the last lane whose run reached min_run
      m = __ballot(act && run >= (long long)a.min_run) & upto;
      const int c_at = __shfl(c, m ? top_bit(m) : lane, 64);
      const int stable = m ? c_at : stable_in;
      if (act) a.stable[(long long)b * a.T + f] = (long long)stable;

      // segments
      const int s_prev = from_lane_before(stable, stable_in);
      const bool change = act && stable != s_prev;
      const unsigned long long changes = __ballot(change);
      const int q = act ? qt_conf_q(conf) : 0;
      const int incl = wave_prefix_sum(q);   // 64 x 65536 fits
      const int excl = incl - q;
      // the segment in front of this lane: from the last change before it, or from the carry
      m = changes & before;
      const int from = m ? top_bit(m) : 0;
      const int excl_from = __shfl(excl, from, 64);
      const long long p_start = m ? seen0 + base + from : start_in;
      const long long p_len = m ? (long long)(lane - from) : len_in + lane;
      const long long p_conf = m ? (long long)(excl - excl_from) : conf_in + excl;
      const bool closes = change && s_prev >= 0 && p_len > 0;
      const unsigned long long closed = __ballot(closes);
      if (closes) put_segment(a, b, total_in + __popcll(closed & before), p_start, p_len, (long long)s_prev, p_conf);
      // the segment this lane is in
      long long o_start = change ? seen0 + f : p_start, o_len = change ? 1 : p_len + 1, o_conf = change ? (long long)q : p_conf + q;
      if (stable < 0) o_start = o_len = o_conf = 0;

      // the carry is what the trip's last frame's lane holds
      stable_in = of_lane(stable, last);
      cand_in = of_lane(c, last);
      run_in = of_lane(run, last);
      start_in = of_lane(o_start, last);
      len_in = of_lane(o_len, last);
      conf_in = of_lane(o_conf, last);
      total_in += __popcll(closed);
    }
  }

  if (lane == 0) {
    const long long seen = seen0 + a.T;
    if (a.flush) {
      if (stable_in >= 0 && len_in > 0) {
        put_segment(a, b, total_in, start_in, len_in, (long long)stable_in, conf_in);
        ++total_in;
      }
      start_in = stable_in >= 0 ? seen : 0;
      len_in = conf_in = 0;
    }
    st[0] = seen;
    st[1] = stable_in + 1;
    st[2] = cand_in + 1;
    st[3] = run_in;
    st[4] = start_in;
    st[5] = len_in;
    st[6] = conf_in;
    st[7] = total_in;
  }
}

// what both entry points ask of batch, frames and num_classes
int check_shape(const char* who, const qt_timeline_desc* d, bool zero_frames_ok) {
  QT_CHECK_ARG(d->batch >= 1, "%s: batch must be positive (got %d)", who, d->batch);
  QT_CHECK_ARG(d->frames >= 0, "%s: frames must not be negative (got %d)", who, d->frames);
  QT_CHECK_ARG(d->frames >= 1 || zero_frames_ok, "%s: frames == 0 is for qt_timeline_decode with flush only", who);
  QT_CHECK_ARG(d->num_classes >= 1 && d->num_classes <= TL_MAX_C, "%s: num_classes = %d; 1 .. %d are handled", who,
               d->num_classes, TL_MAX_C);
  const long long frames = (long long)d->batch * d->frames;
  if (frames > TL_MAX_FRAMES) {
    qt_set_error("%s: %lld frames in one call; at most %lld are handled", who, frames, TL_MAX_FRAMES);
    return QT_ERR_UNSUPPORTED;
  }
  return QT_OK;
}

}  // namespace

extern "C" int qt_timeline_smooth(const qt_timeline_desc* desc, const float* probs, long long ld, const float* hist_in,
                                  const int* hist_count_in, float* hist_out, int* hist_count_out, float* smoothed,
                                  long long ld_smoothed, long long* pred, float* confidence, void* stream) {
  const char* const who = "qt_timeline_smooth";
  QT_CHECK_ARG(desc != nullptr, "%s: null descriptor", who);
  QT_CHECK_ARG(desc->window >= 1 && desc->window <= TL_MAX_W, "%s: window = %d; 1 .. %d are handled", who, desc->window, TL_MAX_W);
  if (const int rc = check_shape(who, desc, false)) return rc;
  const int C = desc->num_classes, back = desc->window - 1;
  QT_CHECK_ARG(ld >= C, "%s: row stride ld = %lld < C = %d", who, ld, C);
  QT_CHECK_ARG(!smoothed || ld_smoothed >= C, "%s: row stride ld_smoothed = %lld < C = %d", who, ld_smoothed, C);
  QT_CHECK_ARG(probs != nullptr, "%s: null probs", who);
  QT_CHECK_ARG(pred != nullptr && confidence != nullptr, "%s: null %s (pred and confidence are both required)", who,
               pred ? "confidence" : "pred");
  QT_CHECK_ARG(!misaligned(probs, 3) && !misaligned(smoothed, 3) && !misaligned(confidence, 3) && !misaligned(pred, 7),
               "%s: probs, smoothed and confidence must be 4-byte aligned, pred 8-byte", who);
  if (back == 0) hist_in = hist_out = nullptr, hist_count_in = hist_count_out = nullptr;   // W == 1: there is no history
  QT_CHECK_ARG((hist_in != nullptr) == (hist_count_in != nullptr) && (hist_out != nullptr) == (hist_count_out != nullptr),
               "%s: a history and its counts come together (half a history pair)", who);
  QT_CHECK_ARG(!misaligned(hist_in, 3) && !misaligned(hist_out, 3) && !misaligned(hist_count_in, 3) && !misaligned(hist_count_out, 3),
               "%s: the histories and their counts must be 4-byte aligned", who);
  if (hist_in && hist_out) {
    const size_t hb = (size_t)desc->batch * back * C * 4, cb = (size_t)desc->batch * 4;
    QT_CHECK_ARG(!overlap(hist_in, hb, hist_out, hb) && !overlap(hist_count_in, cb, hist_count_out, cb),
                 "%s: hist_out / hist_count_out must not overlap hist_in / hist_count_in (swap two buffers)", who);
  }
  const long long rows = (long long)desc->batch * desc->frames;
  if (smoothed)
    QT_CHECK_ARG(!overlap(probs, (size_t)((rows - 1) * ld + C) * 4, smoothed, (size_t)((rows - 1) * ld_smoothed + C) * 4),
                 "%s: smoothed must not overlap probs (other workgroups still read the rows in front of their tiles)", who);

  SmoothArgs a;
  a.probs = probs;
  a.hist_in = hist_in;
  a.hist_count_in = hist_count_in;
  a.hist_out = hist_out;
  a.hist_count_out = hist_count_out;
  a.smoothed = smoothed;
  a.pred = pred;
  a.conf = confidence;
  a.ld = ld;
  a.ld_s = ld_smoothed;
  a.T = desc->frames;
  a.tiles = qt_cdiv(desc->frames, TL_TILE);
  a.C = C;
  a.W = desc->window;
  a.vec = (C & 3) == 0 && (ld & 3) == 0 && !misaligned(probs, 15) && !misaligned(hist_in, 15);
  const dim3 grid((unsigned)((long long)desc->batch * a.tiles));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (C <= 16) hipLaunchKernelGGL(timeline_smooth_kernel<16>, grid, dim3(TL_THREADS), 0, s, a);
  else hipLaunchKernelGGL(timeline_smooth_kernel<64>, grid, dim3(TL_THREADS), 0, s, a);
  QT_CHECK_LAUNCH();
  return QT_OK;
}

extern "C" int qt_timeline_decode(const qt_timeline_desc* desc, const long long* pred, const float* confidence, long long* state,
                                  long long* stable, long long* segments, void* stream) {
  const char* const who = "qt_timeline_decode";
  QT_CHECK_ARG(desc != nullptr, "%s: null descriptor", who);
  QT_CHECK_ARG(desc->min_run >= 1, "%s: min_run must be at least 1 (got %d)", who, desc->min_run);
  QT_CHECK_ARG(desc->min_confidence == desc->min_confidence, "%s: min_confidence is NaN", who);
  QT_CHECK_ARG(desc->capacity >= 0, "%s: capacity must not be negative (got %d)", who, desc->capacity);
  if (const int rc = check_shape(who, desc, desc->flush != 0)) return rc;
  QT_CHECK_ARG(segments != nullptr || desc->capacity == 0, "%s: null segments with capacity = %d", who, desc->capacity);
  QT_CHECK_ARG(state != nullptr, "%s: null state", who);
  QT_CHECK_ARG(desc->frames == 0 || (pred != nullptr && confidence != nullptr && stable != nullptr), "%s: null %s", who,
               !pred ? "pred" : !confidence ? "confidence" : "stable");
  QT_CHECK_ARG(!misaligned(confidence, 3) && !misaligned(pred, 7) && !misaligned(state, 7) && !misaligned(stable, 7) &&
                   !misaligned(segments, 7),
               "%s: confidence must be 4-byte aligned, pred, state, stable and segments 8-byte", who);
  DecodeArgs a;
  a.pred = pred;
  a.conf = confidence;
  a.state = state;
  a.stable = stable;
  a.segments = segments;
  a.T = desc->frames;
  a.C = desc->num_classes;
  a.min_run = desc->min_run;
  a.capacity = desc->capacity;
  a.flush = desc->flush != 0;
  a.min_conf = desc->min_confidence;
  hipLaunchKernelGGL(timeline_decode_kernel, dim3((unsigned)desc->batch), dim3(TL_TRIP), 0, static_cast<hipStream_t>(stream), a);
  QT_CHECK_LAUNCH();
  return QT_OK;
}
