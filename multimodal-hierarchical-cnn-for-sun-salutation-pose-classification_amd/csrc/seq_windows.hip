// Sequence windows on the device: which windows of seq_len consecutive frames a labelled set of clips gives
// (qt_seq_windows_plan; sqn process/create_sequential_dataset.py:154-171 and cnn+lstm/prepare_sequential_dataset.py:46-62),
// and window batches formed from clips held on the device once: any per-frame row (qt_seq_gather_rows) and f32 pose rows with
// the loaders' imputation (qt_seq_gather_features; 3dcnn/dataloaders.py:186-207).  include/qtcnn.h states the rules in full.
//
// The plan is a stream compaction in three launches on the caller's stream; the launch boundary is the only hand-off between
// workgroups, nothing waits inside a launch:
//   1. counts.  A workgroup of 256 threads owns a span of SW_SPAN = 1024 consecutive frame positions, SW_TRIPS trips of 256,
//      thread = position inside a trip.  It stages the span's labels and the seq_len - 1 behind them in LDS as ints (-1 for a
//      value outside [0, num_classes)); a position is a kept window start iff the label rule holds on the staged labels, a
//      binary search of clip_offsets finds the clip c with offsets[c] <= p < offsets[c + 1], p - offsets[c] is a multiple of
//      the stride and p + seq_len <= offsets[c + 1].  One ballot per trip gives a wave's count and every lane's rank; the 16
//      (trip, wave) counts go to LDS and their sum to partial[workgroup];
//   2. scan.  ONE workgroup turns partial[] into its exclusive prefix sums in place, SW_SCAN = 256 entries per trip with the
//      running total carried in a register, and writes the total to count[0];
//   3. scatter.  Step 1 again (the same flags, the same ranks); a kept start goes to slot partial[workgroup] + the (trip,
//      wave) counts before it + its rank in the wave, when that is below the capacity.  Slots follow positions, so the starts
//      ascend: the reference's order, clips in order and i ascending inside a clip.
// Integer sums only: the same bits on every run.  clip_offsets is read at indices 0 .. clips only, labels at 0 .. frames - 1
// only, whatever the offsets hold (a clip's end is cut at `frames`).
//
// A window's rows are consecutive, so a window is ONE contiguous run of seq_len * row_bytes bytes at an arbitrary source
// offset.  The gathers give every run to a group of 2^k threads (8 .. 256; small runs share a workgroup, a run above 16 KiB
// is cut into contiguous pieces of about that size, one workgroup each).  A run is walked by the destination's address:
// single bytes to the first boundary, units of 16 bytes when source and destination agree modulo 16, of 4 bytes when they
// agree modulo 4, single bytes otherwise, single bytes behind; four units in flight per thread.  A window whose start is
// outside [0, src_rows - seq_len] is 0xFF bytes and reads nothing.  The feature gather walks floats the same way (float4
// where both sides allow, single floats otherwise) and applies qt_pose_features' imputation as it stores.
// No atomics, no zero fill, no host synchronisation; 64-bit byte offsets throughout.
#include <limits.h>
#include <stdint.h>

#include "qt_common.h"

namespace {

constexpr int SW_THREADS = 256;
constexpr int SW_TRIPS = 4;
constexpr int SW_SPAN = 1024;                    // frame positions per workgroup: SW_THREADS * SW_TRIPS
constexpr int SW_SCAN = 256;                     // partials per trip of the scan workgroup
constexpr int SW_MAX_SEQ = 64;
constexpr int SW_WAVES = SW_THREADS / QT_WAVE;
constexpr long long SW_MAX_FRAMES = 1LL << 22;
constexpr int SW_MAX_FEATURES = 1024;
constexpr long long SW_PIECE = 16384;            // bytes of a run per workgroup, about
constexpr int SW_MIN_SHIFT = 3;                  // the smallest group: 8 threads
static_assert(SW_SPAN == SW_THREADS * SW_TRIPS && SW_SCAN == SW_THREADS, "span layout");

struct PlanArgs {
  const long long* labels;
  const int* offsets;
  int* starts;
  long long* out_labels;
  int* partial;
  int frames, clips, T, stride, K, capacity, rule;
};

// the label of the window that starts at position s0 + i, or -1 when there is no such window or it is not kept;
// lab: the staged labels of positions s0 ..
__device__ int window_label(const PlanArgs& a, int s0, const int* lab, int i) {
  const int p = s0 + i;
  if (p + a.T > a.frames) return -1;
  const int v = lab[i + a.T - 1];
  if (v < 0) return -1;
  if (a.rule == QT_SEQ_LABEL_UNIFORM)
    for (int t = 0; t < a.T - 1; ++t)
      if (lab[i + t] != v) return -1;
  int lo = 0, hi = a.clips;                      // the last clip with offsets[clip] <= p (an empty clip is stepped over)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a.offsets[mid] <= p)
      lo = mid;
    else
      hi = mid;
  }
  const int begin = a.offsets[lo], end = min(a.offsets[lo + 1], a.frames);
  if (begin < 0 || begin > p || p + a.T > end || (p - begin) % a.stride != 0) return -1;
  return v;
}

// Steps shared by the count and the scatter kernel: stage the labels, find the kept starts of the span.  v[k]: the label of
// the window at position s0 + k * SW_THREADS + tid or -1; rank[k]: kept starts before it in its wave's trip; wc[k][w]: kept
// starts of wave w in trip k (valid after the barrier this ends on).
__device__ __forceinline__ void span_windows(const PlanArgs& a, int s0, int* lab, int (*wc)[SW_WAVES], int (&v)[SW_TRIPS],
                                             int (&rank)[SW_TRIPS]) {
  const int tid = threadIdx.x, lane = tid & (QT_WAVE - 1), wave = tid / QT_WAVE;
  const int n = min(SW_SPAN + a.T - 1, a.frames - s0);
  for (int i = tid; i < n; i += SW_THREADS) {
    const long long l = a.labels[s0 + i];
    lab[i] = (l >= 0 && l < a.K) ? (int)l : -1;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < SW_TRIPS; ++k) {
    v[k] = window_label(a, s0, lab, k * SW_THREADS + tid);
    const unsigned long long kept = __ballot(v[k] >= 0);
    rank[k] = __popcll(kept & ((1ull << lane) - 1ull));
    if (lane == 0) wc[k][wave] = __popcll(kept);
  }
  __syncthreads();
}

__global__ __launch_bounds__(SW_THREADS) void seq_plan_count_kernel(PlanArgs a) {
  __shared__ int lab[SW_SPAN + SW_MAX_SEQ];
  __shared__ int wc[SW_TRIPS][SW_WAVES];
  int v[SW_TRIPS], rank[SW_TRIPS];
  span_windows(a, (int)blockIdx.x * SW_SPAN, lab, wc, v, rank);
  if (threadIdx.x == 0) {
    int total = 0;
    for (int k = 0; k < SW_TRIPS; ++k)
      for (int w = 0; w < SW_WAVES; ++w) total += wc[k][w];
    a.partial[blockIdx.x] = total;
  }
}

// partial[0 .. n) -> its exclusive prefix sums, in place; count[0] = the total.  One workgroup.
__global__ __launch_bounds__(SW_SCAN) void seq_plan_scan_kernel(int* partial, int n, int* count) {
  __shared__ int wsum[SW_WAVES];
  const int tid = threadIdx.x, lane = tid & (QT_WAVE - 1), wave = tid / QT_WAVE;
  int carry = 0;
  for (int base = 0; base < n; base += SW_SCAN) {
    const int i = base + tid;
    const int own = i < n ? partial[i] : 0;
    int inc = own;                               // inclusive scan over the wave
    for (int d = 1; d < QT_WAVE; d <<= 1) {
      const int o = __shfl_up(inc, d);
      if (lane >= d) inc += o;
    }
    if (lane == QT_WAVE - 1) wsum[wave] = inc;
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < SW_WAVES; ++w) {
      if (w < wave) before += wsum[w];
      total += wsum[w];
    }
    if (i < n) partial[i] = carry + before + inc - own;
    carry += total;
    __syncthreads();
  }
  if (tid == 0) count[0] = carry;
}

__global__ __launch_bounds__(SW_THREADS) void seq_plan_scatter_kernel(PlanArgs a) {
  __shared__ int lab[SW_SPAN + SW_MAX_SEQ];
  __shared__ int wc[SW_TRIPS][SW_WAVES];
  int v[SW_TRIPS], rank[SW_TRIPS];
  const int s0 = (int)blockIdx.x * SW_SPAN;
  span_windows(a, s0, lab, wc, v, rank);
  const int tid = threadIdx.x, wave = tid / QT_WAVE;
  int slot = a.partial[blockIdx.x];              // kept starts before this span
#pragma unroll
  for (int k = 0; k < SW_TRIPS; ++k) {
    int mine = slot + rank[k];
    for (int w = 0; w < SW_WAVES; ++w) {
      if (w < wave) mine += wc[k][w];
      slot += wc[k][w];
    }
    if (v[k] >= 0 && mine < a.capacity) {
      a.starts[mine] = s0 + k * SW_THREADS + tid;
      a.out_labels[mine] = v[k];
    }
  }
}

// ---- the gathers ----------------------------------------------------------------------------------------------------------
// How the runs of a gather are dealt out: a group of 1 << shift threads per piece, `pieces` contiguous pieces per run.
struct Deal {
  int shift, pieces;
  long long items;                               // windows * pieces
  unsigned blocks;
};
bool deal_runs(long long windows, long long run_bytes, Deal* d) {
  int shift = SW_MIN_SHIFT;
  while ((1 << shift) < SW_THREADS && ((long long)64 << shift) < run_bytes) ++shift;   // about four 16-byte units per thread
  d->shift = shift;
  d->pieces = (1 << shift) == SW_THREADS ? (int)((run_bytes + SW_PIECE - 1) / SW_PIECE) : 1;
  d->items = windows * d->pieces;
  const long long blocks = (d->items + (SW_THREADS >> shift) - 1) / (SW_THREADS >> shift);
  d->blocks = (unsigned)blocks;
  return blocks <= INT_MAX;
}

// this thread's (item, lane in its group), false behind the last item
struct Slot {
  long long window;
  int piece, lane, group;
};
__device__ __forceinline__ bool my_slot(int shift, int pieces, long long items, Slot* s) {
  s->group = 1 << shift;
  s->lane = (int)threadIdx.x & (s->group - 1);
  const long long item = (long long)blockIdx.x * (SW_THREADS >> shift) + ((int)threadIdx.x >> shift);
  if (item >= items) return false;
  s->window = item / pieces;
  s->piece = (int)(item - s->window * pieces);
  return true;
}
// units [lo, hi) of a piece: this piece's share of n units
__device__ __forceinline__ void piece_range(long long n, const Slot& s, int pieces, long long* lo, long long* hi) {
  const long long per = (n + pieces - 1) / pieces;
  *lo = min(n, s.piece * per);
  *hi = min(n, *lo + per);
}

template <typename U> __device__ __forceinline__ U all_ones();
template <> __device__ __forceinline__ uint4 all_ones<uint4>() { return make_uint4(~0u, ~0u, ~0u, ~0u); }
template <> __device__ __forceinline__ unsigned all_ones<unsigned>() { return ~0u; }
template <> __device__ __forceinline__ unsigned char all_ones<unsigned char>() { return 0xFF; }

// d[u] = s[u] (or 0xFF.. when fill; s is not read then) for units lo <= u < hi, lane after lane, four loads before four stores
template <typename U>
__device__ __forceinline__ void move_units(const unsigned char* sb, unsigned char* db, long long lo, long long hi, int lane,
                                           int group, bool fill) {
  const U* s = reinterpret_cast<const U*>(sb);
  U* d = reinterpret_cast<U*>(db);
  long long u = lo + lane;
  if (fill) {
    for (; u < hi; u += group) d[u] = all_ones<U>();
    return;
  }
  for (; u + 3LL * group < hi; u += 4LL * group) {
    const U v0 = s[u], v1 = s[u + group], v2 = s[u + 2LL * group], v3 = s[u + 3LL * group];
    d[u] = v0;
    d[u + group] = v1;
    d[u + 2LL * group] = v2;
    d[u + 3LL * group] = v3;
  }
  for (; u < hi; u += group) d[u] = s[u];
}

struct RowsArgs {
  const unsigned char* src;
  unsigned char* dst;
  const int* starts;
  long long src_rows, row_bytes, run_bytes, items;
  int T, pieces, shift;
};

__global__ __launch_bounds__(SW_THREADS) void seq_gather_rows_kernel(RowsArgs a) {
  Slot me;
  if (!my_slot(a.shift, a.pieces, a.items, &me)) return;
  const long long start = a.starts[me.window];
  const bool fill = start < 0 || start > a.src_rows - a.T;
  unsigned char* d = a.dst + me.window * a.run_bytes;
  const unsigned char* s = fill ? d : a.src + start * a.row_bytes;   // (a filled run goes by the destination alone)
  const unsigned apart = (unsigned)(reinterpret_cast<uintptr_t>(s) ^ reinterpret_cast<uintptr_t>(d));
  const int width = (apart & 15u) == 0 ? 16 : ((apart & 3u) == 0 ? 4 : 1);
  const long long head = min(a.run_bytes, (long long)((0 - reinterpret_cast<uintptr_t>(d)) & (uintptr_t)(width - 1)));
  const long long units = (a.run_bytes - head) / width;
  const long long behind = head + units * width;                     // first byte of the tail
  if (me.piece == 0)                                                 // head and tail: at most 15 single bytes each
    for (long long i = me.lane; i < head + (a.run_bytes - behind); i += me.group) {
      const long long o = i < head ? i : behind + (i - head);
      d[o] = fill ? (unsigned char)0xFF : s[o];
    }
  long long lo, hi;
  piece_range(units, me, a.pieces, &lo, &hi);
  if (width == 16)
    move_units<uint4>(s + head, d + head, lo, hi, me.lane, me.group, fill);
  else if (width == 4)
    move_units<unsigned>(s + head, d + head, lo, hi, me.lane, me.group, fill);
  else
    move_units<unsigned char>(s + head, d + head, lo, hi, me.lane, me.group, fill);
}

struct FeatArgs {
  const float* raw;
  const int* starts;
  const long long* labels;
  const float* means;
  const float* stds;
  float* out;
  long long src_rows, items;
  int F, T, K, mode, pieces, shift;
};

// qt_pose_features' imputation of column col under a label inside the tables
__device__ __forceinline__ float impute(const FeatArgs& a, float v, long long label, int col) {
  if (a.mode == QT_POSE_RAW) return v;
  if (a.mode == QT_POSE_ZERO) return v != v ? 0.f : v;
  const float m = a.means[label * a.F + col];
  if (v != v) v = m;
  if (a.mode == QT_POSE_CLASS_MEAN) return v;
  const float sd = a.stds[label * a.F + col];
  return sd < 1e-6f ? 0.f : (v - m) / sd;
}

__global__ __launch_bounds__(SW_THREADS) void seq_gather_features_kernel(FeatArgs a) {
  Slot me;
  if (!my_slot(a.shift, a.pieces, a.items, &me)) return;
  const int n = a.T * a.F;                                           // floats of a run, at most 2^16
  const long long start = a.starts[me.window];
  const bool by_class = a.mode == QT_POSE_CLASS_MEAN || a.mode == QT_POSE_STANDARDIZE;
  const long long label = by_class ? a.labels[me.window] : 0;
  const bool no_rows = start < 0 || start > a.src_rows - a.T;
  const bool no_class = by_class && (label < 0 || label >= a.K);     // nothing is indexed with it
  float* d = a.out + me.window * n;
  const float* s = a.raw + (no_rows ? 0 : start) * a.F;              // not read without rows
  int head = (int)((16u - (unsigned)(reinterpret_cast<uintptr_t>(d) & 15u)) & 15u) >> 2;
  if (head > n) head = n;
  const int nvec = (n - head) >> 2;
  const int behind = head + 4 * nvec;
  // an out-of-range start is 0xFF bytes as in qt_seq_gather_rows, an out-of-range label qt_pose_features' NaN
  const float nothing = no_rows ? __uint_as_float(~0u) : __builtin_nanf("");
  const bool blank = no_rows || no_class;
  if (me.piece == 0)
    for (int i = me.lane; i < head + (n - behind); i += me.group) {
      const int o = i < head ? i : behind + (i - head);
      d[o] = blank ? nothing : impute(a, s[o], label, o % a.F);
    }
  long long lo, hi;
  piece_range(nvec, me, a.pieces, &lo, &hi);
  const bool vec = ((reinterpret_cast<uintptr_t>(s) ^ reinterpret_cast<uintptr_t>(d)) & 15u) == 0;
  for (int u = (int)lo + me.lane; u < (int)hi; u += me.group) {
    const int t = head + 4 * u;
    float v[4];
    if (blank) {
      v[0] = v[1] = v[2] = v[3] = nothing;
    } else {
      if (vec) {
        const float4 q = *reinterpret_cast<const float4*>(s + t);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = s[t + k];
      }
      int c = t % a.F;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        v[k] = impute(a, v[k], label, c);
        if (++c == a.F) c = 0;
      }
    }
    *reinterpret_cast<float4*>(d + t) = make_float4(v[0], v[1], v[2], v[3]);
  }
}

bool overlap(const void* p, long long p_bytes, const void* q, long long q_bytes) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return a < b + (uintptr_t)q_bytes && b < a + (uintptr_t)p_bytes;
}

// descriptor checks shared by the size query and the call; leaves the error text
int plan_desc_status(const qt_seq_windows_desc* desc, const char* who) {
  QT_CHECK_ARG(desc != nullptr, "%s: null descriptor", who);
  QT_CHECK_ARG(desc->frames >= 1 && desc->clips >= 1 && desc->num_classes >= 1 && desc->capacity >= 1,
               "%s: frames, clips, num_classes and capacity must be positive (got %d, %d, %d, %d)", who, desc->frames,
               desc->clips, desc->num_classes, desc->capacity);
  QT_CHECK_ARG(desc->seq_len >= 1 && desc->seq_len <= SW_MAX_SEQ, "%s: seq_len must be 1 .. %d (got %d)", who, SW_MAX_SEQ,
               desc->seq_len);
  QT_CHECK_ARG(desc->stride >= 1, "%s: stride must be positive (got %d)", who, desc->stride);
  QT_CHECK_ARG(desc->rule == QT_SEQ_LABEL_UNIFORM || desc->rule == QT_SEQ_LABEL_LAST,
               "%s: unknown rule %d (QT_SEQ_LABEL_UNIFORM or QT_SEQ_LABEL_LAST)", who, desc->rule);
  if (desc->frames > SW_MAX_FRAMES) {
    qt_set_error("%s: %d frames in one call; at most %lld are handled", who, desc->frames, SW_MAX_FRAMES);
    return QT_ERR_UNSUPPORTED;
  }
  return QT_OK;
}

}  // namespace

extern "C" size_t qt_seq_windows_workspace_bytes(const qt_seq_windows_desc* desc) {
  if (plan_desc_status(desc, "qt_seq_windows_workspace_bytes") != QT_OK) return 0;
  return sizeof(int) * (size_t)qt_cdiv(desc->frames, SW_SPAN);
}

extern "C" int qt_seq_windows_plan(const qt_seq_windows_desc* desc, const long long* labels, const int* clip_offsets, int* starts,
                                   long long* window_labels, int* count, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  const char* const who = "qt_seq_windows_plan";
  const int status = plan_desc_status(desc, who);
  if (status != QT_OK) return status;
  QT_CHECK_ARG(labels != nullptr && clip_offsets != nullptr && starts != nullptr && window_labels != nullptr &&
                   count != nullptr && workspace != nullptr,
               "%s: null labels, clip_offsets, starts, window_labels, count or workspace", who);
  QT_CHECK_ARG(!misaligned(labels, 7) && !misaligned(window_labels, 7),
               "%s: labels and window_labels must be 8-byte aligned", who);
  QT_CHECK_ARG(!misaligned(clip_offsets, 3) && !misaligned(starts, 3) && !misaligned(count, 3) && !misaligned(workspace, 3),
               "%s: clip_offsets, starts, count and workspace must be 4-byte aligned", who);
  const int spans = qt_cdiv(desc->frames, SW_SPAN);
  QT_CHECK_ARG(workspace_bytes >= sizeof(int) * (size_t)spans, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes,
               sizeof(int) * (size_t)spans);
  PlanArgs a;
  a.labels = labels;
  a.offsets = clip_offsets;
  a.starts = starts;
  a.out_labels = window_labels;
  a.partial = static_cast<int*>(workspace);
  a.frames = desc->frames;
  a.clips = desc->clips;
  a.T = desc->seq_len;
  a.stride = desc->stride;
  a.K = desc->num_classes;
  a.capacity = desc->capacity;
  a.rule = desc->rule;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(seq_plan_count_kernel, dim3(spans), dim3(SW_THREADS), 0, st, a);
  QT_CHECK_LAUNCH();
  hipLaunchKernelGGL(seq_plan_scan_kernel, dim3(1), dim3(SW_SCAN), 0, st, a.partial, spans, count);
  QT_CHECK_LAUNCH();
  hipLaunchKernelGGL(seq_plan_scatter_kernel, dim3(spans), dim3(SW_THREADS), 0, st, a);
  QT_CHECK_LAUNCH();
  return QT_OK;
}

extern "C" int qt_seq_gather_rows(const qt_seq_gather_desc* desc, const void* src, const int* starts, void* dst, void* stream) {
  const char* const who = "qt_seq_gather_rows";
  QT_CHECK_ARG(desc != nullptr, "%s: null descriptor", who);
  QT_CHECK_ARG(desc->src_rows >= 1 && desc->row_bytes >= 1 && desc->windows >= 1,
               "%s: src_rows, row_bytes and windows must be positive (got %lld, %lld, %d)", who, desc->src_rows, desc->row_bytes,
               desc->windows);
  QT_CHECK_ARG(desc->seq_len >= 1 && desc->seq_len <= SW_MAX_SEQ, "%s: seq_len must be 1 .. %d (got %d)", who, SW_MAX_SEQ,
               desc->seq_len);
  if (desc->src_rows > INT_MAX || desc->row_bytes > (1LL << 40) / SW_MAX_SEQ) {
    qt_set_error("%s: %lld rows of %lld bytes; at most 2^31 - 1 rows (int32 starts) and runs of 2^40 bytes are handled", who,
                 desc->src_rows, desc->row_bytes);
    return QT_ERR_UNSUPPORTED;
  }
  QT_CHECK_ARG(src != nullptr && starts != nullptr && dst != nullptr, "%s: null source, starts or destination", who);
  QT_CHECK_ARG(!misaligned(starts, 3), "%s: starts must be 4-byte aligned", who);
  RowsArgs a;
  a.run_bytes = desc->seq_len * desc->row_bytes;
  QT_CHECK_ARG(!overlap(src, desc->src_rows * desc->row_bytes, dst, desc->windows * a.run_bytes),
               "%s: source and destination overlap", who);
  Deal deal;
  if (!deal_runs(desc->windows, a.run_bytes, &deal)) {
    qt_set_error("%s: %d windows of %lld bytes are more workgroups than one launch takes", who, desc->windows, a.run_bytes);
    return QT_ERR_UNSUPPORTED;
  }
  a.src = static_cast<const unsigned char*>(src);
  a.dst = static_cast<unsigned char*>(dst);
  a.starts = starts;
  a.src_rows = desc->src_rows;
  a.row_bytes = desc->row_bytes;
  a.items = deal.items;
  a.T = desc->seq_len;
  a.pieces = deal.pieces;
  a.shift = deal.shift;
  hipLaunchKernelGGL(seq_gather_rows_kernel, dim3(deal.blocks), dim3(SW_THREADS), 0, static_cast<hipStream_t>(stream), a);
  QT_CHECK_LAUNCH();
  return QT_OK;
}

extern "C" int qt_seq_gather_features(const qt_seq_features_desc* desc, const float* raw, const int* starts,
                                      const long long* window_labels, const float* means, const float* stds, float* out,
                                      void* stream) {
  const char* const who = "qt_seq_gather_features";
  QT_CHECK_ARG(desc != nullptr, "%s: null descriptor", who);
  QT_CHECK_ARG(desc->src_rows >= 1 && desc->windows >= 1, "%s: src_rows and windows must be positive (got %lld, %d)", who,
               desc->src_rows, desc->windows);
  QT_CHECK_ARG(desc->features >= 1 && desc->features <= SW_MAX_FEATURES, "%s: features must be 1 .. %d (got %d)", who,
               SW_MAX_FEATURES, desc->features);
  QT_CHECK_ARG(desc->seq_len >= 1 && desc->seq_len <= SW_MAX_SEQ, "%s: seq_len must be 1 .. %d (got %d)", who, SW_MAX_SEQ,
               desc->seq_len);
  QT_CHECK_ARG(desc->mode == QT_POSE_RAW || desc->mode == QT_POSE_ZERO || desc->mode == QT_POSE_CLASS_MEAN ||
                   desc->mode == QT_POSE_STANDARDIZE,
               "%s: unknown mode %d", who, desc->mode);
  if (desc->src_rows > INT_MAX) {
    qt_set_error("%s: %lld rows; at most 2^31 - 1 are handled (int32 starts)", who, desc->src_rows);
    return QT_ERR_UNSUPPORTED;
  }
  QT_CHECK_ARG(raw != nullptr && starts != nullptr && out != nullptr, "%s: null rows, starts or output", who);
  QT_CHECK_ARG(!misaligned(raw, 3) && !misaligned(starts, 3) && !misaligned(out, 3) && !misaligned(means, 3) &&
                   !misaligned(stds, 3) && !misaligned(window_labels, 7),
               "%s: rows, starts, output, means and stds must be 4-byte aligned, window_labels 8-byte aligned", who);
  const bool by_class = desc->mode == QT_POSE_CLASS_MEAN || desc->mode == QT_POSE_STANDARDIZE;
  if (by_class) {
    QT_CHECK_ARG(window_labels != nullptr && means != nullptr && desc->num_classes >= 1,
                 "%s: mode %d needs window_labels, class means and num_classes >= 1 (got %d)", who, desc->mode,
                 desc->num_classes);
    QT_CHECK_ARG(desc->mode != QT_POSE_STANDARDIZE || stds != nullptr, "%s: QT_POSE_STANDARDIZE needs class stds", who);
  }
  const long long run_bytes = 4LL * desc->seq_len * desc->features;
  QT_CHECK_ARG(!overlap(raw, 4LL * desc->src_rows * desc->features, out, desc->windows * run_bytes),
               "%s: rows and output overlap", who);
  Deal deal;
  if (!deal_runs(desc->windows, run_bytes, &deal)) {
    qt_set_error("%s: %d windows of %lld bytes are more workgroups than one launch takes", who, desc->windows, run_bytes);
    return QT_ERR_UNSUPPORTED;
  }
  FeatArgs a;
  a.raw = raw;
  a.starts = starts;
  a.labels = by_class ? window_labels : nullptr;
  a.means = by_class ? means : nullptr;
  a.stds = desc->mode == QT_POSE_STANDARDIZE ? stds : nullptr;
  a.out = out;
  a.src_rows = desc->src_rows;
  a.items = deal.items;
  a.F = desc->features;
  a.T = desc->seq_len;
  a.K = by_class ? desc->num_classes : 0;
  a.mode = desc->mode;
  a.pieces = deal.pieces;
  a.shift = deal.shift;
  hipLaunchKernelGGL(seq_gather_features_kernel, dim3(deal.blocks), dim3(SW_THREADS), 0, static_cast<hipStream_t>(stream), a);
  QT_CHECK_LAUNCH();
  return QT_OK;
}
