// Segment-level evaluation on the device (qt_segments_update / qt_segments_encode): the segmental edit score and the
// segmental F1 at IoU thresholds of Lea et al. (CVPR 2017) and the MS-TCN evaluation, counted in integers per video and added
// to a state in device memory, as qt_metrics_update does for frames.  The reference has no such step (its evaluation,
// comparative analysis/analysis.py:60-109, counts frames).  include/qtcnn.h states the rule in full.
//
// Update.  One workgroup of 256 threads per video:
//   (a) runs.  Frames are walked in trips of SG_TRIP = 256, thread = frame.  A frame's class is its value when known, -1
//       otherwise; a run ENDS at a frame whose class is known and differs from the next frame's, and STARTS at one whose class
//       is known and differs from the frame's before.  The thread at a run's end writes the whole run: its slot is the rank of
//       its end (64-bit ballot, plus the ends of the waves and trips before it), its start the last start at or before it (the
//       ballot of starts in its wave, else the last start of an earlier wave of the trip, else the one carried from earlier
//       trips).  What crosses a trip is two integers (ends so far, last start); the per-wave counts go through eight LDS words
//       that alternate between two sets, so a trip costs one barrier.  Runs go to LDS up to QT_SEGMENTS_MAX, the count goes on
//       past it.  Each frame's value and its two neighbours' are loaded by the thread itself (three cached loads, bounded by
//       the video's length), one trip ahead of their use.  qt_segments_encode is the same device function with a writer to
//       global memory;
//   (b) the frame counts, one more pass over the two rows, summed through LDS atomics;
//   (c) the Levenshtein table by anti-diagonals d = i + j, three rotating diagonals of QT_SEGMENTS_MAX + 1 int32 in LDS indexed
//       by i, thread = cell, one barrier per diagonal, at most 2049 diagonals;
//   (d) matching.  Thread = predicted run; a plain scan of the true runs (all lanes read the same LDS word), fractions compared
//       by cross-multiplication in int64, the first best kept; one LDS atomic OR of the passed thresholds' bits on the partner;
//       bits counted by ballot;
//   (e) thread 0 writes the video's record to the workspace.
// A second launch of ONE workgroup sums the records of the workspace into the state (integer atomics: 10 + K per call) and
// copies them to `records` when asked.  Static LDS of the update kernel: 40 KiB.
// No workgroup waits for another inside a launch, no zero fill, no host synchronisation; inputs are never written; nothing
// outside [0, len_b) of a row is read.
#include <stdint.h>

#include "qt_common.h"

namespace {

constexpr int SG_THREADS = 256;
constexpr int SG_TRIP = 256;                     // frames per trip: one per thread
constexpr int SG_WAVES = SG_THREADS / QT_WAVE;
constexpr int SG_MAX = QT_SEGMENTS_MAX;
constexpr int SG_MAX_C = QT_SEGMENTS_MAX_CLASSES;
constexpr int SG_MAX_K = QT_SEGMENTS_MAX_THRESHOLDS;
constexpr int SG_RECORD = QT_SEGMENTS_RECORD;
constexpr int SG_STATE = QT_SEGMENTS_STATE;
constexpr long long SG_MAX_FRAMES = 1LL << 22;
static_assert(SG_TRIP == SG_THREADS && SG_RECORD == 5 && SG_STATE == 10 && SG_MAX_K == 8, "the header states these");
static_assert((6 * SG_MAX + 3 * (SG_MAX + 1) + SG_MAX + 64) * 4 < 64 * 1024, "LDS of the update kernel");

struct UpdateArgs {
  const long long* pred;
  const long long* label;
  const int* lengths;
  long long* work;      // [batch][SG_RECORD + K]
  long long ld_pred, ld_label;
  int T, C, K;
  int pct[SG_MAX_K];
};

struct SumArgs {
  const long long* work;
  long long* state;
  long long* records;
  int batch, K;
};

struct EncodeArgs {
  const long long* values;
  const int* lengths;
  int* runs;
  int* counts;
  long long ld;
  int T, C, capacity;
};

__device__ __forceinline__ int known_class(long long v, int C) { return v >= 0 && v < (long long)C ? (int)v : -1; }
__device__ __forceinline__ int video_length(const int* lengths, int b, int T) { return lengths ? min(max(lengths[b], 0), T) : T; }

// The runs of row[0 .. len): put(slot, start, length, class) is called once per run by the thread at its last frame, slots
// ascending by start; returns the number of runs (in every thread).  `sh`: 2 x 2 x SG_WAVES ints of LDS.  Every thread of the
// workgroup calls it with the same len; the caller puts a barrier between two calls and before it reads what put wrote.
template <typename Put>
__device__ __forceinline__ int extract_runs(const long long* __restrict__ row, int len, int C, int* sh, Put put) {
  const int tid = threadIdx.x, lane = tid & (QT_WAVE - 1), wave = tid / QT_WAVE;
  const unsigned long long before = (1ull << lane) - 1ull, upto = before | (1ull << lane);
  int count = 0, open_start = 0;
  // frame f's class and its two neighbours'; outside [0, len) nothing is loaded and the class is -1
  auto fetch = [&](int f, int& c, int& c_prev, int& c_next) {
    c = c_prev = c_next = -1;
    if (f < len) {
      c = known_class(row[f], C);
      if (f > 0) c_prev = known_class(row[f - 1], C);
      if (f + 1 < len) c_next = known_class(row[f + 1], C);
    }
  };
  int c, c_prev, c_next, ahead, ahead_prev, ahead_next;
  fetch(tid, ahead, ahead_prev, ahead_next);
  for (int base = 0, trip = 0; base < len; base += SG_TRIP, ++trip) {
    const int f = base + tid;
    c = ahead, c_prev = ahead_prev, c_next = ahead_next;
    fetch(f + SG_TRIP, ahead, ahead_prev, ahead_next);   // the next trip's loads are in flight across this trip's barrier
    const bool starts = c >= 0 && c != c_prev, ends = c >= 0 && c != c_next;
    const unsigned long long sb = __ballot(starts), eb = __ballot(ends);
    int* s = sh + (trip & 1) * 2 * SG_WAVES;
    if (lane == 0) {
      s[wave] = __popcll(eb);
      s[SG_WAVES + wave] = sb ? base + wave * QT_WAVE + top_bit(sb) : -1;
    }
    __syncthreads();
    int slot = count + __popcll(eb & before), total = 0, last = open_start, mine = open_start;
#pragma unroll
    for (int w = 0; w < SG_WAVES; ++w) {
      const int ne = s[w], ls = s[SG_WAVES + w];
      if (w < wave) {
        slot += ne;
        if (ls >= 0) mine = ls;
      }
      total += ne;
      if (ls >= 0) last = ls;
    }
    if (ends) {
      const unsigned long long m = sb & upto;
      const int start = m ? base + wave * QT_WAVE + top_bit(m) : mine;
      put(slot, start, f + 1 - start, c);
    }
    count += total;
    open_start = last;
  }
  return count;
}

__global__ __launch_bounds__(SG_THREADS) void segments_update_kernel(UpdateArgs a) {
  __shared__ int p_start[SG_MAX], p_end[SG_MAX], p_cls[SG_MAX];
  __shared__ int y_start[SG_MAX], y_end[SG_MAX], y_cls[SG_MAX];
  __shared__ int diag[3 * (SG_MAX + 1)];
  __shared__ unsigned passed[SG_MAX];            // per true run: bit k = some predicted run passed threshold k with it
  __shared__ int trip_sh[2 * 2 * SG_WAVES];
  __shared__ int sums[2 + SG_MAX_K];             // frames_labelled, frames_correct, tp_k
  const int tid = threadIdx.x, lane = tid & (QT_WAVE - 1), b = blockIdx.x;
  const int len = video_length(a.lengths, b, a.T);
  const long long* __restrict__ pr = a.pred + (long long)b * a.ld_pred;
  const long long* __restrict__ lb = a.label + (long long)b * a.ld_label;

  for (int i = tid; i < SG_MAX; i += SG_THREADS) passed[i] = 0u;
  if (tid < 2 + SG_MAX_K) sums[tid] = 0;

  // (a)
  const int m = extract_runs(pr, len, a.C, trip_sh, [&](int slot, int start, int length, int c) {
    if (slot < SG_MAX) {
      p_start[slot] = start;
      p_end[slot] = start + length;
      p_cls[slot] = c;
    }
  });
  __syncthreads();
  const int n = extract_runs(lb, len, a.C, trip_sh, [&](int slot, int start, int length, int c) {
    if (slot < SG_MAX) {
      y_start[slot] = start;
      y_end[slot] = start + length;
      y_cls[slot] = c;
    }
  });

  // (b)
  int labelled = 0, correct = 0;
#pragma unroll 4
  for (int f = tid; f < len; f += SG_THREADS) {
    const long long l = lb[f];
    if (l >= 0 && l < (long long)a.C) {
      ++labelled;
      correct += pr[f] == l;
    }
  }
  __syncthreads();   // the zeroed sums, and every run
  if (labelled) atomicAdd(&sums[0], labelled);
  if (correct) atomicAdd(&sums[1], correct);

  const bool overflow = m > SG_MAX || n > SG_MAX;   // the workgroup's
  int D = -1;
  if (!overflow) {
    // (c) diagonal d holds D[i][d - i] at index i
    for (int d = 0; d <= m + n; ++d) {
      int* cur = diag + (d % 3) * (SG_MAX + 1);
      const int* d1 = diag + ((d + 2) % 3) * (SG_MAX + 1);
      const int* d2 = diag + ((d + 1) % 3) * (SG_MAX + 1);
      const int hi = min(m, d);
      for (int i = max(0, d - n) + tid; i <= hi; i += SG_THREADS) {
        const int j = d - i;
        int v;
        if (i == 0) v = j;
        else if (j == 0) v = i;
        else v = min(min(d1[i - 1], d1[i]) + 1, d2[i - 1] + (p_cls[i - 1] != y_cls[j - 1]));
        cur[i] = v;
      }
      __syncthreads();
    }
    D = diag[((m + n) % 3) * (SG_MAX + 1) + m];

    // (d)
    for (int i = tid; i < m; i += SG_THREADS) {
      const int ps = p_start[i], pe = p_end[i], c = p_cls[i];
      long long best_inter = 0, best_union = 1;
      int best = -1;
      for (int y = 0; y < n; ++y) {
        if (y_cls[y] != c) continue;
        const int ys = y_start[y], ye = y_end[y];
        const long long inter = max(0, min(pe, ye) - max(ps, ys)), uni = max(pe, ye) - min(ps, ys);
        if (best < 0 || inter * best_union > best_inter * uni) {   // strictly better: a tie keeps the lower index
          best = y;
          best_inter = inter;
          best_union = uni;
        }
      }
      if (best >= 0) {
        unsigned bits = 0u;
        for (int k = 0; k < a.K; ++k)
          if (100 * best_inter >= (long long)a.pct[k] * best_union) bits |= 1u << k;
        if (bits) atomicOr(&passed[best], bits);
      }
    }
    __syncthreads();
    for (int y0 = 0; y0 < n; y0 += SG_THREADS) {   // (the trip count is the workgroup's: every lane reaches the ballots)
      const unsigned bits = y0 + tid < n ? passed[y0 + tid] : 0u;
      for (int k = 0; k < a.K; ++k) {
        const unsigned long long hit = __ballot((bits >> k) & 1u);
        if (lane == 0 && hit) atomicAdd(&sums[2 + k], __popcll(hit));
      }
    }
  }
  __syncthreads();

  // (e)
  if (tid == 0) {
    long long* __restrict__ r = a.work + (long long)b * (SG_RECORD + a.K);
    r[0] = m;
    r[1] = n;
    r[2] = D;
    r[3] = sums[0];
    r[4] = sums[1];
    for (int k = 0; k < a.K; ++k) r[SG_RECORD + k] = overflow ? -1 : sums[2 + k];
  }
}

// one workgroup: the records of the workspace into the state, and to `records`
__global__ __launch_bounds__(SG_THREADS) void segments_sum_kernel(SumArgs a) {
  __shared__ unsigned long long acc[SG_STATE + SG_MAX_K];
  const int tid = threadIdx.x, W = SG_RECORD + a.K;
  if (tid < SG_STATE + SG_MAX_K) acc[tid] = 0ull;
  __syncthreads();
  long long part[SG_STATE + SG_MAX_K];
#pragma unroll
  for (int i = 0; i < SG_STATE + SG_MAX_K; ++i) part[i] = 0;
  for (int b = tid; b < a.batch; b += SG_THREADS) {
    const long long* __restrict__ r = a.work + (long long)b * W;
    const long long m = r[0], n = r[1], D = r[2];
    if (a.records) {
      long long* __restrict__ o = a.records + (long long)b * W;
      for (int i = 0; i < W; ++i) o[i] = r[i];
    }
    part[0] += 1;
    part[8] += r[3];
    part[9] += r[4];
    if (D < 0) {
      part[1] += 1;
      continue;
    }
    const long long M = m > n ? m : n;
    part[3] += m;
    part[4] += n;
    if (M == 0) {
      part[2] += 1;
    } else {
      part[5] += D;
      part[6] += M;
      part[7] += ((M - D) << 32) / M;
    }
#pragma unroll
    for (int k = 0; k < SG_MAX_K; ++k)
      if (k < a.K) part[SG_STATE + k] += r[SG_RECORD + k];
  }
#pragma unroll
  for (int i = 0; i < SG_STATE + SG_MAX_K; ++i)
    if (part[i]) atomicAdd(&acc[i], (unsigned long long)part[i]);
  __syncthreads();
  if (tid < SG_STATE + a.K && acc[tid]) atomicAdd(reinterpret_cast<unsigned long long*>(a.state) + tid, acc[tid]);
}

__global__ __launch_bounds__(SG_THREADS) void segments_encode_kernel(EncodeArgs a) {
  __shared__ int trip_sh[2 * 2 * SG_WAVES];
  const int b = blockIdx.x;
  const int len = video_length(a.lengths, b, a.T);
  int* __restrict__ out = a.runs + (long long)b * a.capacity * 3;
  const int total = extract_runs(a.values + (long long)b * a.ld, len, a.C, trip_sh, [&](int slot, int start, int length, int c) {
    if (slot < a.capacity) {
      out[slot * 3 + 0] = start;
      out[slot * 3 + 1] = length;
      out[slot * 3 + 2] = c;
    }
  });
  if (threadIdx.x == 0) a.counts[b] = total;
}

// what both entry points ask of batch, frames and num_classes
int check_shape(const char* who, const qt_segments_desc* d) {
  QT_CHECK_ARG(d->batch >= 1, "%s: batch must be positive (got %d)", who, d->batch);
  QT_CHECK_ARG(d->frames >= 0, "%s: frames must not be negative (got %d)", who, d->frames);
  QT_CHECK_ARG(d->num_classes >= 1 && d->num_classes <= SG_MAX_C, "%s: num_classes = %d; 1 .. %d are handled", who, d->num_classes,
               SG_MAX_C);
  return QT_OK;
}
int check_frames(const char* who, const qt_segments_desc* d) {
  const long long frames = (long long)d->batch * d->frames;
  if (frames > SG_MAX_FRAMES || d->batch > SG_MAX_FRAMES) {
    qt_set_error("%s: %d videos of %d frames in one call; at most %lld frames (and videos) are handled", who, d->batch, d->frames,
                 SG_MAX_FRAMES);
    return QT_ERR_UNSUPPORTED;
  }
  return QT_OK;
}
int check_thresholds(const char* who, const qt_segments_desc* d) {
  QT_CHECK_ARG(d->num_thresholds >= 1 && d->num_thresholds <= SG_MAX_K, "%s: num_thresholds = %d; 1 .. %d are handled", who,
               d->num_thresholds, SG_MAX_K);
  for (int k = 0; k < d->num_thresholds; ++k)
    QT_CHECK_ARG(d->pct[k] >= 1 && d->pct[k] <= 100, "%s: pct[%d] = %d; thresholds are 1 .. 100 per cent", who, k, d->pct[k]);
  return QT_OK;
}

}  // namespace

extern "C" size_t qt_segments_workspace_bytes(const qt_segments_desc* desc) {
  if (!desc || desc->batch < 1 || desc->num_thresholds < 1 || desc->num_thresholds > SG_MAX_K) return 0;
  return (size_t)desc->batch * (SG_RECORD + desc->num_thresholds) * sizeof(long long);
}

extern "C" int qt_segments_update(const qt_segments_desc* desc, const long long* pred, long long ld_pred, const long long* label,
                                  long long ld_label, const int* lengths, long long* state, long long* records, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  const char* const who = "qt_segments_update";
  QT_CHECK_ARG(desc != nullptr, "%s: null descriptor", who);
  if (const int rc = check_shape(who, desc)) return rc;
  if (const int rc = check_thresholds(who, desc)) return rc;
  QT_CHECK_ARG(ld_pred >= desc->frames, "%s: row stride ld_pred = %lld < frames = %d", who, ld_pred, desc->frames);
  QT_CHECK_ARG(ld_label >= desc->frames, "%s: row stride ld_label = %lld < frames = %d", who, ld_label, desc->frames);
  QT_CHECK_ARG(desc->frames == 0 || (pred != nullptr && label != nullptr), "%s: null %s", who, !pred ? "pred" : "label");
  QT_CHECK_ARG(state != nullptr, "%s: null state", who);
  QT_CHECK_ARG(workspace != nullptr, "%s: null workspace", who);
  QT_CHECK_ARG(!misaligned(pred, 7) && !misaligned(label, 7) && !misaligned(state, 7) && !misaligned(records, 7) &&
                   !misaligned(workspace, 7) && !misaligned(lengths, 3),
               "%s: pred, label, state, records and workspace must be 8-byte aligned, lengths 4-byte", who);
  const size_t need = qt_segments_workspace_bytes(desc);
  QT_CHECK_ARG(workspace_bytes >= need, "%s: workspace of %zu bytes; qt_segments_workspace_bytes asks for %zu", who, workspace_bytes,
               need);
  if (const int rc = check_frames(who, desc)) return rc;

  UpdateArgs u;
  u.pred = pred;
  u.label = label;
  u.lengths = lengths;
  u.work = static_cast<long long*>(workspace);
  u.ld_pred = ld_pred;
  u.ld_label = ld_label;
  u.T = desc->frames;
  u.C = desc->num_classes;
  u.K = desc->num_thresholds;
  for (int k = 0; k < SG_MAX_K; ++k) u.pct[k] = k < u.K ? desc->pct[k] : 100;
  SumArgs s;
  s.work = u.work;
  s.state = state;
  s.records = records;
  s.batch = desc->batch;
  s.K = u.K;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(segments_update_kernel, dim3((unsigned)desc->batch), dim3(SG_THREADS), 0, st, u);
  QT_CHECK_LAUNCH();
  hipLaunchKernelGGL(segments_sum_kernel, dim3(1), dim3(SG_THREADS), 0, st, s);
  QT_CHECK_LAUNCH();
  return QT_OK;
}

extern "C" int qt_segments_encode(const qt_segments_desc* desc, const long long* values, long long ld, const int* lengths, int* runs,
                                  int* counts, void* stream) {
  const char* const who = "qt_segments_encode";
  QT_CHECK_ARG(desc != nullptr, "%s: null descriptor", who);
  if (const int rc = check_shape(who, desc)) return rc;
  QT_CHECK_ARG(desc->capacity >= 0, "%s: capacity must not be negative (got %d)", who, desc->capacity);
  QT_CHECK_ARG(ld >= desc->frames, "%s: row stride ld = %lld < frames = %d", who, ld, desc->frames);
  QT_CHECK_ARG(desc->frames == 0 || values != nullptr, "%s: null values", who);
  QT_CHECK_ARG(counts != nullptr, "%s: null counts", who);
  QT_CHECK_ARG(runs != nullptr || desc->capacity == 0, "%s: null runs with capacity = %d", who, desc->capacity);
  QT_CHECK_ARG(!misaligned(values, 7) && !misaligned(lengths, 3) && !misaligned(runs, 3) && !misaligned(counts, 3),
               "%s: values must be 8-byte aligned, lengths, runs and counts 4-byte", who);
  if (const int rc = check_frames(who, desc)) return rc;
  if ((long long)desc->batch * desc->capacity * 3 > (1LL << 31) - 1) {
    qt_set_error("%s: batch x capacity x 3 = %lld ints of runs; below 2^31 are handled", who, (long long)desc->batch * desc->capacity * 3);
    return QT_ERR_UNSUPPORTED;
  }
  EncodeArgs e;
  e.values = values;
  e.lengths = lengths;
  e.runs = runs;
  e.counts = counts;
  e.ld = ld;
  e.T = desc->frames;
  e.C = desc->num_classes;
  e.capacity = desc->capacity;
  hipLaunchKernelGGL(segments_encode_kernel, dim3((unsigned)desc->batch), dim3(SG_THREADS), 0, static_cast<hipStream_t>(stream), e);
  QT_CHECK_LAUNCH();
  return QT_OK;
}
