// What the kernels of the pose-order chain share (pose_order.hip: the decoder and fixed-lag paths; pose_posterior.hip: the
// posteriors, the learner's E-step and fixed-lag posteriors; pose_prior.hip: path counts and the M-step; and, through
// pose_duration_chain.h, which adds what the chain with hold durations alone needs, the pose_duration*.hip files): the limits,
// the emission rule q with its table and the loop that stages a tile's emissions, the chain's inputs as one kernel-argument
// struct, the M-step of a row, and on the host the descriptor checks, the fixed-lag route and span, the checks of an entry
// point's buffers (nulls, alignment, workspace size, overlap) from one list and the S <= 16 template switch.
// The build is not relocatable: every .hip that uses pc_q (pose_order.hip, pose_posterior.hip) has the table in its own code
// object.
#pragma once
#include "qt_common.h"

constexpr int PC_TILE = 64;                      // frames per tile; calls of up to PC_TILE frames take the short routes
constexpr int PC_MAX_S = 64;
constexpr int PC_MAX_C = 64;
constexpr long long PC_MAX_FRAMES = 1LL << 20;
constexpr int PC_FLOOR = -8192;                  // q of NaN and of everything below 2^-32
constexpr int PC_TRANS_FLOOR = -65536;
constexpr int PC_LAG_MAX = 63;
static_assert(PC_TILE == QT_POSE_ORDER_TILE && PC_MAX_S == QT_POSE_ORDER_MAX_STATES && PC_MAX_C == QT_POSE_ORDER_MAX_CLASSES &&
                  PC_LAG_MAX == QT_POSE_LAG_MAX,
              "the header states these");
static_assert(PC_TILE == QT_WAVE, "lane = frame where a tile's frames are spread over a wave");

// rint(256 log2(1 + (2 i + 1) / 512)), i = 0 .. 255 (no entry closer than 0.0015 to a half)
static __device__ const unsigned short PC_LOG2[256] = {
      1,   2,   4,   5,   6,   8,   9,  11,  12,  13,  15,  16,  18,  19,  20,  22,
     23,  24,  26,  27,  28,  30,  31,  32,  34,  35,  36,  38,  39,  40,  42,  43,
     44,  45,  47,  48,  49,  50,  52,  53,  54,  55,  57,  58,  59,  60,  62,  63,
     64,  65,  66,  68,  69,  70,  71,  72,  74,  75,  76,  77,  78,  80,  81,  82,
     83,  84,  85,  86,  88,  89,  90,  91,  92,  93,  94,  95,  97,  98,  99, 100,
    101, 102, 103, 104, 105, 106, 108, 109, 110, 111, 112, 113, 114, 115, 116, 117,
    118, 119, 120, 121, 122, 123, 124, 125, 126, 127, 128, 129, 131, 132, 133, 134,
    135, 136, 137, 138, 139, 140, 140, 141, 142, 143, 144, 145, 146, 147, 148, 149,
    150, 151, 152, 153, 154, 155, 156, 157, 158, 159, 160, 161, 162, 163, 163, 164,
    165, 166, 167, 168, 169, 170, 171, 172, 173, 173, 174, 175, 176, 177, 178, 179,
    180, 181, 182, 182, 183, 184, 185, 186, 187, 188, 189, 189, 190, 191, 192, 193,
    194, 195, 195, 196, 197, 198, 199, 200, 200, 201, 202, 203, 204, 205, 205, 206,
    207, 208, 209, 210, 210, 211, 212, 213, 214, 214, 215, 216, 217, 218, 218, 219,
    220, 221, 222, 222, 223, 224, 225, 226, 226, 227, 228, 229, 229, 230, 231, 232,
    233, 233, 234, 235, 236, 236, 237, 238, 239, 239, 240, 241, 242, 242, 243, 244,
    245, 245, 246, 247, 248, 248, 249, 250, 251, 251, 252, 253, 253, 254, 255, 256
};

// the chain's inputs: the head of every kernel-argument struct of the family
struct PcChain {
  const float* probs;
  const int* state_class;
  const int* trans;
  const int* init;
  long long ld;
  int T, tiles, C, S;          // tiles: T in tiles of PC_TILE frames
  FastDiv div_s, div_c;
};
inline void pc_fill(PcChain& a, const float* probs, long long ld, const int* state_class, const int* trans, const int* init,
                    int T, int C, int S) {
  a.probs = probs;
  a.state_class = state_class;
  a.trans = trans;
  a.init = init;
  a.ld = ld;
  a.T = T;
  a.tiles = qt_cdiv(T, PC_TILE);
  a.C = C;
  a.S = S;
  a.div_s = make_fastdiv((unsigned)S);
  a.div_c = make_fastdiv((unsigned)C);
}

__device__ __forceinline__ int pc_q(float p) {
  if (!(p >= 0x1p-32f)) return PC_FLOOR;         // NaN, negatives, zeros, denormals
  if (p >= 1.0f) return 0;
  const unsigned b = __float_as_uint(p);
  return 256 * ((int)(b >> 23) - 127) + (int)PC_LOG2[(b >> 15) & 255u];
}
__device__ __forceinline__ int pc_clamp_trans(int v) { return min(max(v, PC_TRANS_FLOOR), 0); }
__device__ __forceinline__ float pc_score(int v) { return (float)v * 0x1p-8f; }   // exact: |v| < 2^24

// the emissions of frames [f0, f0 + n) of stream b into e_l [n][S], as the integers q or as scores, and to the emissions
// output ([batch][T][S]) when there is one
__device__ __forceinline__ void pc_put(short* e_l, int idx, int e) { e_l[idx] = (short)e; }
__device__ __forceinline__ void pc_put(float* e_l, int idx, int e) { e_l[idx] = pc_score(e); }
template <typename E>
__device__ __forceinline__ void pc_stage_emissions(const PcChain& a, int b, int f0, int n, E* e_l, int* emissions = nullptr) {
  const int S = a.S;
  const float* __restrict__ p = a.probs + ((long long)b * a.T + f0) * a.ld;
  int* __restrict__ out = emissions ? emissions + ((long long)b * a.T + f0) * S : nullptr;
  for (int idx = threadIdx.x; idx < n * S; idx += blockDim.x) {
    const int f = (int)fdiv((unsigned)idx, a.div_s), s = idx - f * S;
    const int k = a.state_class[s];
    int e = PC_FLOOR;
    if ((unsigned)k < (unsigned)a.C) e = pc_q(p[(long long)f * a.ld + k]);
    pc_put(e_l, idx, e);
    if (out) out[idx] = e;
  }
}

// the M-step of a row of transition (or start) scores (pose_prior.hip, pose_duration_prior.hip).  Row `src` of counts -> `dst`:
// r[j] = allowed ? count + pseudo : 0, R = sum in ascending j; R > 0: rint(256 log2(r / R)) clamped to [-65536, 0] where r > 0
// and -65536 elsewhere; otherwise the old values (zeros where there are none)
__device__ __forceinline__ void pc_update_row(const double* __restrict__ src, const int* __restrict__ allowed, double pseudo,
                                              const int* old, int* dst, int S) {
  double R = 0.0;
  for (int j = 0; j < S; ++j) R += (!allowed || allowed[j]) ? src[j] + pseudo : 0.0;
  for (int j = 0; j < S; ++j) {
    const double rj = (!allowed || allowed[j]) ? src[j] + pseudo : 0.0;
    int v;
    if (R > 0.0) {
      v = PC_TRANS_FLOOR;
      if (rj > 0.0) v = (int)fmin(fmax(rint(256.0 * log2(rj / R)), (double)PC_TRANS_FLOOR), 0.0);
    } else {
      v = old ? old[j] : 0;
    }
    dst[j] = v;
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------------
inline int pc_check_desc(const char* who, const qt_pose_order_desc* d) {
  QT_CHECK_ARG(d != nullptr, "%s: null descriptor", who);
  QT_CHECK_ARG(d->batch >= 1, "%s: batch must be positive (got %d)", who, d->batch);
  QT_CHECK_ARG(d->frames >= 1, "%s: frames must be positive (got %d)", who, d->frames);
  QT_CHECK_ARG(d->num_classes >= 1 && d->num_classes <= PC_MAX_C, "%s: num_classes = %d; 1 .. %d are handled", who,
               d->num_classes, PC_MAX_C);
  QT_CHECK_ARG(d->num_states >= 1 && d->num_states <= PC_MAX_S, "%s: num_states = %d; 1 .. %d are handled", who, d->num_states,
               PC_MAX_S);
  const long long frames = (long long)d->batch * d->frames;
  if (frames > PC_MAX_FRAMES) {
    qt_set_error("%s: %lld frames in one call; at most %lld are handled", who, frames, PC_MAX_FRAMES);
    return QT_ERR_UNSUPPORTED;
  }
  return QT_OK;
}

// the fixed-lag pair (qt_pose_lag_smooth, qt_pose_lag_decode): the descriptor checks, the route and the frames a call emits
inline int pc_lag_check_desc(const char* who, const qt_pose_lag_desc* d) {
  QT_CHECK_ARG(d != nullptr, "%s: null descriptor", who);
  QT_CHECK_ARG(d->batch >= 1, "%s: batch must be positive (got %d)", who, d->batch);
  QT_CHECK_ARG(d->frames >= 0, "%s: frames must not be negative (got %d)", who, d->frames);
  QT_CHECK_ARG(d->frames >= 1 || d->flush, "%s: frames == 0 is a flush only (flush is 0)", who);
  QT_CHECK_ARG(d->num_classes >= 1 && d->num_classes <= PC_MAX_C, "%s: num_classes = %d; 1 .. %d are handled", who,
               d->num_classes, PC_MAX_C);
  QT_CHECK_ARG(d->num_states >= 1 && d->num_states <= PC_MAX_S, "%s: num_states = %d; 1 .. %d are handled", who, d->num_states,
               PC_MAX_S);
  QT_CHECK_ARG(d->lag >= 0 && d->lag <= PC_LAG_MAX, "%s: lag = %d; 0 .. %d are handled", who, d->lag, PC_LAG_MAX);
  QT_CHECK_ARG(d->seen >= 0, "%s: seen must not be negative (got %lld)", who, d->seen);
  const long long frames = (long long)d->batch * d->frames;
  if (frames > PC_MAX_FRAMES) {
    qt_set_error("%s: %lld frames in one call; at most %lld are handled", who, frames, PC_MAX_FRAMES);
    return QT_ERR_UNSUPPORTED;
  }
  return QT_OK;
}
// true: the live route.  QTCNN_POSE_LAG = 1 / 2 forces the live / the batch route (per call); otherwise one new frame, or n
// frames (a flush alone: its pending frames) with n (lag + 1) <= live_steps, the caller's own measured threshold
inline bool pc_lag_live(const qt_pose_lag_desc* d, long long live_steps) {
  const int mode = qt_env_int("QTCNN_POSE_LAG", 0);
  if (mode == 1 || mode == 2) return mode == 1;
  const long long n = d->frames ? d->frames : d->lag;
  return d->frames == 1 || n * (d->lag + 1) <= live_steps;
}
// the frames g0 .. g1 - 1 that a call emits
struct PcSpan {
  long long g0, g1, count;
};
inline PcSpan pc_lag_span(const qt_pose_lag_desc* d) {
  const long long end = d->seen + d->frames;
  PcSpan s;
  s.g0 = d->seen > d->lag ? d->seen - d->lag : 0;
  s.g1 = d->flush ? end : (end > d->lag ? end - d->lag : 0);
  s.count = s.g1 - s.g0;
  return s;
}

// a buffer of an entry point: its extent and name, the alignment its address must have (mask + 1 bytes) and whether it may
// be null
struct PcBuf {
  const void* p;
  size_t bytes;
  const char* name;
  unsigned mask = 0;
  bool required = false;
};
// no output may overlap an input or another output
template <int N_IN, int N_OUT>
inline int pc_check_disjoint(const char* who, const PcBuf (&in)[N_IN], const PcBuf (&out)[N_OUT]) {
  for (const PcBuf& o : out) {
    for (const PcBuf& i : in)
      QT_CHECK_ARG(!overlap(o.p, o.bytes, i.p, i.bytes), "%s: %s must not overlap %s", who, o.name, i.name);
    for (const PcBuf& o2 : out)
      QT_CHECK_ARG(&o == &o2 || !overlap(o.p, o.bytes, o2.p, o2.bytes), "%s: %s must not overlap %s", who, o.name, o2.name);
  }
  return QT_OK;
}

// The checks of an entry point's buffers from its two lists, in the order every entry point keeps: pc_check_present, the first
// required buffer that is null (inputs, then outputs); then the entry's own conditions, spelled out at the site; then
// pc_check_layout: the first misaligned buffer, the workspace's size, the overlaps (the pieces stand alone for an entry with a
// condition of its own between them).  pc_check_bufs is the two in a row.
struct PcRoom {                // the workspace: what the caller gave, what the call needs, and how the message states the need
  const void* p;
  long long bytes, need;
  const char* asks;            // a format for `need`, e.g. "qt_..._workspace_bytes asks for %lld"
};
template <int N_IN, int N_OUT>
inline int pc_check_present(const char* who, const PcBuf (&in)[N_IN], const PcBuf (&out)[N_OUT]) {
  for (const PcBuf& i : in) QT_CHECK_ARG(i.p != nullptr || !i.required, "%s: null %s", who, i.name);
  for (const PcBuf& o : out) QT_CHECK_ARG(o.p != nullptr || !o.required, "%s: null %s", who, o.name);
  return QT_OK;
}
template <int N_IN, int N_OUT>
inline int pc_check_aligned(const char* who, const PcBuf (&in)[N_IN], const PcBuf (&out)[N_OUT]) {
  for (const PcBuf& i : in) QT_CHECK_ARG(!misaligned(i.p, i.mask), "%s: %s must be %u-byte aligned", who, i.name, i.mask + 1);
  for (const PcBuf& o : out) QT_CHECK_ARG(!misaligned(o.p, o.mask), "%s: %s must be %u-byte aligned", who, o.name, o.mask + 1);
  return QT_OK;
}
inline int pc_check_room(const char* who, const PcRoom& room) {
  if (room.need == 0 || (room.p != nullptr && room.bytes >= room.need)) return QT_OK;
  char asks[128];
  snprintf(asks, sizeof asks, room.asks, room.need);
  qt_set_error("%s: workspace of %lld bytes; %s", who, room.p ? room.bytes : 0LL, asks);
  return QT_ERR_INVALID_ARG;
}
template <int N_IN, int N_OUT>
inline int pc_check_layout(const char* who, const PcBuf (&in)[N_IN], const PcBuf (&out)[N_OUT], const PcRoom& room = {}) {
  if (const int rc = pc_check_aligned(who, in, out)) return rc;
  if (const int rc = pc_check_room(who, room)) return rc;
  return pc_check_disjoint(who, in, out);
}
template <int N_IN, int N_OUT>
inline int pc_check_bufs(const char* who, const PcBuf (&in)[N_IN], const PcBuf (&out)[N_OUT], const PcRoom& room = {}) {
  if (const int rc = pc_check_present(who, in, out)) return rc;
  return pc_check_layout(who, in, out, room);
}

// The kernels' SMALL switch (S <= 16: a lane's table entries in registers): calls f with std::true_type or std::false_type; the
// launch itself stays at the site, as with qt_by_dtype:
//   pc_by_small(S, [&](auto small) { hipLaunchKernelGGL(k<PC_SMALL(small)>, ...); });
template <typename F>
inline void pc_by_small(int S, F&& f) {
  if (S <= 16) f(std::true_type{});
  else f(std::false_type{});
}
#define PC_SMALL(tag) decltype(tag)::value
