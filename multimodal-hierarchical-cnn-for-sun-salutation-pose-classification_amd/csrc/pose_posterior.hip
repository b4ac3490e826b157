// Pose-order posteriors on the device (qt_pose_posterior): the marginals of the hidden-Markov chain that qt_pose_order_decode
// (pose_order.hip) maximises, by forward-backward in log2.  Emissions are the decoder's integers q (the same rule and table, pinned
// by tests/test_pose_posterior_gpu.py), scores are in units of 1/256 bit and exact in f32; every L x = log2 sum 2^x[i] is taken
// with its maximum out and its sum in ascending order, so nothing is infinite for any table in range and every run gives the
// same bits; whatever grows with the frame count is a double.  include/qtcnn.h states the rule in full.
// The rule q, its table, the loop that stages a tile's emissions, the limits PC_*, the chain's inputs PcChain and the host's
// shared checks are in pose_chain.h, once for the decoder and for this file: the posterior's bits rest on that q.
//
// Short route (frames <= PC_TILE): one launch, one wave per stream, lane = state, no workspace.  The table (row stride S | 1: a
// column for the forward step and a row for the backward one are both free of bank conflicts), the tile's emissions and its a_f
// rows are in LDS.  A forward step is the decoder's vector step with (L, +) for (max, +): S times { v_readlane of a_prev[i], add
// the table entry }, a tree of maxima, the sum of v_exp_f32 in ascending i, v_log_f32; for S <= 16 the lane's column (and, for the
// backward step, its row) is in registers.  Then c_f = L_j A_f[j] over the lanes (S readlanes for the maximum, S for the sum), so
// that the next frame starts from the a_f of the rule and a split into calls changes no bit.  The backward sweep walks the same
// LDS rows, one frame per step, overwrites a_f with the posterior and stores it; class_posterior is summed from those rows at the
// end (thread = (frame, class), ascending j).
// Tiled route (frames > PC_TILE), three launches, M_f[i][j] = T[i][j] + E[f][j]:
//   (a) pp_products: a workgroup of 256 per (stream, tile) forms P = M_a (x) ... (x) M_b in the (L, +) semiring in LDS, thread =
//       (i, j), two buffers in turn, one barrier per frame.  Row i is a forward filter started at state i: every frame takes the
//       row's maximum out (each thread finds it while it reads the row) and adds it to the row's offset, a double;
//   (b) pp_scan: a workgroup per stream; wave 0, lane = state, carries the start vector forward through the products of tiles
//       0 .. tiles - 2 (offsets added in double, the maximum out before going back to f32) and the end vector backward through
//       those of tiles tiles - 1 .. 1, while all four waves stage the next trip's products (16 KB, at most 16) through registers
//       into the other LDS buffer.  It leaves every tile's start a, end b and the evidence before the tile in the workspace;
//   (c) pp_replay: a wave per (stream, tile) replays its frames from its start a with the short route's step (filtered, the a_f
//       rows in LDS), sweeps backward from its end b and writes the outputs; the stream's last tile writes the carry.
// f32 (L, +) products are not exactly associative, so (a)-(c) differ from the frame-by-frame rule by rounding.
// No workgroup waits for another inside a launch, no atomics, no zero fill, no host synchronisation; every order is fixed; the
// workspace is the caller's and every slot that is read has been written in the same call.
// qt_pose_prior_expect (the learner's E-step, further down) runs (a) and (b) as they are and a replay of its own that sums the
// pairwise posteriors instead of storing rows; qt_pose_prior_count_paths and qt_pose_prior_update are in pose_prior.hip.
// QTCNN_POSE_POSTERIOR=1 (consulted per call; measurements only, scripts/bench_pose_posterior.py): the short route's algorithm as
// ONE wave per stream over all tiles, the a_f rows parked in the posterior output between the two sweeps.
#include <stdint.h>

#include "pose_chain.h"

namespace {

constexpr float PP_PAD = -1e30f;                 // a candidate in a slot beyond S: never the maximum, and 2^(it - m) is 0
constexpr int PP_SCAN_FLOATS = 4096;             // (b): floats of products per trip
constexpr int PP_SCAN_MAX_TILES = 16;            // (b): products per trip at the most
constexpr int PP_SCAN_PAD = PP_SCAN_MAX_TILES * 16;   // a trip's tiles * S <= 256 for every S: the rows' padding to S | 1, the offsets
constexpr int PP_PROD_THREADS = 256;
constexpr int PP_SCAN_THREADS = 256;
static_assert(PP_SCAN_FLOATS >= PC_MAX_S * PC_MAX_S && PP_SCAN_FLOATS % PP_SCAN_THREADS == 0, "a trip holds at least one product");

// what the tiled route's products and scan read and leave, and the learner's replay as well as the posterior's
struct PpTiles : PcChain {
  double* offsets;           // workspace: double [batch][tiles][S], the products' row offsets
  double* before;            //            double [batch][tiles], the evidence before the tile
  float* products;           //            f32 [batch][tiles][S][S], row maximum 0
  float* starts;             //            f32 [batch][tiles][S], a in front of the tile's first frame
  float* ends;               //            f32 [batch][tiles][S], b at the tile's last frame
};
struct PpArgs : PpTiles {
  double* carry;
  float* posterior;
  float* filtered;
  float* class_posterior;
  double* evidence;
};

__device__ __forceinline__ float pp_trans(int v) { return pc_score(pc_clamp_trans(v)); }

__device__ __forceinline__ float pp_exp2(float x) { return __builtin_amdgcn_exp2f(x); }   // v_exp_f32; x <= 0 here
__device__ __forceinline__ float pp_log2(float x) { return __builtin_amdgcn_logf(x); }    // v_log_f32; x in [1, S] here
// log2 of a sum s in [1, S] in two parts, s = 2^k t with t in [1, 2): k is exact and log2 t < 1 keeps 2^-24 where log2 s, up to 6,
// keeps 2^-22.  Where the maximum in front of it is about -log2 s (a normalised vector, a flat table) m + k is exact and the sum
// keeps the better figure; c_f takes the parts as doubles.
__device__ __forceinline__ void pp_log2_parts(float s, float& k, float& lt) {
  const unsigned b = __float_as_uint(s);
  k = (float)((int)(b >> 23) - 127);
  lt = pp_log2(__uint_as_float((b & 0x007FFFFFu) | 0x3F800000u));
}
__device__ __forceinline__ float pp_m_plus_log2(float m, float s) {
  float k, lt;
  pp_log2_parts(s, k, lt);
  return (m + k) + lt;
}
__device__ __forceinline__ float pp_lane(float v, int i) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), i));
}
__device__ __forceinline__ double pp_lane(double v, int i) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), i), __builtin_amdgcn_readlane(__double2loint(v), i));
}
template <typename V>
__device__ __forceinline__ V pp_max16(V (&t)[16]) {
#pragma unroll
  for (int w = 8; w >= 1; w >>= 1)
#pragma unroll
    for (int i = 0; i < w; ++i) t[i] = t[i + w] > t[i] ? t[i + w] : t[i];
  return t[0];
}

// over the states of a per-lane value (one wave, lane = state; lanes >= S hold state S - 1 again), every lane receives the
// result.  SMALL: S <= 16, sixteen readlanes and a tree, no loop.
template <bool SMALL, typename V>
__device__ __forceinline__ V pp_max_states(V v, int S) {
  if (SMALL) {
    V t[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) t[i] = pp_lane(v, i);
    return pp_max16(t);
  }
  V m = pp_lane(v, 0);
  for (int i = 1; i < S; ++i) {
    const V o = pp_lane(v, i);
    m = o > m ? o : m;
  }
  return m;
}
// L over the states: the maximum m and lg = log2 of the sum, in ascending state, of 2^(v - m); c = m + lg from lg's parts.
// live: lane < S.  SMALL: the lanes S .. 15 contribute zeros behind the last state, which changes no bit of the sum.
template <bool SMALL>
__device__ __forceinline__ void pp_L_states(float v, int S, bool live, float& m, float& lg, double& c) {
  m = pp_max_states<SMALL>(v, S);
  const float p = live ? pp_exp2(v - m) : 0.0f;
  float s = pp_lane(p, 0);
  if (SMALL) {
#pragma unroll
    for (int i = 1; i < 16; ++i) s += pp_lane(p, i);
  } else {
    for (int i = 1; i < S; ++i) s += pp_lane(p, i);
  }
  float k, lt;
  pp_log2_parts(s, k, lt);
  lg = k + lt;
  c = ((double)m + (double)k) + (double)lt;
}
template <bool SMALL>
__device__ __forceinline__ void pp_L_states(float v, int S, bool live, float& m, float& lg) {
  double c;
  pp_L_states<SMALL>(v, S, live, m, lg, c);
}

// sixteen table entries of a lane into registers; slots >= S hold PP_PAD, which changes no maximum and adds 0 to a sum
__device__ __forceinline__ void pp_load16(float (&reg)[16], const float* __restrict__ tab, int stride, int S) {
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const float v = tab[(k < S ? k : 0) * stride];
    reg[k] = k < S ? v : PP_PAD;
  }
}

// L_k (bc[k] + table[k]) for one lane: bc[k] is lane k's value, table[k] the lane's own entry (a column of the table going
// forward, a row going backward).  SMALL: S <= 16, the entries in `reg`; otherwise tab[k * stride] in LDS.
template <bool SMALL>
__device__ __forceinline__ float pp_step(float bc, const float (&reg)[16], const float* __restrict__ tab, int stride, int S) {
  if (SMALL) {
    float x[16], t[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) t[k] = x[k] = pp_lane(bc, k) + reg[k];   // (lanes S .. 15 hold finite values; reg pads them out)
    const float m = pp_max16(t);
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < 16; ++k) s += pp_exp2(x[k] - m);
    return pp_m_plus_log2(m, s);
  }
  float m = pp_lane(bc, 0) + tab[0];
  for (int k = 1; k < S; ++k) m = fmaxf(m, pp_lane(bc, k) + tab[k * stride]);
  float s = 0.0f;
  for (int k = 0; k < S; ++k) s += pp_exp2((pp_lane(bc, k) + tab[k * stride]) - m);
  return pp_m_plus_log2(m, s);
}

// the LDS of the one-wave kernels
struct PpLds {
  float* t;              // [S][S | 1]: the table
  float* a;              // [PC_TILE][S]: a_f, then the posterior
  float* e;              // [PC_TILE][S]
  int* sc;               // [S]
};
__device__ __forceinline__ PpLds pp_carve(float* lds, int S) {
  PpLds l;
  l.t = lds;
  l.a = l.t + S * (S | 1);
  l.e = l.a + PC_TILE * S;
  l.sc = reinterpret_cast<int*>(l.e + PC_TILE * S);
  return l;
}
inline size_t pp_wave_lds_bytes(int S) { return 4 * ((size_t)S * (S | 1) + 2 * PC_TILE * S + S); }

__device__ __forceinline__ void pp_stage_table(const PcChain& a, const PpLds& l) {
  const int S = a.S, SP = S | 1;
  for (int idx = threadIdx.x; idx < S * S; idx += blockDim.x) {
    const int i = (int)fdiv((unsigned)idx, a.div_s);
    l.t[i * SP + (idx - i * S)] = pp_trans(a.trans[idx]);
  }
  for (int idx = threadIdx.x; idx < S; idx += blockDim.x) l.sc[idx] = a.state_class[idx];
}

// Forward over the n staged frames, lane = state (one wave; lanes >= S compute on state S - 1 and store nothing).  av: the
// lane's a in front of the first frame on entry, a of the last frame on exit.  Leaves the a_f rows in LDS, writes `filtered`
// ([batch][T][S]) when there is one, adds every c_f to both sums.
template <bool SMALL>
__device__ __forceinline__ void pp_forward(const PcChain& a, float* filtered, const PpLds& l, const float (&col)[16], int b,
                                           int f0, int n, int lane, float& av, double& total, double& call) {
  const int S = a.S, jj = min(lane, S - 1);
  float* __restrict__ filt = filtered ? filtered + ((long long)b * a.T + f0) * S : nullptr;
  float e = l.e[jj];
  for (int f = 0; f < n; ++f) {
    const float e_next = f + 1 < n ? l.e[(f + 1) * S + jj] : 0.0f;
    const float A = e + pp_step<SMALL>(av, col, l.t + jj, S | 1, S);
    float m, lg;
    double c;
    pp_L_states<SMALL>(A, S, lane < S, m, lg, c);
    av = (A - m) - lg;
    total += c;
    call += c;
    if (lane < S) {
      l.a[f * S + lane] = av;
      if (filt) filt[f * S + lane] = pp_exp2(av);
    }
    e = e_next;
  }
}

// b of a frame from g[j] = E[f + 1][j] + b_(f + 1)[j], its maximum taken out
template <bool SMALL>
__device__ __forceinline__ float pp_b_from_g(const PpLds& l, const float (&row)[16], float g, int S, int jj) {
  const float B = pp_step<SMALL>(g, row, l.t + jj * (S | 1), 1, S);
  return B - pp_max_states<SMALL>(B, S);
}

// Backward over the n staged frames whose a_f rows are in LDS.  bv: the lane's b at the tile's last frame on entry.  call_end:
// that frame is the call's last, where b is 0 and the posterior is the filtered row itself, bit for bit.  Overwrites the rows
// with the posterior, stores it, and returns g of the tile's first frame for the tile in front.
template <bool SMALL>
__device__ __forceinline__ float pp_backward(const PpArgs& a, const PpLds& l, const float (&row)[16], int b, int f0, int n, int lane,
                                             float bv, bool call_end) {
  const int S = a.S, jj = min(lane, S - 1);
  float* __restrict__ out = a.posterior + ((long long)b * a.T + f0) * S;
  float g = 0.0f;
  for (int f = n - 1; f >= 0; --f) {
    if (f < n - 1) bv = pp_b_from_g<SMALL>(l, row, g, S, jj);
    const float av = l.a[f * S + jj];
    float post;
    if (call_end && f == n - 1) {
      post = pp_exp2(av);
    } else {
      const float u = av + bv;
      float m, lg;
      pp_L_states<SMALL>(u, S, lane < S, m, lg);
      post = pp_exp2((u - m) - lg);
    }
    if (lane < S) {
      l.a[f * S + lane] = post;
      out[f * S + lane] = post;
    }
    g = l.e[f * S + jj] + bv;
  }
  return g;
}

// class_posterior of the n frames whose posterior rows are in LDS: thread = (frame, class), ascending j
__device__ __forceinline__ void pp_classes(const PpArgs& a, const PpLds& l, int b, int f0, int n) {
  if (!a.class_posterior) return;
  const int S = a.S, C = a.C;
  float* __restrict__ out = a.class_posterior + ((long long)b * a.T + f0) * C;
  for (int idx = threadIdx.x; idx < n * C; idx += blockDim.x) {
    const int f = (int)fdiv((unsigned)idx, a.div_c), c = idx - f * C;
    float s = 0.0f;
    for (int j = 0; j < S; ++j)
      if (l.sc[j] == c) s += l.a[f * S + j];
    out[idx] = s;
  }
}

// a stream's start vector for lane jj: init before its first frame, the carry after it
__device__ __forceinline__ float pp_stream_start(const PcChain& a, const double* carry, int b, int jj) {
  const double* __restrict__ c = carry + (long long)b * (a.S + 2);
  if (c[0] == 0.0) return a.init ? pp_trans(a.init[jj]) : 0.0f;
  return (float)c[2 + jj];
}
// the same of a whole video (qt_pose_prior_expect: no carry)
__device__ __forceinline__ float pp_video_start(const PcChain& a, int jj) { return a.init ? pp_trans(a.init[jj]) : 0.0f; }
// after a stream's last frame: av = a_last; sum = the c_f of this call
__device__ __forceinline__ void pp_write_carry(const PpArgs& a, int b, int lane, float av, double seen, double total, double call) {
  double* __restrict__ c = a.carry + (long long)b * (a.S + 2);
  if (lane < a.S) c[2 + lane] = (double)av;
  if (lane == 0) {
    c[0] = seen + (double)a.T;
    c[1] = total;
    if (a.evidence) a.evidence[b] = call;
  }
}

// ---- the short route, and (QTCNN_POSE_POSTERIOR=1) the same algorithm over all tiles of a stream -----------------------------
template <bool SMALL>
__global__ __launch_bounds__(QT_WAVE) void pp_stream_kernel(PpArgs a) {
  extern __shared__ __attribute__((aligned(16))) float pp_lds[];
  const PpLds l = pp_carve(pp_lds, a.S);
  const int lane = threadIdx.x, b = blockIdx.x, S = a.S, SP = S | 1, jj = min(lane, S - 1);
  pp_stage_table(a, l);
  const double seen = a.carry[(long long)b * (S + 2)];
  double total = a.carry[(long long)b * (S + 2) + 1], call = 0.0;
  float av = pp_stream_start(a, a.carry, b, jj);
  __syncthreads();
  float col[16], row[16];
  if (SMALL) {
    pp_load16(col, l.t + jj, SP, S);
    pp_load16(row, l.t + jj * SP, 1, S);
  }
  for (int tile = 0; tile < a.tiles; ++tile) {
    const int f0 = tile * PC_TILE, n = min(PC_TILE, a.T - f0);
    __syncthreads();
    pc_stage_emissions(a, b, f0, n, l.e);
    __syncthreads();
    pp_forward<SMALL>(a, a.filtered, l, col, b, f0, n, lane, av, total, call);
    if (a.tiles > 1) {   // the a_f rows wait in the posterior output for the backward sweep
      __syncthreads();
      float* __restrict__ out = a.posterior + ((long long)b * a.T + f0) * S;
      for (int idx = lane; idx < n * S; idx += QT_WAVE) out[idx] = l.a[idx];
    }
  }
  pp_write_carry(a, b, lane, av, seen, total, call);
  float g = 0.0f;
  for (int tile = a.tiles - 1; tile >= 0; --tile) {
    const int f0 = tile * PC_TILE, n = min(PC_TILE, a.T - f0);
    const bool last = tile == a.tiles - 1;
    if (a.tiles > 1) {
      __syncthreads();
      pc_stage_emissions(a, b, f0, n, l.e);
      const float* in = a.posterior + ((long long)b * a.T + f0) * S;
      for (int idx = lane; idx < n * S; idx += QT_WAVE) l.a[idx] = in[idx];
    }
    __syncthreads();
    const float bv = last ? 0.0f : pp_b_from_g<SMALL>(l, row, g, S, jj);
    g = pp_backward<SMALL>(a, l, row, b, f0, n, lane, bv, last);
    __syncthreads();
    pp_classes(a, l, b, f0, n);
  }
}

// ---- (a) tile products ---------------------------------------------------------------------------------------------------------
// One entry of the next product: row `pr` of the current one (unnormalised: its maximum r is found here and taken out), column
// `tc` of the table (stride S).  SMALL: S <= 16, the row in registers.
template <bool SMALL>
__device__ __forceinline__ float pp_product_entry(const float* __restrict__ pr, const float* __restrict__ tc, int S, float& r) {
  if (SMALL) {
    float q[16], x[16], t[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) t[k] = q[k] = pr[k < S ? k : 0];
    r = pp_max16(t);
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const float v = (q[k] - r) + tc[(k < S ? k : 0) * S];
      t[k] = x[k] = k < S ? v : PP_PAD;
    }
    const float m = pp_max16(t);
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < 16; ++k) s += pp_exp2(x[k] - m);
    return pp_m_plus_log2(m, s);
  }
  r = pr[0];
  for (int k = 1; k < S; ++k) r = fmaxf(r, pr[k]);
  float m = (pr[0] - r) + tc[0];
  for (int k = 1; k < S; ++k) m = fmaxf(m, (pr[k] - r) + tc[k * S]);
  float s = 0.0f;
  for (int k = 0; k < S; ++k) s += pp_exp2(((pr[k] - r) + tc[k * S]) - m);
  return pp_m_plus_log2(m, s);
}

template <bool SMALL>
__global__ __launch_bounds__(PP_PROD_THREADS) void pp_products_kernel(PpTiles a) {
  extern __shared__ __attribute__((aligned(16))) float pp_lds[];
  const int S = a.S, SS = S * S, tid = threadIdx.x;
  double* off = reinterpret_cast<double*>(pp_lds);   // [S] (64 doubles reserved)
  float* tr = pp_lds + 2 * PC_MAX_S;
  float* cur = tr + SS;
  float* nxt = cur + SS;
  short* e_l = reinterpret_cast<short*>(nxt + SS);   // q: three products of 64 x 64 leave no room for 16 KB of scores
  const int b = blockIdx.x / a.tiles, tile = blockIdx.x - b * a.tiles;
  const int f0 = tile * PC_TILE, n = min(PC_TILE, a.T - f0);
  for (int idx = tid; idx < SS; idx += PP_PROD_THREADS) tr[idx] = pp_trans(a.trans[idx]);
  for (int idx = tid; idx < S; idx += PP_PROD_THREADS) off[idx] = 0.0;
  pc_stage_emissions(a, b, f0, n, e_l);
  __syncthreads();
  for (int idx = tid; idx < SS; idx += PP_PROD_THREADS) {
    const int i = (int)fdiv((unsigned)idx, a.div_s);
    cur[idx] = tr[idx] + pc_score(e_l[idx - i * S]);
  }
  __syncthreads();
  for (int f = 1; f < n; ++f) {
    for (int idx = tid; idx < SS; idx += PP_PROD_THREADS) {
      const int i = (int)fdiv((unsigned)idx, a.div_s), j = idx - i * S;
      float r;
      const float v = pp_product_entry<SMALL>(cur + i * S, tr + j, S, r);
      nxt[idx] = pc_score(e_l[f * S + j]) + v;
      if (j == 0) off[i] += (double)r;   // (row i's own thread: nobody else touches off[i])
    }
    __syncthreads();
    float* t = cur;
    cur = nxt;
    nxt = t;
  }
  float* __restrict__ out = a.products + ((long long)b * a.tiles + tile) * SS;
  double* __restrict__ out_off = a.offsets + ((long long)b * a.tiles + tile) * S;
  for (int idx = tid; idx < SS; idx += PP_PROD_THREADS) {
    const int i = (int)fdiv((unsigned)idx, a.div_s), j = idx - i * S;
    const float* __restrict__ pr = cur + i * S;
    float r = pr[0];
    for (int k = 1; k < S; ++k) r = fmaxf(r, pr[k]);
    out[idx] = cur[idx] - r;
    if (j == 0) out_off[i] = off[i] + (double)r;
  }
}

// ---- (b) the start vector forward and the end vector backward through the products ------------------------------------------
__host__ __device__ inline int pp_scan_trip_tiles(int S) {
  const int k = PP_SCAN_FLOATS / (S * S);
  return k > PP_SCAN_MAX_TILES ? PP_SCAN_MAX_TILES : k;
}

// CARRY: the stream's start is pp_stream_start's; without it (the learner, every call a whole video) init / 256 or 0
template <bool SMALL, bool CARRY = true>
__global__ __launch_bounds__(PP_SCAN_THREADS) void pp_scan_kernel(const double* carry, PpTiles a) {
  __shared__ __attribute__((aligned(16))) double offs[2][PP_SCAN_PAD];
  __shared__ __attribute__((aligned(16))) float buf[2][PP_SCAN_FLOATS + PP_SCAN_PAD];
  constexpr int PER = PP_SCAN_FLOATS / PP_SCAN_THREADS, PER_OFF = PP_SCAN_PAD / PP_SCAN_THREADS;
  const int S = a.S, SS = S * S, SP = S | 1, tid = threadIdx.x, lane = tid & (QT_WAVE - 1);
  const bool chain = tid < QT_WAVE;   // wave 0
  const int K = pp_scan_trip_tiles(S), jj = min(lane, S - 1), b = blockIdx.x, tiles = a.tiles;
  const float* __restrict__ prod = a.products + (long long)b * tiles * SS;
  const double* __restrict__ poff = a.offsets + (long long)b * tiles * S;
  float* __restrict__ starts = a.starts + (long long)b * tiles * S;
  float* __restrict__ ends = a.ends + (long long)b * tiles * S;
  double* __restrict__ before = a.before + (long long)b * tiles;
  float r[PER];
  double ro[PER_OFF];
  auto fetch = [&](int t0, int kt) {   // products t0 .. t0 + kt - 1 and their offsets into registers
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int idx = tid + u * PP_SCAN_THREADS;
      r[u] = idx < kt * SS ? prod[(long long)t0 * SS + idx] : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < PER_OFF; ++u) {
      const int idx = tid + u * PP_SCAN_THREADS;
      ro[u] = idx < kt * S ? poff[(long long)t0 * S + idx] : 0.0;
    }
  };
  auto put = [&](int which, int kt) {   // rows padded to S | 1
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int idx = tid + u * PP_SCAN_THREADS;
      if (idx < kt * SS) {
        const int row = (int)fdiv((unsigned)idx, a.div_s);
        buf[which][row * SP + (idx - row * S)] = r[u];
      }
    }
#pragma unroll
    for (int u = 0; u < PER_OFF; ++u) {
      const int idx = tid + u * PP_SCAN_THREADS;
      if (idx < kt * S) offs[which][idx] = ro[u];
    }
  };
  float reg[16];

  // forward: the products of tiles 0 .. tiles - 2 give the starts of tiles 1 .. tiles - 1
  const int count = tiles - 1;
  float v = 0.0f;
  double ev = 0.0;
  if (chain) {
    v = CARRY ? pp_stream_start(a, carry, b, jj) : pp_video_start(a, jj);
    if (lane < S) starts[lane] = v;
    if (lane == 0) before[0] = 0.0;
  }
  fetch(0, min(K, count));
  put(0, min(K, count));
  __syncthreads();
  int which = 0;
  for (int t0 = 0; t0 < count; t0 += K) {
    const int kt = min(K, count - t0), kn = min(K, count - (t0 + K));
    if (kn > 0) fetch(t0 + K, kn);
    if (chain) {
      for (int u = 0; u < kt; ++u) {
        const float* __restrict__ P = buf[which] + u * S * SP;
        const double w = (double)v + offs[which][u * S + jj];
        const double W = pp_max_states<SMALL>(w, S);
        const float wf = (float)(w - W);
        if (SMALL) pp_load16(reg, P + jj, SP, S);
        const float A = pp_step<SMALL>(wf, reg, P + jj, SP, S);
        float m, lg;
        double c;
        pp_L_states<SMALL>(A, S, lane < S, m, lg, c);
        v = (A - m) - lg;
        ev += W + c;
        if (lane < S) starts[(long long)(t0 + u + 1) * S + lane] = v;
        if (lane == 0) before[t0 + u + 1] = ev;
      }
    }
    if (kn > 0) put(which ^ 1, kn);
    __syncthreads();
    which ^= 1;
  }

  // backward: the products of tiles tiles - 1 .. 1 give the ends of tiles tiles - 2 .. 0
  float bv = 0.0f;
  if (chain && lane < S) ends[(long long)(tiles - 1) * S + lane] = 0.0f;
  {
    const int lo = max(tiles - K, 1);
    fetch(lo, tiles - lo);
    put(which, tiles - lo);
  }
  __syncthreads();
  for (int hi = tiles - 1; hi >= 1; hi -= K) {   // this trip: tiles lo .. hi
    const int lo = max(hi - K + 1, 1), nhi = lo - 1, nlo = max(nhi - K + 1, 1);
    if (nhi >= 1) fetch(nlo, nhi - nlo + 1);
    if (chain) {
      for (int t = hi; t >= lo; --t) {
        const float* __restrict__ P = buf[which] + (t - lo) * S * SP;
        if (SMALL) pp_load16(reg, P + jj * SP, 1, S);
        const float B = pp_step<SMALL>(bv, reg, P + jj * SP, 1, S);
        const double Bd = offs[which][(t - lo) * S + jj] + (double)B;
        bv = (float)(Bd - pp_max_states<SMALL>(Bd, S));
        if (lane < S) ends[(long long)(t - 1) * S + lane] = bv;
      }
    }
    if (nhi >= 1) put(which ^ 1, nhi - nlo + 1);
    __syncthreads();
    which ^= 1;
  }
}

// ---- (c) replay ----------------------------------------------------------------------------------------------------------------
template <bool SMALL>
__global__ __launch_bounds__(QT_WAVE) void pp_replay_kernel(PpArgs a) {
  extern __shared__ __attribute__((aligned(16))) float pp_lds[];
  const PpLds l = pp_carve(pp_lds, a.S);
  const int lane = threadIdx.x, S = a.S, SP = S | 1, jj = min(lane, S - 1);
  const int b = blockIdx.x / a.tiles, tile = blockIdx.x - b * a.tiles;
  const int f0 = tile * PC_TILE, n = min(PC_TILE, a.T - f0);
  const bool last = tile == a.tiles - 1;
  pp_stage_table(a, l);
  pc_stage_emissions(a, b, f0, n, l.e);
  float av = a.starts[((long long)b * a.tiles + tile) * S + jj];
  const float bv = a.ends[((long long)b * a.tiles + tile) * S + jj];
  __syncthreads();
  float col[16], row[16];
  if (SMALL) {
    pp_load16(col, l.t + jj, SP, S);
    pp_load16(row, l.t + jj * SP, 1, S);
  }
  double call = a.before[(long long)b * a.tiles + tile], unused = 0.0;
  pp_forward<SMALL>(a, a.filtered, l, col, b, f0, n, lane, av, unused, call);
  if (last) {
    const double seen = a.carry[(long long)b * (S + 2)], total = a.carry[(long long)b * (S + 2) + 1];
    pp_write_carry(a, b, lane, av, seen, total + call, call);
  }
  __syncthreads();
  pp_backward<SMALL>(a, l, row, b, f0, n, lane, bv, last);
  __syncthreads();
  pp_classes(a, l, b, f0, n);
}

// ---- the learner's E-step (qt_pose_prior_expect): the pairwise posteriors xi summed over the frames -------------------------
// A wave per (stream, tile), lane = state i: the replay's forward step (the a_f rows in LDS, nothing stored), then the backward
// sweep with one more L over the states per frame: the un-normalised B_f[i] = L_j (T[i][j] + g_f[j]) that gives b_(f-1) also
// gives Z_f = L_i (a_(f-1)[i] + B_f[i]), and the lane adds 2^(((a_(f-1)[i] - Z_f) + T[i][j]) + g_f[j]) into row i of the tile's
// f32 partial: sixteen registers for S <= 16, its own LDS row (stride S | 1) above.  The emissions stay the integers q in LDS
// (8 KB at S = 64), so the partial fits beside the table and the a_f rows: 57,856 bytes at S = 64.  A video's frame 0 goes into
// the start partial (the sum over j in ascending j), every other frame into the partial; the tile's `starts` vector is the
// a_(f0 - 1) of its first frame.  pr_reduce then adds tiles and streams in ascending order, in double, one thread per entry.
struct PrArgs : PpTiles {
  double* evidence;          // workspace: double [batch]
  float* partial;            //            f32 [batch][tiles][S][S]
  float* start_partial;      //            f32 [batch][S]
  double* counts;
  double* start_counts;
  double* totals;
};
inline size_t pr_wave_lds_bytes(int S) {
  return 4 * ((size_t)S * (S | 1) * (S <= 16 ? 1 : 2) + PC_TILE * S) + 2 * PC_TILE * S;
}

template <bool SMALL>
__global__ __launch_bounds__(QT_WAVE) void pr_expect_kernel(PrArgs r) {
  extern __shared__ __attribute__((aligned(16))) float pp_lds[];
  const PrArgs& a = r;
  const int lane = threadIdx.x, S = a.S, SP = S | 1, jj = min(lane, S - 1);
  float* t_l = pp_lds;                                  // [S][S | 1]
  float* a_l = t_l + S * SP;                            // [PC_TILE][S]
  float* acc_l = a_l + PC_TILE * S;                     // [S][S | 1], S > 16 only
  short* e_l = reinterpret_cast<short*>(acc_l + (SMALL ? 0 : S * SP));   // [PC_TILE][S]
  const int b = blockIdx.x / a.tiles, tile = blockIdx.x - b * a.tiles;
  const int f0 = tile * PC_TILE, n = min(PC_TILE, a.T - f0);
  const bool last = tile == a.tiles - 1;
  const long long slot = (long long)b * a.tiles + tile;
  for (int idx = lane; idx < S * S; idx += QT_WAVE) {
    const int i = (int)fdiv((unsigned)idx, a.div_s);
    t_l[i * SP + (idx - i * S)] = pp_trans(a.trans[idx]);
    if (!SMALL) acc_l[i * SP + (idx - i * S)] = 0.0f;
  }
  pc_stage_emissions(a, b, f0, n, e_l);
  const float a0 = tile == 0 ? pp_video_start(a, jj) : a.starts[slot * S + jj];   // (the short route runs no scan)
  float bv = last ? 0.0f : a.ends[slot * S + jj];
  double call = tile == 0 ? 0.0 : a.before[slot];
  __syncthreads();
  float col[16], row[16];
  if (SMALL) {
    pp_load16(col, t_l + jj, SP, S);
    pp_load16(row, t_l + jj * SP, 1, S);
  }
  float av = a0;
  for (int f = 0; f < n; ++f) {   // pp_forward's frames, the emissions from their integers
    const float A = pc_score(e_l[f * S + jj]) + pp_step<SMALL>(av, col, t_l + jj, SP, S);
    float m, lg;
    double c;
    pp_L_states<SMALL>(A, S, lane < S, m, lg, c);
    av = (A - m) - lg;
    call += c;
    if (lane < S) a_l[f * S + lane] = av;
  }
  if (last && lane == 0) a.evidence[b] = call;
  __syncthreads();
  float acc[16], sp = 0.0f;
#pragma unroll
  for (int k = 0; k < 16; ++k) acc[k] = 0.0f;
  for (int f = n - 1; f >= 0; --f) {
    const float g = pc_score(e_l[f * S + jj]) + bv;
    const float B = pp_step<SMALL>(g, row, t_l + jj * SP, 1, S);
    const float ap = f > 0 ? a_l[(f - 1) * S + jj] : a0;
    float m, lg;
    pp_L_states<SMALL>(ap + B, S, lane < S, m, lg);
    const float w = (ap - m) - lg;                      // a_(f-1)[i] - Z_f
    const bool first = f == 0 && tile == 0;             // the virtual transition out of the start vector
    if (SMALL) {
#pragma unroll
      for (int k = 0; k < 16; ++k) {                    // (row pads the slots beyond S out: 2^-1e30 is 0)
        const float x = pp_exp2((w + row[k]) + pp_lane(g, k));
        if (first) sp += x;
        else acc[k] += x;
      }
    } else {
      for (int k = 0; k < S; ++k) {
        const float x = pp_exp2((w + t_l[jj * SP + k]) + pp_lane(g, k));
        if (first) sp += x;
        else if (lane < S) acc_l[lane * SP + k] += x;
      }
    }
    bv = B - pp_max_states<SMALL>(B, S);
  }
  float* __restrict__ out = r.partial + slot * S * S;
  if (SMALL) {
    if (lane < S) {
#pragma unroll
      for (int k = 0; k < 16; ++k)
        if (k < S) out[lane * S + k] = acc[k];
    }
  } else {
    __syncthreads();
    for (int idx = lane; idx < S * S; idx += QT_WAVE) {
      const int i = (int)fdiv((unsigned)idx, a.div_s);
      out[idx] = acc_l[i * SP + (idx - i * S)];
    }
  }
  if (tile == 0 && lane < S) r.start_partial[(long long)b * S + lane] = sp;
}

// thread = one entry of counts, start_counts or totals: a stream's tiles in ascending order, then the streams in ascending
// order, all in double, then one addition onto the caller's accumulator
constexpr int PR_REDUCE_THREADS = 256;
constexpr int PR_REDUCE_AHEAD = 16;
__global__ __launch_bounds__(PR_REDUCE_THREADS) void pr_reduce_kernel(PrArgs r, int batch) {
  const PrArgs& a = r;
  const int S = a.S, SS = S * S, idx = blockIdx.x * PR_REDUCE_THREADS + threadIdx.x;
  if (idx < SS) {
    // the (stream, tile) slots are one run in memory: PR_REDUCE_AHEAD loads in flight, then their additions in the fixed order
    const float* __restrict__ p = r.partial + idx;
    const long long slots = (long long)batch * a.tiles;
    double s = 0.0, sb = 0.0;
    int tile = 0;
    auto add = [&](float v) {
      sb += (double)v;
      if (++tile == a.tiles) {   // the stream's last tile
        s += sb;
        sb = 0.0;
        tile = 0;
      }
    };
    long long k = 0;
    for (; k + PR_REDUCE_AHEAD <= slots; k += PR_REDUCE_AHEAD) {
      float v[PR_REDUCE_AHEAD];
#pragma unroll
      for (int u = 0; u < PR_REDUCE_AHEAD; ++u) v[u] = p[(k + u) * SS];
#pragma unroll
      for (int u = 0; u < PR_REDUCE_AHEAD; ++u) add(v[u]);
    }
    for (; k < slots; ++k) add(p[k * SS]);
    r.counts[idx] += s;
  } else if (idx < SS + S) {
    double s = 0.0;
    for (int b = 0; b < batch; ++b) s += (double)r.start_partial[(long long)b * S + (idx - SS)];
    r.start_counts[idx - SS] += s;
  } else if (idx == SS + S) {
    double s = 0.0;
    for (int b = 0; b < batch; ++b) s += a.evidence[b];
    r.totals[0] += s;
  } else if (idx == SS + S + 1) {
    r.totals[1] += (double)batch * (double)a.T;
  }
}

// the workspace of the tiled route, the doubles first
struct PpLayout {
  long long offsets, before, products, starts, ends, total;
};
PpLayout pp_layout(const qt_pose_order_desc* d) {
  PpLayout w = {0, 0, 0, 0, 0, 0};
  if (d->frames <= PC_TILE) return w;
  const long long B = d->batch, S = d->num_states, tiles = qt_cdiv(d->frames, PC_TILE);
  w.offsets = 0;
  w.before = w.offsets + B * tiles * S * 8;
  w.products = w.before + B * tiles * 8;
  w.starts = w.products + B * tiles * S * S * 4;
  w.ends = w.starts + B * tiles * S * 4;
  w.total = w.ends + B * tiles * S * 4;
  return w;
}
void pp_fill_tiles(PpTiles& a, void* workspace, const PpLayout& w) {
  char* ws = static_cast<char*>(workspace);
  a.offsets = reinterpret_cast<double*>(ws + w.offsets);
  a.before = reinterpret_cast<double*>(ws + w.before);
  a.products = reinterpret_cast<float*>(ws + w.products);
  a.starts = reinterpret_cast<float*>(ws + w.starts);
  a.ends = reinterpret_cast<float*>(ws + w.ends);
}
inline size_t pp_prod_lds_bytes(int S) { return 4 * (2 * PC_MAX_S + 3 * (size_t)S * S) + 2 * PC_TILE * S; }

// the learner's workspace: the tiled route's (none up to PC_TILE frames), then the evidence, the partials, the start partials
struct PrLayout {
  PpLayout pp;
  long long evidence, partial, start_partial, total;
};
PrLayout pr_layout(const qt_pose_order_desc* d) {
  PrLayout w;
  w.pp = pp_layout(d);
  const long long B = d->batch, S = d->num_states, tiles = qt_cdiv(d->frames, PC_TILE);
  w.evidence = (w.pp.total + 7) / 8 * 8;
  w.partial = w.evidence + B * 8;
  w.start_partial = w.partial + B * tiles * S * S * 4;
  w.total = (w.start_partial + B * S * 4 + 7) / 8 * 8;
  return w;
}

}  // namespace

extern "C" long long qt_pose_prior_workspace_bytes(const qt_pose_order_desc* desc) {
  if (pc_check_desc("qt_pose_prior_workspace_bytes", desc) != QT_OK) return 0;
  return pr_layout(desc).total;
}

extern "C" int qt_pose_prior_expect(const qt_pose_order_desc* desc, const float* probs, long long ld, const int* state_class,
                                    const int* trans, const int* init, double* counts, double* start_counts, double* totals,
                                    void* workspace, long long workspace_bytes, void* stream) {
  const char* const who = "qt_pose_prior_expect";
  if (const int rc = pc_check_desc(who, desc)) return rc;
  const int B = desc->batch, T = desc->frames, C = desc->num_classes, S = desc->num_states;
  QT_CHECK_ARG(ld >= C, "%s: row stride ld = %lld < C = %d", who, ld, C);
  QT_CHECK_ARG(probs != nullptr && state_class != nullptr && trans != nullptr && counts != nullptr && start_counts != nullptr &&
                   totals != nullptr,
               "%s: null %s", who,
               !probs ? "probs" : !state_class ? "state_class" : !trans ? "trans" : !counts ? "counts" : !start_counts ? "start_counts"
                                                                                                                        : "totals");
  QT_CHECK_ARG(!misaligned(probs, 3) && !misaligned(state_class, 3) && !misaligned(trans, 3) && !misaligned(init, 3) &&
                   !misaligned(counts, 7) && !misaligned(start_counts, 7) && !misaligned(totals, 7) && !misaligned(workspace, 7),
               "%s: probs, state_class, trans and init must be 4-byte aligned, counts, start_counts, totals and the workspace "
               "8-byte", who);
  const PrLayout w = pr_layout(desc);
  QT_CHECK_ARG(workspace != nullptr && workspace_bytes >= w.total,
               "%s: workspace of %lld bytes; qt_pose_prior_workspace_bytes asks for %lld", who, workspace ? workspace_bytes : 0LL,
               w.total);
  const long long rows = (long long)B * T;
  const PcBuf in[] = {{probs, (size_t)((rows - 1) * ld + C) * 4, "probs"}, {state_class, (size_t)S * 4, "state_class"},
                      {trans, (size_t)S * S * 4, "trans"}, {init, (size_t)S * 4, "init"}};
  const PcBuf out[] = {{counts, (size_t)S * S * 8, "counts"}, {start_counts, (size_t)S * 8, "start_counts"},
                       {totals, 16, "totals"}, {workspace, (size_t)w.total, "workspace"}};
  if (const int rc = pc_check_disjoint(who, in, out)) return rc;

  PrArgs r;
  pc_fill(r, probs, ld, state_class, trans, init, T, C, S);
  pp_fill_tiles(r, workspace, w.pp);
  char* ws = static_cast<char*>(workspace);
  r.evidence = reinterpret_cast<double*>(ws + w.evidence);
  r.partial = reinterpret_cast<float*>(ws + w.partial);
  r.start_partial = reinterpret_cast<float*>(ws + w.start_partial);
  r.counts = counts;
  r.start_counts = start_counts;
  r.totals = totals;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 all((unsigned)((long long)B * r.tiles)), streams((unsigned)B);
  const dim3 wave(QT_WAVE), prod(PP_PROD_THREADS), scan(PP_SCAN_THREADS);
  const PpTiles& tiles = r;
  if (r.tiles > 1) {
    const size_t prod_lds = pp_prod_lds_bytes(S);
    pc_by_small(S, [&](auto sm) { hipLaunchKernelGGL(pp_products_kernel<PC_SMALL(sm)>, all, prod, prod_lds, s, tiles); });
    QT_CHECK_LAUNCH();
    pc_by_small(S, [&](auto sm) {
      hipLaunchKernelGGL((pp_scan_kernel<PC_SMALL(sm), false>), streams, scan, 0, s, (const double*)nullptr, tiles);
    });
    QT_CHECK_LAUNCH();
  }
  pc_by_small(S, [&](auto sm) { hipLaunchKernelGGL(pr_expect_kernel<PC_SMALL(sm)>, all, wave, pr_wave_lds_bytes(S), s, r); });
  QT_CHECK_LAUNCH();
  hipLaunchKernelGGL(pr_reduce_kernel, dim3((unsigned)qt_cdiv(S * S + S + 2, PR_REDUCE_THREADS)), dim3(PR_REDUCE_THREADS), 0, s, r,
                     B);
  QT_CHECK_LAUNCH();
  return QT_OK;
}

extern "C" long long qt_pose_posterior_workspace_bytes(const qt_pose_order_desc* desc) {
  if (pc_check_desc("qt_pose_posterior_workspace_bytes", desc) != QT_OK) return 0;
  return pp_layout(desc).total;
}

extern "C" int qt_pose_posterior(const qt_pose_order_desc* desc, const float* probs, long long ld, const int* state_class,
                                 const int* trans, const int* init, double* carry, float* posterior, float* filtered,
                                 float* class_posterior, double* log2_evidence, void* workspace, long long workspace_bytes,
                                 void* stream) {
  const char* const who = "qt_pose_posterior";
  if (const int rc = pc_check_desc(who, desc)) return rc;
  const int B = desc->batch, T = desc->frames, C = desc->num_classes, S = desc->num_states;
  QT_CHECK_ARG(ld >= C, "%s: row stride ld = %lld < C = %d", who, ld, C);
  QT_CHECK_ARG(probs != nullptr && state_class != nullptr && trans != nullptr && carry != nullptr && posterior != nullptr,
               "%s: null %s", who,
               !probs ? "probs" : !state_class ? "state_class" : !trans ? "trans" : !carry ? "carry" : "posterior");
  QT_CHECK_ARG(!misaligned(probs, 3) && !misaligned(state_class, 3) && !misaligned(trans, 3) && !misaligned(init, 3) &&
                   !misaligned(posterior, 3) && !misaligned(filtered, 3) && !misaligned(class_posterior, 3) &&
                   !misaligned(carry, 7) && !misaligned(log2_evidence, 7) && !misaligned(workspace, 7),
               "%s: probs, state_class, trans, init, posterior, filtered and class_posterior must be 4-byte aligned, carry, "
               "log2_evidence and the workspace 8-byte", who);
  const PpLayout w = pp_layout(desc);
  QT_CHECK_ARG(w.total == 0 || (workspace != nullptr && workspace_bytes >= w.total),
               "%s: workspace of %lld bytes; qt_pose_posterior_workspace_bytes asks for %lld", who,
               workspace ? workspace_bytes : 0LL, w.total);
  const long long rows = (long long)B * T;
  const PcBuf in[] = {{probs, (size_t)((rows - 1) * ld + C) * 4, "probs"}, {state_class, (size_t)S * 4, "state_class"},
                      {trans, (size_t)S * S * 4, "trans"}, {init, (size_t)S * 4, "init"}};
  const PcBuf out[] = {{carry, (size_t)B * (S + 2) * 8, "carry"}, {posterior, (size_t)rows * S * 4, "posterior"},
                       {filtered, (size_t)rows * S * 4, "filtered"}, {class_posterior, (size_t)rows * C * 4, "class_posterior"},
                       {log2_evidence, (size_t)B * 8, "log2_evidence"}, {workspace, (size_t)w.total, "workspace"}};
  if (const int rc = pc_check_disjoint(who, in, out)) return rc;

  PpArgs a;
  pc_fill(a, probs, ld, state_class, trans, init, T, C, S);
  pp_fill_tiles(a, workspace, w);
  a.carry = carry;
  a.posterior = posterior;
  a.filtered = filtered;
  a.class_posterior = class_posterior;
  a.evidence = log2_evidence;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t wave_lds = pp_wave_lds_bytes(S);
  const dim3 all((unsigned)((long long)B * a.tiles)), streams((unsigned)B);
  const dim3 wave(QT_WAVE), prod(PP_PROD_THREADS), scan(PP_SCAN_THREADS);
  const bool one_wave = a.tiles > 1 && qt_env_int("QTCNN_POSE_POSTERIOR", 0) == 1;   // per call: see the head of the file
  if (a.tiles == 1 || one_wave) {
    pc_by_small(S, [&](auto sm) { hipLaunchKernelGGL(pp_stream_kernel<PC_SMALL(sm)>, streams, wave, wave_lds, s, a); });
    QT_CHECK_LAUNCH();
    return QT_OK;
  }
  const PpTiles& tiles = a;
  const size_t prod_lds = pp_prod_lds_bytes(S);
  pc_by_small(S, [&](auto sm) { hipLaunchKernelGGL(pp_products_kernel<PC_SMALL(sm)>, all, prod, prod_lds, s, tiles); });
  QT_CHECK_LAUNCH();
  pc_by_small(S, [&](auto sm) {
    hipLaunchKernelGGL((pp_scan_kernel<PC_SMALL(sm), true>), streams, scan, 0, s, (const double*)a.carry, tiles);
  });
  QT_CHECK_LAUNCH();
  pc_by_small(S, [&](auto sm) { hipLaunchKernelGGL(pp_replay_kernel<PC_SMALL(sm)>, all, wave, wave_lds, s, a); });
  QT_CHECK_LAUNCH();
  return QT_OK;
}

// ---- fixed-lag posteriors across calls (qt_pose_lag_smooth) -------------------------------------------------------------------
// lagged[g] is the posterior of frame g given the frames up to w = min(g + lag, the call's last frame): the forward pass is the
// frame-by-frame rule above (pp_forward as it is), and every emitted frame sweeps backward over its own window of at most lag
// steps with pp_backward's arithmetic (pp_b_from_g, pp_L_states), so a window's bits depend neither on the call boundaries nor on
// the route.  Frames carry global indices; the LDS rings hold frame g in row g & 127 (lag + PC_TILE <= 127 rows are alive at a
// time), and the forward pass goes in chunks that end on multiples of PC_TILE so that a chunk's rows are one run.
// Live route: pl_stream_kernel<LIVE>, one launch, one wave per stream: table, history (from carry_in) and new emissions in LDS,
// forward over a chunk, then that chunk's windows one after another, then carry_out.  4 (S (S | 1) + 256 S + S) bytes of LDS:
// 82,432 at S = 64, 26,208 at S = 12.
// Batch route: pl_stream_kernel<!LIVE> is the same forward pass and carry, and leaves the a rows and the integer emissions of the
// new frames in the workspace; pl_window_kernel then takes PL_GROUP = 16 emitted frames per workgroup of four waves, a wave per
// frame in turn, lane = state: table, 16 rows of a and 16 + lag - 1 rows of emissions in LDS (41,472 bytes at S = 64).
// QTCNN_POSE_LAG (consulted per call): 1 forces the live route, 2 the batch route.  Otherwise one new frame goes live, and so do
// n frames with n (lag + 1) <= PL_LIVE_STEPS = 16: the live route runs its windows one after another, n lag dependent steps of
// about 0.5 us at S = 12, the batch route runs them side by side behind a second launch of about 3 us (16 streams, lag 16: 16.5
// against 19.4 us at n = 1, 25.1 against 20.3 at n = 2, 148.0 against 55.6 at n = 16; lag 5: 13.0 against 13.4 at n = 2, 16.9
// against 13.8 at n = 3; scripts/bench_pose_lag.py).  A flush without frames counts its pending frames.
namespace {

constexpr int PL_RING = 128;
constexpr int PL_GROUP = 16;
constexpr int PL_WIN_THREADS = 256;
constexpr int PL_WIN_ROWS = PL_GROUP + PC_LAG_MAX + 1;   // emission rows of a group: frames gs + 1 .. gs + PL_GROUP - 1 + lag
constexpr long long PL_LIVE_STEPS = 16;
static_assert(PC_LAG_MAX + 1 <= PC_TILE, "a window fits the short route");
static_assert(PC_LAG_MAX + PC_TILE < PL_RING && PL_WIN_ROWS <= PL_RING && (PL_RING & (PL_RING - 1)) == 0, "the ring holds a chunk and its windows");

struct PlArgs : PcChain {    // T: the new frames of the call (tiles: not read)
  float* filtered;
  double* evidence;
  const char* carry_in;
  char* carry_out;
  float* lagged;
  float* lagged_class;
  float* ws_a;               // workspace: f32 [batch][n][S], the a rows of the new frames
  short* ws_e;               //            int16 [batch][n][S], their emissions q
  long long seen, g0, g1, carry_stride;
  int lag;
};

// a stream's carry: { double evidence_total; f32 a_last[S]; f32 a[lag][S]; int16 q[lag][S] }, slot k = frame seen - lag + k
struct PlCarry {
  double* ev;
  float* a_last;
  float* a;
  short* e;
};
inline long long pl_carry_stride(int S, int lag) { return (8 + 4LL * S * (1 + lag) + 2LL * S * lag + 7) / 8 * 8; }
__device__ __forceinline__ PlCarry pl_carry(const char* base, long long stride, int b, int S, int lag) {
  char* p = const_cast<char*>(base) + (long long)b * stride;
  PlCarry c;
  c.ev = reinterpret_cast<double*>(p);
  c.a_last = reinterpret_cast<float*>(p + 8);
  c.a = c.a_last + S;
  c.e = reinterpret_cast<short*>(c.a + (long long)lag * S);
  return c;
}
__device__ __forceinline__ short pl_q(float score) { return (short)(int)(score * 256.0f); }   // exact: the score is q / 256

// The window of emitted frame g, one wave, lane = state: b_w = 0, b_f from g[j] = E[f + 1][j] + b_(f + 1)[j] down to f = g, then
// pp_backward's posterior of a_g and b_g (the filtered row itself where w == g).  a_row: a_g in LDS; the emissions of frame f
// are at e_l[((f - ebase) & 127) * S].  Stores lagged and, when asked, lagged_class (lane = class, ascending j).
template <bool SMALL>
__device__ __forceinline__ void pl_window(const PlArgs& r, const PpLds& l, const float (&row)[16], const float* __restrict__ a_row,
                                          const float* __restrict__ e_l, long long ebase, long long g, long long w, int b, int lane) {
  const int S = r.S, C = r.C, jj = min(lane, S - 1);
  float bv = 0.0f;
  for (long long f = w - 1; f >= g; --f) {
    const float gv = e_l[(int)((f + 1 - ebase) & (PL_RING - 1)) * S + jj] + bv;
    bv = pp_b_from_g<SMALL>(l, row, gv, S, jj);
  }
  const float av = a_row[jj];
  float post;
  if (w == g) {
    post = pp_exp2(av);
  } else {
    const float u = av + bv;
    float m, lg;
    pp_L_states<SMALL>(u, S, lane < S, m, lg);
    post = pp_exp2((u - m) - lg);
  }
  const long long slot = (long long)b * (r.g1 - r.g0) + (g - r.g0);
  if (lane < S) r.lagged[slot * S + lane] = post;
  if (r.lagged_class) {
    float s = 0.0f;
    for (int j = 0; j < S; ++j) {
      const float pj = pp_lane(post, j);
      if (l.sc[j] == lane) s += pj;
    }
    if (lane < C) r.lagged_class[slot * C + lane] = s;
  }
}

template <bool SMALL, bool LIVE>
__global__ __launch_bounds__(QT_WAVE) void pl_stream_kernel(PlArgs r) {
  extern __shared__ __attribute__((aligned(16))) float pp_lds[];
  const PcChain& a = r;
  const int lane = threadIdx.x, b = blockIdx.x, S = a.S, SP = S | 1, jj = min(lane, S - 1), lag = r.lag;
  float* a_l = pp_lds + S * SP;                         // [PL_RING][S]
  float* e_l = a_l + PL_RING * S;                       // [PL_RING][S]
  PpLds l;
  l.t = pp_lds;
  l.a = a_l;
  l.e = e_l;
  l.sc = reinterpret_cast<int*>(e_l + PL_RING * S);
  pp_stage_table(a, l);
  const long long seen = r.seen, end = seen + a.T, last = end - 1;
  const PlCarry in = pl_carry(r.carry_in, r.carry_stride, b, S, lag);
  const PlCarry out = pl_carry(r.carry_out, r.carry_stride, b, S, lag);
  double total = seen > 0 ? *in.ev : 0.0, call = 0.0;
  float av = seen > 0 ? in.a_last[jj] : pp_video_start(a, jj);
  for (long long g = seen > lag ? seen - lag : 0; g < seen; ++g) {   // the history: frames seen - lag .. seen - 1 that exist
    const long long k = g - (seen - lag);
    if (lane < S) {
      a_l[(int)(g & (PL_RING - 1)) * S + lane] = in.a[k * S + lane];
      e_l[(int)(g & (PL_RING - 1)) * S + lane] = pc_score(in.e[k * S + lane]);
    }
  }
  __syncthreads();
  float col[16], row[16];
  if (SMALL) {
    pp_load16(col, l.t + jj, SP, S);
    pp_load16(row, l.t + jj * SP, 1, S);
  }
  long long lo = seen;
  do {
    const long long nxt = (lo / PC_TILE + 1) * PC_TILE, hi = nxt < end ? nxt : end;
    const int m = (int)(hi - lo), f0 = (int)(lo - seen), r0 = (int)(lo & (PL_RING - 1)) * S;
    if (m > 0) {
      l.a = a_l + r0;
      l.e = e_l + r0;
      pc_stage_emissions(a, b, f0, m, l.e);
      __syncthreads();
      pp_forward<SMALL>(a, r.filtered, l, col, b, f0, m, lane, av, total, call);
      __syncthreads();
    }
    if (LIVE) {
      const long long first = lo > lag ? lo - lag : 0, until = hi == end ? r.g1 : (hi > lag ? hi - lag : 0);
      for (long long g = first; g < until; ++g) {
        const long long w = g + lag < last ? g + lag : last;
        pl_window<SMALL>(r, l, row, a_l + (int)(g & (PL_RING - 1)) * S, e_l, 0, g, w, b, lane);
      }
    } else {
      float* __restrict__ wa = r.ws_a + ((long long)b * a.T + f0) * S;
      short* __restrict__ we = r.ws_e + ((long long)b * a.T + f0) * S;
      for (int idx = lane; idx < m * S; idx += QT_WAVE) {
        wa[idx] = a_l[r0 + idx];
        we[idx] = pl_q(e_l[r0 + idx]);
      }
    }
    lo = hi;
  } while (lo < end);
  if (lane < S) out.a_last[lane] = av;
  if (lane == 0) {
    *out.ev = total;
    if (r.evidence) r.evidence[b] = call;
  }
  for (int k = 0; k < lag; ++k) {   // frames end - lag .. end - 1: all in the rings; zeros in front of the stream's start
    const long long g = end - lag + k;
    if (lane < S) {
      out.a[k * S + lane] = g >= 0 ? a_l[(int)(g & (PL_RING - 1)) * S + lane] : 0.0f;
      out.e[k * S + lane] = g >= 0 ? pl_q(e_l[(int)(g & (PL_RING - 1)) * S + lane]) : (short)0;
    }
  }
}

template <bool SMALL>
__global__ __launch_bounds__(PL_WIN_THREADS) void pl_window_kernel(PlArgs r) {
  extern __shared__ __attribute__((aligned(16))) float pp_lds[];
  const PcChain& a = r;
  const int tid = threadIdx.x, lane = tid & (QT_WAVE - 1), wave = tid / QT_WAVE, S = a.S, SP = S | 1, jj = min(lane, S - 1);
  const int lag = r.lag;
  PpLds l;
  l.t = pp_lds;
  l.a = l.t + S * SP;                                   // [PL_GROUP][S]: a of frames gs ..
  l.e = l.a + PL_GROUP * S;                             // [PL_WIN_ROWS][S]: row f - gs
  l.sc = reinterpret_cast<int*>(l.e + PL_WIN_ROWS * S);
  const long long count = r.g1 - r.g0, seen = r.seen, last = seen + a.T - 1;
  const int groups = (int)((count + PL_GROUP - 1) / PL_GROUP), b = blockIdx.x / groups, grp = blockIdx.x - b * groups;
  const long long gs = r.g0 + (long long)grp * PL_GROUP, ge = gs + PL_GROUP < r.g1 ? gs + PL_GROUP : r.g1;
  const long long we = ge - 1 + lag < last ? ge - 1 + lag : last;   // the last frame any window of the group reaches
  const PlCarry in = pl_carry(r.carry_in, r.carry_stride, b, S, lag);
  pp_stage_table(a, l);
  for (int idx = tid; idx < (int)(ge - gs) * S; idx += PL_WIN_THREADS) {
    const int fr = (int)fdiv((unsigned)idx, a.div_s), s = idx - fr * S;
    const long long f = gs + fr;
    l.a[idx] = f >= seen ? r.ws_a[((long long)b * a.T + (f - seen)) * S + s] : in.a[(f - (seen - lag)) * S + s];
  }
  for (int idx = tid; idx < (int)(we - gs) * S; idx += PL_WIN_THREADS) {   // frames gs + 1 .. we
    const int fr = (int)fdiv((unsigned)idx, a.div_s) + 1, s = idx - (fr - 1) * S;
    const long long f = gs + fr;
    const short q = f >= seen ? r.ws_e[((long long)b * a.T + (f - seen)) * S + s] : in.e[(f - (seen - lag)) * S + s];
    l.e[fr * S + s] = pc_score(q);
  }
  __syncthreads();
  float row[16];
  if (SMALL) pp_load16(row, l.t + jj * SP, 1, S);
  for (long long g = gs + wave; g < ge; g += PL_WIN_THREADS / QT_WAVE) {
    const long long w = g + lag < last ? g + lag : last;
    pl_window<SMALL>(r, l, row, l.a + (int)(g - gs) * S, l.e, gs, g, w, b, lane);
  }
}

inline size_t pl_stream_lds_bytes(int S) { return 4 * ((size_t)S * (S | 1) + 2 * PL_RING * S + S); }
inline size_t pl_window_lds_bytes(int S) { return 4 * ((size_t)S * (S | 1) + (PL_GROUP + PL_WIN_ROWS) * S + S); }

}  // namespace

extern "C" long long qt_pose_lag_smooth_carry_bytes(const qt_pose_lag_desc* desc) {
  if (pc_lag_check_desc("qt_pose_lag_smooth_carry_bytes", desc) != QT_OK) return 0;
  return desc->batch * pl_carry_stride(desc->num_states, desc->lag);
}

extern "C" long long qt_pose_lag_smooth_workspace_bytes(const qt_pose_lag_desc* desc) {
  if (pc_lag_check_desc("qt_pose_lag_smooth_workspace_bytes", desc) != QT_OK) return 0;
  if (pc_lag_live(desc, PL_LIVE_STEPS)) return 0;
  return ((long long)desc->batch * desc->frames * desc->num_states * 6 + 7) / 8 * 8;
}

extern "C" int qt_pose_lag_smooth(const qt_pose_lag_desc* desc, const float* probs, long long ld, const int* state_class,
                                  const int* trans, const int* init, const void* carry_in, void* carry_out, float* lagged,
                                  float* lagged_class, float* filtered, double* log2_evidence, void* workspace,
                                  long long workspace_bytes, void* stream) {
  const char* const who = "qt_pose_lag_smooth";
  if (const int rc = pc_lag_check_desc(who, desc)) return rc;
  const int B = desc->batch, T = desc->frames, C = desc->num_classes, S = desc->num_states, lag = desc->lag;
  const PcSpan span = pc_lag_span(desc);
  const long long count = span.count;
  QT_CHECK_ARG(ld >= C, "%s: row stride ld = %lld < C = %d", who, ld, C);
  QT_CHECK_ARG((probs != nullptr || T == 0) && state_class != nullptr && trans != nullptr && carry_out != nullptr, "%s: null %s",
               who, !probs && T ? "probs" : !state_class ? "state_class" : !trans ? "trans" : "carry_out");
  QT_CHECK_ARG(count == 0 || lagged != nullptr, "%s: null lagged (the call emits %lld frames)", who, count);
  QT_CHECK_ARG(desc->seen == 0 || carry_in != nullptr, "%s: null carry_in with seen = %lld", who, desc->seen);
  QT_CHECK_ARG(!misaligned(probs, 3) && !misaligned(state_class, 3) && !misaligned(trans, 3) && !misaligned(init, 3) &&
                   !misaligned(lagged, 3) && !misaligned(lagged_class, 3) && !misaligned(filtered, 3) &&
                   !misaligned(carry_in, 7) && !misaligned(carry_out, 7) && !misaligned(log2_evidence, 7) &&
                   !misaligned(workspace, 7),
               "%s: probs, state_class, trans, init, lagged, lagged_class and filtered must be 4-byte aligned, carry_in, "
               "carry_out, log2_evidence and the workspace 8-byte", who);
  const bool live = pc_lag_live(desc, PL_LIVE_STEPS);
  const long long ws_bytes = live ? 0 : ((long long)B * T * S * 6 + 7) / 8 * 8;
  QT_CHECK_ARG(ws_bytes == 0 || (workspace != nullptr && workspace_bytes >= ws_bytes),
               "%s: workspace of %lld bytes; qt_pose_lag_smooth_workspace_bytes asks for %lld", who,
               workspace ? workspace_bytes : 0LL, ws_bytes);
  const long long stride = pl_carry_stride(S, lag), rows = (long long)B * T;
  const size_t carry_bytes = (size_t)(B * stride);
  if (desc->seen == 0) carry_in = nullptr;   // not read
  QT_CHECK_ARG(!overlap(carry_in, carry_bytes, carry_out, carry_bytes), "%s: carry_in must not overlap carry_out", who);
  const PcBuf in[] = {{probs, rows ? (size_t)((rows - 1) * ld + C) * 4 : 0, "probs"},
                      {state_class, (size_t)S * 4, "state_class"}, {trans, (size_t)S * S * 4, "trans"},
                      {init, (size_t)S * 4, "init"}, {carry_in, carry_bytes, "carry_in"}};
  const PcBuf out[] = {{carry_out, carry_bytes, "carry_out"}, {lagged, (size_t)(B * count * S) * 4, "lagged"},
                       {lagged_class, (size_t)(B * count * C) * 4, "lagged_class"},
                       {filtered, (size_t)rows * S * 4, "filtered"}, {log2_evidence, (size_t)B * 8, "log2_evidence"},
                       {workspace, (size_t)ws_bytes, "workspace"}};
  if (const int rc = pc_check_disjoint(who, in, out)) return rc;

  PlArgs r;
  pc_fill(r, probs, ld, state_class, trans, init, T, C, S);
  r.filtered = filtered;
  r.evidence = log2_evidence;
  r.carry_in = static_cast<const char*>(carry_in);
  r.carry_out = static_cast<char*>(carry_out);
  r.lagged = lagged;
  r.lagged_class = lagged_class;
  r.ws_a = static_cast<float*>(workspace);
  r.ws_e = reinterpret_cast<short*>(static_cast<char*>(workspace) + rows * S * 4);
  r.seen = desc->seen;
  r.g0 = span.g0;
  r.g1 = span.g1;
  r.carry_stride = stride;
  r.lag = lag;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool small = S <= 16;
  const size_t lds = pl_stream_lds_bytes(S);
  static std::atomic<unsigned long long> raised[4] = {{0}, {0}, {0}, {0}};
  auto stream_kernel = small ? (live ? pl_stream_kernel<true, true> : pl_stream_kernel<true, false>)
                             : (live ? pl_stream_kernel<false, true> : pl_stream_kernel<false, false>);
  if (lds > 64 * 1024)
    if (int rc = qt_raise_lds_limit(reinterpret_cast<const void*>(stream_kernel), (int)pl_stream_lds_bytes(PC_MAX_S),
                                    raised[(small ? 2 : 0) + (live ? 1 : 0)]))
      return rc;
  hipLaunchKernelGGL(stream_kernel, dim3((unsigned)B), dim3(QT_WAVE), lds, s, r);
  QT_CHECK_LAUNCH();
  if (!live && count > 0) {
    const unsigned grid = (unsigned)(B * ((count + PL_GROUP - 1) / PL_GROUP));
    pc_by_small(S, [&](auto sm) {
      hipLaunchKernelGGL(pl_window_kernel<PC_SMALL(sm)>, dim3(grid), dim3(PL_WIN_THREADS), pl_window_lds_bytes(S), s, r);
    });
    QT_CHECK_LAUNCH();
  }
  return QT_OK;
}
