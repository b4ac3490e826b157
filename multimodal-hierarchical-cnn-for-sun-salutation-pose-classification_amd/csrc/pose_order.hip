// Pose-order decoding on the device (qt_pose_order_decode): the best path of a hidden-Markov chain whose states are the steps
// of the pose sequence, each emitting one class, over the per-frame probabilities of the video loop.  Scores are integers
// (an emission is log2 p in units of 1/256 bit, taken from the float's bit pattern; transitions are int32), so (max, +)
// products are exactly associative and a chain of `frames` dependent steps can be cut into tiles that run in parallel and
// still give the bits of the frame-by-frame rule.  include/qtcnn.h states the rule in full; the reference has no such step.
// pose_chain.h holds what this file shares with pose_posterior.hip and pose_prior.hip: the limits PC_*, the emission rule
// (pc_q, its table, pc_stage_emissions), the chain's inputs PcChain at the head of every argument struct, and the host's
// descriptor checks, fixed-lag route and span, overlap check and S <= 16 launch switch.  Here: the integer kernels.
//
// Short route (frames <= PC_TILE): one launch, one wave per stream, no workspace.  The tile's emissions, the transition
// table, psi and delta are in LDS.  Forward with lane = state j: a step is S times { v_readlane of d[i], add the table entry,
// max }, where value and predecessor travel in one integer, key = 64 (d[i] + trans[i][j]) + (63 - i): the maximum key is the
// maximum value at the lowest i.  For S <= 16 lane j keeps its table column in registers, the sixteen candidates (slots beyond
// S repeat candidate 0, which changes no maximum and needs no branch) are formed independently and meet in a tree of maxima: a
// frame is five dependent steps deep; above that four maxima run side by side over the table in LDS.
// Then filtered (lane = frame, the delta rows padded to an odd stride), the backtrace through psi, the carry.
// Tiled route (frames > PC_TILE), five launches (seven above 32 tiles), M_f[i][j] = trans[i][j] + e[f][j]:
//   (a) po_products: a workgroup of 256 per (stream, tile but the last) forms P = M_a (x) ... (x) M_b in LDS, thread = (i, j),
//       two buffers in turn, one barrier per frame, and writes it to the workspace;
//   (b) po_scan carries a start vector through products in order: wave 0 with lane = j in int32 against an int64 offset, all
//       four waves staging the next trip's products (16 KB, at most 16 of them) through registers into the other LDS buffer
//       meanwhile; every start vector goes to the workspace as int64.  A wave's step costs about 0.4 us, so the chain is two
//       levels deep: tiles go in groups of PO_GROUP = 32; with more than one group po_group_products multiplies each full
//       group's tile products into one (thread = (i, j), as in (a)), one workgroup per stream carries the stream's start through
//       the group products (level 2), and then a workgroup per (stream, group) carries its group's start through its tile
//       products (level 1): at most 31 + (groups - 1) steps in sequence instead of tiles - 1;
//   (c) po_replay: a wave per (stream, tile) replays its frames from its start vector with the short route's vector step:
//       psi, filtered and emissions get the sequential rule's lowest-index ties here (the products carry values only).  It
//       composes its psi maps into one back-map (state at its last frame -> state at the previous tile's last frame, S
//       bytes), leaves psi in the workspace, and the stream's last tile writes its end state and the carry;
//   (d) po_walk: one wave per stream walks the back-maps from the last tile to the first (staged through LDS, 256 tiles at a
//       time) and leaves every tile's end state; po_backtrace: a wave per (stream, tile) walks its psi from that state and
//       writes path.
// No workgroup waits for another inside a launch, no atomics, no zero fill, no host synchronisation; every order is fixed; the
// workspace is the caller's and every slot that is read has been written in the same call.
// QTCNN_POSE_ORDER (consulted per call, so that one process can alternate the forms; measurements only, scripts/
// bench_pose_order.py): 1 = the short route's algorithm as ONE wave per stream over all tiles (psi through the workspace),
// 2 = (d) as one launch in which every tile walks the back-maps from the stream's end to itself, 3 = po_backtrace recomputes
// psi by a second replay instead of reading it from the workspace.  All give the same bits.
#include <limits.h>
#include <stdint.h>

#include "pose_chain.h"

namespace {

constexpr int PO_LOW = -(1 << 24);               // a start vector is taken relative to its maximum and not below this (a carry
                                                 // written by this kernel spreads over 73,728 at the most): 64 frames further
                                                 // down the key 64 v + r still fits 32 bits
constexpr int PO_SCAN_INTS = 4096;               // (b): ints of products per LDS buffer
constexpr int PO_SCAN_MAX_TILES = 16;            // (b): products per trip at the most
constexpr int PO_GROUP = 32;                     // (b): tiles per group: the scan is two levels deep
constexpr int PO_WALK_TILES = 256;               // (d): back-maps staged at a time
constexpr int PO_PROD_THREADS = 256;
constexpr int PO_SCAN_THREADS = 256;
static_assert(PO_SCAN_INTS >= PC_MAX_S * PC_MAX_S && PO_SCAN_INTS % PO_SCAN_THREADS == 0, "a trip holds at least one product");

struct PoArgs : PcChain {
  long long* carry;
  long long* path;
  long long* filtered;
  int* emissions;
  long long* starts;         // workspace: int64 [batch][tiles][S]
  long long* gstarts;        //            int64 [batch][groups][S]
  int* products;             //            int32 [batch][tiles - 1][S][S]
  int* gproducts;            //            int32 [batch][groups - 1][S][S]
  int* ends;                 //            int32 [batch][tiles]
  unsigned char* psi;        //            [batch][T][S]
  unsigned char* back;       //            [batch][tiles][S]
  int groups, mode;
};

__device__ __forceinline__ int po_max16(int (&t)[16]) {
#pragma unroll
  for (int w = 8; w >= 1; w >>= 1)
#pragma unroll
    for (int i = 0; i < w; ++i) t[i] = max(t[i], t[i + w]);
  return t[0];
}

// maximum over the lanes of a wave (every lane calls it and receives it)
__device__ __forceinline__ long long po_wave_max(long long v) {
#pragma unroll
  for (int s = 1; s < QT_WAVE; s <<= 1) {
    const long long o = __shfl_xor(v, s, QT_WAVE);
    v = o > v ? o : v;
  }
  return v;
}
__device__ __forceinline__ int po_wave_max(int v) {
#pragma unroll
  for (int s = 1; s < QT_WAVE; s <<= 1) v = max(v, __shfl_xor(v, s, QT_WAVE));
  return v;
}

// a stream's start vector for lane j: init before its first frame, the carry after it
__device__ __forceinline__ long long po_stream_start(const PoArgs& a, int b, int lane) {
  if (lane >= a.S) return LLONG_MIN;
  const long long* __restrict__ c = a.carry + (long long)b * (a.S + 2);
  if (c[0] == 0) return a.init ? (long long)pc_clamp_trans(a.init[lane]) : 0;
  return c[2 + lane];
}
// D relative to its maximum over the states, as the int32 the tile works in; lanes >= S hold LLONG_MIN and get PO_LOW
__device__ __forceinline__ int po_normalise(long long D, long long& mx) {
  mx = po_wave_max(D);
  const long long r = D == LLONG_MIN ? (long long)PO_LOW : D - mx;
  return (int)(r < (long long)PO_LOW ? (long long)PO_LOW : r);
}

// the LDS of the one-wave kernels
struct PoLds {
  int* tk;               // [S][S]: 64 trans[i][j] + (63 - i)
  int* dl;               // [PC_TILE][S | 1]: delta
  int* path;             // [PC_TILE]
  short* e;              // [PC_TILE][S]
  unsigned char* psi;    // [PC_TILE][S]
};
__device__ __forceinline__ PoLds po_carve(int* lds, int S) {
  PoLds l;
  l.tk = lds;
  l.dl = l.tk + S * S;
  l.path = l.dl + PC_TILE * (S | 1);
  l.e = reinterpret_cast<short*>(l.path + PC_TILE);
  l.psi = reinterpret_cast<unsigned char*>(l.e + PC_TILE * S);
  return l;
}
inline size_t po_wave_lds_bytes(int S) { return 4 * ((size_t)S * S + PC_TILE * (S | 1) + PC_TILE) + 2 * PC_TILE * S + PC_TILE * S; }

__device__ __forceinline__ void po_stage_keys(const PcChain& a, int* tk) {
  const int S = a.S;
  for (int idx = threadIdx.x; idx < S * S; idx += blockDim.x) {
    const int i = (int)fdiv((unsigned)idx, a.div_s);
    tk[idx] = pc_clamp_trans(a.trans[idx]) * 64 + (63 - i);
  }
}

// Forward over the n staged frames, lane = state j (one wave; lanes >= S compute on state S - 1 and store nothing).  d: the
// lane's score before the first frame on entry (maximum 0 over the states), after the last on exit.  Leaves delta and psi in
// LDS.  SMALL: S <= 16, the lane's column of the table in registers.
template <bool SMALL>
__device__ __forceinline__ void po_forward(const PoLds& l, int n, int S, int lane, int& d) {
  const int jj = min(lane, S - 1), SP = S | 1;
  int col[16];
  if (SMALL) {
#pragma unroll
    for (int i = 0; i < 16; ++i) col[i] = l.tk[(i < S ? i : 0) * S + jj];   // slots >= S repeat candidate 0: the maximum stays
  }
  int e = l.e[jj];
  for (int f = 0; f < n; ++f) {
    const int e_next = f + 1 < n ? l.e[(f + 1) * S + jj] : 0;
    int best;
    if (SMALL) {   // sixteen independent candidates, then a tree: the chain of dependent steps is five deep, not S
      int t[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) t[i] = __builtin_amdgcn_readlane(d, i < S ? i : 0) * 64 + col[i];
      best = po_max16(t);
    } else {
      int b0 = INT_MIN, b1 = INT_MIN, b2 = INT_MIN, b3 = INT_MIN;
      const int* __restrict__ tc = l.tk + jj;
      int i = 0;
      for (; i + 3 < S; i += 4) {
        b0 = max(b0, __builtin_amdgcn_readlane(d, i) * 64 + tc[i * S]);
        b1 = max(b1, __builtin_amdgcn_readlane(d, i + 1) * 64 + tc[(i + 1) * S]);
        b2 = max(b2, __builtin_amdgcn_readlane(d, i + 2) * 64 + tc[(i + 2) * S]);
        b3 = max(b3, __builtin_amdgcn_readlane(d, i + 3) * 64 + tc[(i + 3) * S]);
      }
      for (; i < S; ++i) b0 = max(b0, __builtin_amdgcn_readlane(d, i) * 64 + tc[i * S]);
      best = max(max(b0, b1), max(b2, b3));
    }
    d = (best >> 6) + e;
    if (lane < S) {
      l.dl[f * SP + lane] = d;
      l.psi[f * S + lane] = (unsigned char)(63 - (best & 63));
    }
    e = e_next;
  }
}

// the filtered state bj of the lane's frame and its score bv (lane = frame; lanes >= n take frame n - 1) among the n frames
// whose delta is in LDS, rows SP = S | 1 apart: the lowest state at the row's maximum.  The caller broadcasts what it needs.
__device__ __forceinline__ void po_row_argmax(const PoLds& l, int S, int SP, int n, int lane, int& bv, int& bj) {
  const int* __restrict__ row = l.dl + min(lane, n - 1) * SP;
  bv = row[0], bj = 0;
  for (int j = 1; j < S; ++j) {
    const int v = row[j];
    if (v > bv) bv = v, bj = j;
  }
}
// filtered of those n frames to the output when asked.  end / m: the last frame's state and score (wave-uniform).
__device__ __forceinline__ void po_filtered(const PoArgs& a, const PoLds& l, int b, int f0, int n, int lane, int& end, int& m) {
  const int S = a.S, SP = S | 1;
  int bv, bj;
  po_row_argmax(l, S, SP, n, lane, bv, bj);
  if (a.filtered && lane < n) a.filtered[(long long)b * a.T + f0 + lane] = (long long)bj;
  end = __builtin_amdgcn_readlane(bj, n - 1);
  m = __builtin_amdgcn_readlane(bv, n - 1);
}

// path of the n frames whose psi is in LDS, backwards from state s at the last one; returns the state in front of the first
__device__ __forceinline__ int po_backtrace(const PoArgs& a, const PoLds& l, int b, int f0, int n, int lane, int s) {
  const int S = a.S;
  for (int f = n - 1; f >= 0; --f) {
    if (lane == 0) l.path[f] = s;
    s = l.psi[f * S + s];
  }
  __syncthreads();
  if (lane < n) a.path[(long long)b * a.T + f0 + lane] = (long long)l.path[lane];
  return s;
}

// after a stream's last frame: lane j holds delta[last][j] = d relative to `base`; m = max_j d
__device__ __forceinline__ void po_write_carry(const PoArgs& a, int b, int lane, int d, int m, long long base) {
  long long* __restrict__ c = a.carry + (long long)b * (a.S + 2);
  const long long seen = c[0], offset = c[1];
  if (lane < a.S) c[2 + lane] = (long long)(d - m);
  if (lane == 0) {
    c[0] = seen + a.T;
    c[1] = offset + base + m;
  }
}

// ---- the short route, and (QTCNN_POSE_ORDER=1) the same algorithm over all tiles of a stream --------------------------------
template <bool SMALL>
__global__ __launch_bounds__(QT_WAVE) void po_stream_kernel(PoArgs a) {
  extern __shared__ __attribute__((aligned(16))) int po_lds[];
  const PoLds l = po_carve(po_lds, a.S);
  const int lane = threadIdx.x, b = blockIdx.x, S = a.S;
  po_stage_keys(a, l.tk);
  long long base;
  int d = po_normalise(po_stream_start(a, b, lane), base);
  int end = 0, m = 0;
  for (int tile = 0; tile < a.tiles; ++tile) {
    const int f0 = tile * PC_TILE, n = min(PC_TILE, a.T - f0);
    __syncthreads();
    pc_stage_emissions(a, b, f0, n, l.e, a.emissions);
    __syncthreads();
    po_forward<SMALL>(l, n, S, lane, d);
    __syncthreads();
    po_filtered(a, l, b, f0, n, lane, end, m);
    if (a.tiles > 1) {   // psi leaves LDS; the scores are taken relative to their maximum again (max_j d is m)
      unsigned char* __restrict__ out = a.psi + ((long long)b * a.T + f0) * S;
      for (int idx = lane; idx < n * S; idx += QT_WAVE) out[idx] = l.psi[idx];
      if (tile + 1 < a.tiles) {
        d -= m;
        base += m;
        m = 0;
      }
    }
  }
  po_write_carry(a, b, lane, d, m, base);
  int s = end;
  for (int tile = a.tiles - 1; tile >= 0; --tile) {
    const int f0 = tile * PC_TILE, n = min(PC_TILE, a.T - f0);
    if (a.tiles > 1) {
      __syncthreads();
      const unsigned char* __restrict__ in = a.psi + ((long long)b * a.T + f0) * S;
      for (int idx = lane; idx < n * S; idx += QT_WAVE) l.psi[idx] = in[idx];
      __syncthreads();
    }
    s = po_backtrace(a, l, b, f0, n, lane, s);
  }
}

// ---- (a) tile products ------------------------------------------------------------------------------------------------------
// SMALL: S <= 16, so a thread owns one (i, j) for the whole tile: its column of trans stays in registers, and a frame is sixteen
// independent candidates (slots beyond S repeat candidate 0) and a tree of maxima.
// `tiles` (= a.tiles) is an argument of its own on purpose: read out of the struct it rides in the load of T, C and S, the
// prologue is one s_load shorter, the frame loop sits 8 bytes lower in the code object, and the kernel takes 20.4 instead of
// 19.3 us at 64 x 256 frames (EXPERIMENTS.md, "Pose-chain refactor"); with it the loop is where it has been measured.
template <bool SMALL>
__global__ __launch_bounds__(PO_PROD_THREADS) void po_products_kernel(PoArgs a, int tiles) {
  extern __shared__ __attribute__((aligned(16))) int po_lds[];
  const int S = a.S, SS = S * S, tid = threadIdx.x;
  int* tr = po_lds;
  int* cur = tr + SS;
  int* nxt = cur + SS;
  short* e_l = reinterpret_cast<short*>(nxt + SS);
  const int per = tiles - 1;
  const int b = blockIdx.x / per, tile = blockIdx.x - b * per;
  for (int idx = tid; idx < SS; idx += PO_PROD_THREADS) tr[idx] = pc_clamp_trans(a.trans[idx]);
  pc_stage_emissions(a, b, tile * PC_TILE, PC_TILE, e_l);   // (never a stream's last tile: PC_TILE frames)
  __syncthreads();
  for (int idx = tid; idx < SS; idx += PO_PROD_THREADS) {
    const int i = (int)fdiv((unsigned)idx, a.div_s);
    cur[idx] = tr[idx] + e_l[idx - i * S];
  }
  __syncthreads();
  const int own = min(tid, SS - 1), own_i = (int)fdiv((unsigned)own, a.div_s), own_j = own - own_i * S;
  int col[16];
  if (SMALL) {
#pragma unroll
    for (int k = 0; k < 16; ++k) col[k] = tr[(k < S ? k : 0) * S + own_j];
  }
  for (int f = 1; f < PC_TILE; ++f) {
    if (SMALL) {
      int t[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) t[k] = cur[own_i * S + (k < S ? k : 0)] + col[k];
      const int acc = po_max16(t);
      if (tid < SS) nxt[tid] = acc + e_l[f * S + own_j];
    } else {
      for (int idx = tid; idx < SS; idx += PO_PROD_THREADS) {
        const int i = (int)fdiv((unsigned)idx, a.div_s), j = idx - i * S;
        const int* __restrict__ pr = cur + i * S;
        const int* __restrict__ tc = tr + j;
        int acc = INT_MIN;
#pragma unroll 4
        for (int k = 0; k < S; ++k) acc = max(acc, pr[k] + tc[k * S]);
        nxt[idx] = acc + e_l[f * S + j];
      }
    }
    __syncthreads();
    int* t = cur;
    cur = nxt;
    nxt = t;
  }
  int* __restrict__ out = a.products + ((long long)b * per + tile) * SS;
  for (int idx = tid; idx < SS; idx += PO_PROD_THREADS) out[idx] = cur[idx];
}

// ---- (b) the start vector through the products ------------------------------------------------------------------------------
__host__ __device__ inline int po_scan_trip_tiles(int S) {
  const int k = PO_SCAN_INTS / (S * S);
  return k > PO_SCAN_MAX_TILES ? PO_SCAN_MAX_TILES : k;
}
// (a2) a group's product: the PO_GROUP tile products of a full group, in order (the last group's is never needed)
template <bool SMALL>
__global__ __launch_bounds__(PO_PROD_THREADS) void po_group_products_kernel(PoArgs a) {
  extern __shared__ __attribute__((aligned(16))) int po_lds[];
  const int S = a.S, SS = S * S, tid = threadIdx.x;
  int* cur = po_lds;
  int* nxt = cur + SS;
  int* rhs = nxt + SS;
  const int per = a.groups - 1;
  const int b = blockIdx.x / per, g = blockIdx.x - b * per;
  const int* __restrict__ src = a.products + ((long long)b * (a.tiles - 1) + (long long)g * PO_GROUP) * SS;
  for (int idx = tid; idx < SS; idx += PO_PROD_THREADS) cur[idx] = src[idx];
  const int own = min(tid, SS - 1), own_i = (int)fdiv((unsigned)own, a.div_s), own_j = own - own_i * S;
  for (int t = 1; t < PO_GROUP; ++t) {
    for (int idx = tid; idx < SS; idx += PO_PROD_THREADS) rhs[idx] = src[(long long)t * SS + idx];
    __syncthreads();
    if (SMALL) {
      int t[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int kk = k < S ? k : 0;
        t[k] = cur[own_i * S + kk] + rhs[kk * S + own_j];
      }
      const int acc = po_max16(t);
      if (tid < SS) nxt[tid] = acc;
    } else {
      for (int idx = tid; idx < SS; idx += PO_PROD_THREADS) {
        const int i = (int)fdiv((unsigned)idx, a.div_s), j = idx - i * S;
        const int* __restrict__ pr = cur + i * S;
        const int* __restrict__ tc = rhs + j;
        int acc = INT_MIN;
#pragma unroll 4
        for (int k = 0; k < S; ++k) acc = max(acc, pr[k] + tc[k * S]);
        nxt[idx] = acc;
      }
    }
    __syncthreads();
    int* t2 = cur;
    cur = nxt;
    nxt = t2;
  }
  int* __restrict__ out = a.gproducts + ((long long)b * per + g) * SS;
  for (int idx = tid; idx < SS; idx += PO_PROD_THREADS) out[idx] = cur[idx];
}

// level 1: a workgroup per (stream, group) carries the group's start vector through its tile products and leaves every tile's
// start vector; level 2 (run first, when there is more than one group): a workgroup per stream carries the stream's start
// vector through the group products and leaves every group's.  A group product takes a score down by PO_GROUP tiles at once, so
// level 2 takes the scores relative to their maximum again after every product, level 1 once per trip.
template <bool SMALL>
__global__ __launch_bounds__(PO_SCAN_THREADS) void po_scan_kernel(PoArgs a, int level) {
  __shared__ int buf[2][PO_SCAN_INTS];
  constexpr int PER = PO_SCAN_INTS / PO_SCAN_THREADS;
  const int S = a.S, SS = S * S, tid = threadIdx.x, lane = tid & (QT_WAVE - 1);
  const bool chain = tid < QT_WAVE;   // wave 0
  const int K = po_scan_trip_tiles(S), jj = min(lane, S - 1);
  int b, g = 0, count;
  const int* __restrict__ prod;
  long long* __restrict__ starts;
  if (level == 2) {
    b = blockIdx.x;
    count = a.groups - 1;
    prod = a.gproducts + (long long)b * count * SS;
    starts = a.gstarts + (long long)b * a.groups * S;
  } else {
    b = blockIdx.x / a.groups;
    g = blockIdx.x - b * a.groups;
    const int first = g * PO_GROUP;
    count = min(PO_GROUP, a.tiles - first) - 1;
    prod = a.products + ((long long)b * (a.tiles - 1) + first) * SS;
    starts = a.starts + ((long long)b * a.tiles + first) * S;
  }
  long long offset = 0;
  int v = 0;
  if (chain) {
    long long D = po_stream_start(a, b, lane);
    if (g > 0) D = lane < S ? a.gstarts[((long long)b * a.groups + g) * S + lane] : LLONG_MIN;
    if (lane < S) starts[lane] = D;
    v = po_normalise(D, offset);
  }
  int r[PER];
  auto fetch = [&](int t0) {
    const int ints = min(K, count - t0) * SS;
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int idx = tid + u * PO_SCAN_THREADS;
      r[u] = idx < ints ? prod[(long long)t0 * SS + idx] : 0;
    }
  };
  auto put = [&](int* dst) {
#pragma unroll
    for (int u = 0; u < PER; ++u) dst[tid + u * PO_SCAN_THREADS] = r[u];
  };
  fetch(0);
  put(buf[0]);
  __syncthreads();
  int which = 0;
  for (int t0 = 0; t0 < count; t0 += K) {
    const bool more = t0 + K < count;
    if (more) fetch(t0 + K);
    if (chain) {
      if (level != 2) {   // once per trip: K tiles take v down by K * 64 * 73,728 at the most
        const int m = po_wave_max(lane < S ? v : INT_MIN);
        v -= m;
        offset += m;
      }
      const int kt = min(K, count - t0);
      int col[16];
      if (SMALL) {
#pragma unroll
        for (int i = 0; i < 16; ++i) col[i] = buf[which][(i < S ? i : 0) * S + jj];
      }
      for (int u = 0; u < kt; ++u) {
        const int* __restrict__ P = buf[which] + u * SS + jj;
        int nv;
        if (SMALL) {   // the next tile's column is on its way while this tile's sixteen candidates go through the tree
          int nxt[16], t[16];
          const int* __restrict__ Pn = u + 1 < kt ? P + SS : P;
#pragma unroll
          for (int i = 0; i < 16; ++i) nxt[i] = Pn[(i < S ? i : 0) * S];
#pragma unroll
          for (int i = 0; i < 16; ++i) t[i] = __builtin_amdgcn_readlane(v, i < S ? i : 0) + col[i];
          nv = po_max16(t);
#pragma unroll
          for (int i = 0; i < 16; ++i) col[i] = nxt[i];
        } else {
          int b0 = INT_MIN, b1 = INT_MIN, b2 = INT_MIN, b3 = INT_MIN;
          int i = 0;
          for (; i + 3 < S; i += 4) {
            b0 = max(b0, __builtin_amdgcn_readlane(v, i) + P[i * S]);
            b1 = max(b1, __builtin_amdgcn_readlane(v, i + 1) + P[(i + 1) * S]);
            b2 = max(b2, __builtin_amdgcn_readlane(v, i + 2) + P[(i + 2) * S]);
            b3 = max(b3, __builtin_amdgcn_readlane(v, i + 3) + P[(i + 3) * S]);
          }
          for (; i < S; ++i) b0 = max(b0, __builtin_amdgcn_readlane(v, i) + P[i * S]);
          nv = max(max(b0, b1), max(b2, b3));
        }
        v = nv;
        if (level == 2) {
          const int m = po_wave_max(lane < S ? v : INT_MIN);
          v -= m;
          offset += m;
        }
        if (lane < S) starts[(long long)(t0 + u + 1) * S + lane] = offset + v;
      }
    }
    if (more) put(buf[which ^ 1]);
    __syncthreads();
    which ^= 1;
  }
}

// ---- (c) replay ---------------------------------------------------------------------------------------------------------------
template <bool SMALL>
__global__ __launch_bounds__(QT_WAVE) void po_replay_kernel(PoArgs a) {
  extern __shared__ __attribute__((aligned(16))) int po_lds[];
  const PoLds l = po_carve(po_lds, a.S);
  const int lane = threadIdx.x, S = a.S;
  const int b = blockIdx.x / a.tiles, tile = blockIdx.x - b * a.tiles;
  const int f0 = tile * PC_TILE, n = min(PC_TILE, a.T - f0);
  po_stage_keys(a, l.tk);
  pc_stage_emissions(a, b, f0, n, l.e, a.emissions);
  long long base;
  int d = po_normalise(lane < S ? a.starts[((long long)b * a.tiles + tile) * S + lane] : LLONG_MIN, base);
  __syncthreads();
  po_forward<SMALL>(l, n, S, lane, d);
  __syncthreads();
  int end, m;
  po_filtered(a, l, b, f0, n, lane, end, m);
  if (a.mode != 3) {
    unsigned char* __restrict__ out = a.psi + ((long long)b * a.T + f0) * S;
    for (int idx = lane; idx < n * S; idx += QT_WAVE) out[idx] = l.psi[idx];
  }
  // the back-map: lane = the state at the tile's last frame
  int s = min(lane, S - 1);
  for (int f = n - 1; f >= 0; --f) s = l.psi[f * S + s];
  if (lane < S) a.back[((long long)b * a.tiles + tile) * S + lane] = (unsigned char)s;
  if (tile == a.tiles - 1) {
    if (lane == 0) a.ends[(long long)b * a.tiles + tile] = end;
    po_write_carry(a, b, lane, d, m, base);
  }
}

// ---- (d) end states, then every tile's path -----------------------------------------------------------------------------------
__global__ __launch_bounds__(QT_WAVE) void po_walk_kernel(PoArgs a) {
  __shared__ unsigned char maps[PO_WALK_TILES * PC_MAX_S];
  __shared__ int ends_l[PO_WALK_TILES];
  const int lane = threadIdx.x, b = blockIdx.x, S = a.S;
  int* __restrict__ ends = a.ends + (long long)b * a.tiles;
  const unsigned char* __restrict__ back = a.back + (long long)b * a.tiles * S;
  int s = ends[a.tiles - 1];
  for (int hi = a.tiles - 1; hi >= 1; hi -= PO_WALK_TILES) {   // tiles lo + 1 .. hi give the end states of lo .. hi - 1
    const int lo = max(hi - PO_WALK_TILES, 0), cnt = hi - lo;
    for (int idx = lane; idx < cnt * S; idx += QT_WAVE) maps[idx] = back[(long long)(lo + 1) * S + idx];
    __syncthreads();
    for (int u = cnt - 1; u >= 0; --u) {
      s = maps[u * S + s];
      if (lane == 0) ends_l[u] = s;
    }
    __syncthreads();
    for (int idx = lane; idx < cnt; idx += QT_WAVE) ends[lo + idx] = ends_l[idx];
    __syncthreads();
  }
}

template <bool SMALL>
__global__ __launch_bounds__(QT_WAVE) void po_backtrace_kernel(PoArgs a) {
  extern __shared__ __attribute__((aligned(16))) int po_lds[];
  const PoLds l = po_carve(po_lds, a.S);
  const int lane = threadIdx.x, S = a.S;
  const int b = blockIdx.x / a.tiles, tile = blockIdx.x - b * a.tiles;
  const int f0 = tile * PC_TILE, n = min(PC_TILE, a.T - f0);
  int s;
  if (a.mode == 2) {   // every tile walks from the stream's end to itself
    s = a.ends[(long long)b * a.tiles + a.tiles - 1];
    const unsigned char* __restrict__ back = a.back + (long long)b * a.tiles * S;
    for (int u = a.tiles - 1; u > tile; --u) s = back[(long long)u * S + s];
  } else {
    s = a.ends[(long long)b * a.tiles + tile];
  }
  if (a.mode == 3) {   // psi by a second replay
    po_stage_keys(a, l.tk);
    pc_stage_emissions(a, b, f0, n, l.e);
    long long base;
    int d = po_normalise(lane < S ? a.starts[((long long)b * a.tiles + tile) * S + lane] : LLONG_MIN, base);
    __syncthreads();
    po_forward<SMALL>(l, n, S, lane, d);
  } else {
    const unsigned char* __restrict__ in = a.psi + ((long long)b * a.T + f0) * S;
    for (int idx = lane; idx < n * S; idx += QT_WAVE) l.psi[idx] = in[idx];
  }
  __syncthreads();
  po_backtrace(a, l, b, f0, n, lane, s);
}

// the workspace of the tiled route, sections in the order of their alignment
struct PoLayout {
  long long starts, gstarts, products, gproducts, ends, psi, back, total;
};
PoLayout po_layout(const qt_pose_order_desc* d) {
  PoLayout w = {0, 0, 0, 0, 0, 0, 0, 0};
  if (d->frames <= PC_TILE) return w;
  const long long B = d->batch, S = d->num_states, tiles = qt_cdiv(d->frames, PC_TILE);
  const long long groups = qt_cdiv(tiles, PO_GROUP);
  w.starts = 0;
  w.gstarts = w.starts + B * tiles * S * 8;
  w.products = w.gstarts + (groups > 1 ? B * groups * S * 8 : 0);
  w.gproducts = w.products + B * (tiles - 1) * S * S * 4;
  w.ends = w.gproducts + B * (groups - 1) * S * S * 4;
  w.psi = w.ends + B * tiles * 4;
  w.back = w.psi + B * d->frames * S;
  w.total = w.back + B * tiles * S;
  return w;
}

}  // namespace

extern "C" long long qt_pose_order_workspace_bytes(const qt_pose_order_desc* desc) {
  if (pc_check_desc("qt_pose_order_workspace_bytes", desc) != QT_OK) return 0;
  return po_layout(desc).total;
}

extern "C" int qt_pose_order_decode(const qt_pose_order_desc* desc, const float* probs, long long ld, const int* state_class,
                                    const int* trans, const int* init, long long* carry, long long* path, long long* filtered,
                                    int* emissions, void* workspace, long long workspace_bytes, void* stream) {
  const char* const who = "qt_pose_order_decode";
  if (const int rc = pc_check_desc(who, desc)) return rc;
  const int B = desc->batch, T = desc->frames, C = desc->num_classes, S = desc->num_states;
  QT_CHECK_ARG(ld >= C, "%s: row stride ld = %lld < C = %d", who, ld, C);
  QT_CHECK_ARG(probs != nullptr && state_class != nullptr && trans != nullptr && carry != nullptr && path != nullptr,
               "%s: null %s", who, !probs ? "probs" : !state_class ? "state_class" : !trans ? "trans" : !carry ? "carry" : "path");
  QT_CHECK_ARG(!misaligned(probs, 3) && !misaligned(state_class, 3) && !misaligned(trans, 3) && !misaligned(init, 3) &&
                   !misaligned(emissions, 3) && !misaligned(carry, 7) && !misaligned(path, 7) && !misaligned(filtered, 7) &&
                   !misaligned(workspace, 7),
               "%s: probs, state_class, trans, init and emissions must be 4-byte aligned, carry, path, filtered and the "
               "workspace 8-byte", who);
  const PoLayout w = po_layout(desc);
  QT_CHECK_ARG(w.total == 0 || (workspace != nullptr && workspace_bytes >= w.total),
               "%s: workspace of %lld bytes; qt_pose_order_workspace_bytes asks for %lld", who, workspace ? workspace_bytes : 0LL,
               w.total);
  const long long rows = (long long)B * T;
  const PcBuf in[] = {{probs, (size_t)((rows - 1) * ld + C) * 4, "probs"}, {state_class, (size_t)S * 4, "state_class"},
                      {trans, (size_t)S * S * 4, "trans"}, {init, (size_t)S * 4, "init"}};
  const PcBuf out[] = {{carry, (size_t)B * (S + 2) * 8, "carry"}, {path, (size_t)rows * 8, "path"},
                       {filtered, (size_t)rows * 8, "filtered"}, {emissions, (size_t)rows * S * 4, "emissions"},
                       {workspace, (size_t)w.total, "workspace"}};
  if (const int rc = pc_check_disjoint(who, in, out)) return rc;

  const int env_mode = desc->frames > PC_TILE ? qt_env_int("QTCNN_POSE_ORDER", 0) : 0;   // per call: see the head of the file
  PoArgs a;
  pc_fill(a, probs, ld, state_class, trans, init, T, C, S);
  a.carry = carry;
  a.path = path;
  a.filtered = filtered;
  a.emissions = emissions;
  char* ws = static_cast<char*>(workspace);
  a.starts = reinterpret_cast<long long*>(ws + w.starts);
  a.gstarts = reinterpret_cast<long long*>(ws + w.gstarts);
  a.products = reinterpret_cast<int*>(ws + w.products);
  a.gproducts = reinterpret_cast<int*>(ws + w.gproducts);
  a.ends = reinterpret_cast<int*>(ws + w.ends);
  a.psi = reinterpret_cast<unsigned char*>(ws + w.psi);
  a.back = reinterpret_cast<unsigned char*>(ws + w.back);
  a.groups = qt_cdiv(a.tiles, PO_GROUP);
  a.mode = a.tiles > 1 && env_mode >= 1 && env_mode <= 3 ? env_mode : 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t wave_lds = po_wave_lds_bytes(S);
  const dim3 wave(QT_WAVE), prod(PO_PROD_THREADS), scan(PO_SCAN_THREADS);
  if (a.tiles == 1 || a.mode == 1) {
    const dim3 streams((unsigned)B);
    pc_by_small(S, [&](auto sm) { hipLaunchKernelGGL(po_stream_kernel<PC_SMALL(sm)>, streams, wave, wave_lds, s, a); });
    QT_CHECK_LAUNCH();
    return QT_OK;
  }
  const dim3 all((unsigned)((long long)B * a.tiles)), inner((unsigned)((long long)B * (a.tiles - 1)));
  const size_t prod_lds = 4 * 3 * (size_t)S * S + 2 * PC_TILE * S;
  pc_by_small(S, [&](auto sm) { hipLaunchKernelGGL(po_products_kernel<PC_SMALL(sm)>, inner, prod, prod_lds, s, a, a.tiles); });
  QT_CHECK_LAUNCH();
  if (a.groups > 1) {
    const dim3 full((unsigned)((long long)B * (a.groups - 1)));
    pc_by_small(S, [&](auto sm) {
      hipLaunchKernelGGL(po_group_products_kernel<PC_SMALL(sm)>, full, prod, 4 * 3 * (size_t)S * S, s, a);
    });
    QT_CHECK_LAUNCH();
    pc_by_small(S, [&](auto sm) { hipLaunchKernelGGL(po_scan_kernel<PC_SMALL(sm)>, dim3((unsigned)B), scan, 0, s, a, 2); });
    QT_CHECK_LAUNCH();
  }
  const dim3 scans((unsigned)((long long)B * a.groups));
  pc_by_small(S, [&](auto sm) { hipLaunchKernelGGL(po_scan_kernel<PC_SMALL(sm)>, scans, scan, 0, s, a, 1); });
  QT_CHECK_LAUNCH();
  pc_by_small(S, [&](auto sm) { hipLaunchKernelGGL(po_replay_kernel<PC_SMALL(sm)>, all, wave, wave_lds, s, a); });
  QT_CHECK_LAUNCH();
  if (a.mode != 2) {
    hipLaunchKernelGGL(po_walk_kernel, dim3((unsigned)B), wave, 0, s, a);
    QT_CHECK_LAUNCH();
  }
  pc_by_small(S, [&](auto sm) { hipLaunchKernelGGL(po_backtrace_kernel<PC_SMALL(sm)>, all, wave, wave_lds, s, a); });
  QT_CHECK_LAUNCH();
  return QT_OK;
}

// ---- fixed-lag paths across calls (qt_pose_lag_decode) ------------------------------------------------------------------------
// lag_path[g] is the state at frame g of the best path that ends at frame w = min(g + lag, the call's last frame): the forward
// pass is the integer rule above (po_forward as it is, the scores taken relative to their maximum after every chunk), and every
// emitted frame walks psi back from filtered[w].  Frames carry global indices; the LDS rings hold psi and filtered of frame g in
// row g & 127, and the forward pass goes in chunks that end on multiples of PC_TILE so that a chunk's rows are one run.
// Live route: pld_stream_kernel<LIVE>, one launch, one wave per stream; the walks run with lane = emitted frame, lag byte reads
// each.  Batch route: the same forward pass leaves psi and filtered of the new frames in the workspace, and pld_walk_kernel
// walks with one thread per emitted frame, psi from the workspace or from carry_in's history.  Integers: the same bits.
// The live route's walks cost a chunk of 64 frames about a tenth of its forward pass, the batch route's second launch about
// 3 us: n (lag + 1) <= PLD_LIVE_STEPS = 4096 goes live (16 streams, lag 16, n = 1 .. 16: 10.2 .. 11.5 us against 13.0 .. 15.0;
// 64 x 256: 79.7 against 80.3; 1 x 65,536: 21.4 against 19.7 ms; scripts/bench_pose_lag.py), QTCNN_POSE_LAG=1 / 2 forces either.
namespace {

constexpr int PLD_RING = 128;
constexpr int PLD_WALK_THREADS = 256;
constexpr long long PLD_LIVE_STEPS = 4096;
static_assert(PC_LAG_MAX + PC_TILE < PLD_RING && (PLD_RING & (PLD_RING - 1)) == 0,
              "the ring holds a chunk and its windows");

struct PldArgs : PcChain {   // T: the new frames of the call (tiles: not read)
  long long* filtered;
  const char* carry_in;
  char* carry_out;
  long long* lag_path;
  unsigned char* ws_psi;     // workspace: [batch][n][S]
  int* ws_filt;              //            int32 [batch][n]
  long long seen, g0, g1, carry_stride;
  int lag;
};

// a stream's carry: { int64 score_offset; int32 delta[S] (maximum 0); uint8 psi[lag][S] }, slot k = frame seen - lag + k
struct PldCarry {
  long long* offset;
  int* delta;
  unsigned char* psi;
};
inline long long pld_carry_stride(int S, int lag) { return (8 + 4LL * S + (long long)lag * S + 7) / 8 * 8; }
__device__ __forceinline__ PldCarry pld_carry(const char* base, long long stride, int b, int S) {
  char* p = const_cast<char*>(base) + (long long)b * stride;
  PldCarry c;
  c.offset = reinterpret_cast<long long*>(p);
  c.delta = reinterpret_cast<int*>(p + 8);
  c.psi = reinterpret_cast<unsigned char*>(c.delta + S);
  return c;
}
inline size_t pld_stream_lds_bytes(int S) {
  return 4 * ((size_t)S * S + PC_TILE * (S | 1) + PLD_RING) + 2 * PC_TILE * S + PLD_RING * S;
}

template <bool SMALL, bool LIVE>
__global__ __launch_bounds__(QT_WAVE) void pld_stream_kernel(PldArgs r) {
  extern __shared__ __attribute__((aligned(16))) int po_lds[];
  const PcChain& a = r;
  const int lane = threadIdx.x, b = blockIdx.x, S = a.S, SP = S | 1, lag = r.lag;
  PoLds l;
  l.tk = po_lds;
  l.dl = l.tk + S * S;                                   // [PC_TILE][S | 1]
  int* filt_l = l.dl + PC_TILE * SP;                     // [PLD_RING]
  l.path = filt_l;
  l.e = reinterpret_cast<short*>(filt_l + PLD_RING);     // [PC_TILE][S]
  unsigned char* psi_l = reinterpret_cast<unsigned char*>(l.e + PC_TILE * S);   // [PLD_RING][S]
  l.psi = psi_l;
  po_stage_keys(a, l.tk);
  const long long seen = r.seen, end = seen + a.T, last = end - 1, count = r.g1 - r.g0;
  const PldCarry in = pld_carry(r.carry_in, r.carry_stride, b, S);
  const PldCarry out = pld_carry(r.carry_out, r.carry_stride, b, S);
  long long D = LLONG_MIN;
  if (lane < S) D = seen > 0 ? (long long)in.delta[lane] : (a.init ? (long long)pc_clamp_trans(a.init[lane]) : 0);
  long long base;
  int d = po_normalise(D, base);
  long long offset = (seen > 0 ? *in.offset : 0) + base;
  if (seen > 0) {   // filtered of the frame in front of the call: the lowest state at the carry's maximum
    const unsigned long long top = __ballot(lane < S && d == 0);
    if (lane == 0) filt_l[(int)((seen - 1) & (PLD_RING - 1))] = __ffsll((long long)top) - 1;
    for (long long g = seen > lag ? seen - lag : 0; g < seen; ++g)
      if (lane < S) psi_l[(int)(g & (PLD_RING - 1)) * S + lane] = in.psi[(g - (seen - lag)) * S + lane];
  }
  long long lo = seen;
  do {
    const long long nxt = (lo / PC_TILE + 1) * PC_TILE, hi = nxt < end ? nxt : end;
    const int m = (int)(hi - lo), f0 = (int)(lo - seen), r0 = (int)(lo & (PLD_RING - 1));
    __syncthreads();
    if (m > 0) {
      l.psi = psi_l + r0 * S;
      pc_stage_emissions(a, b, f0, m, l.e);
      __syncthreads();
      po_forward<SMALL>(l, m, S, lane, d);
      __syncthreads();
      int bv, bj;
      po_row_argmax(l, S, SP, m, lane, bv, bj);   // filtered, lane = frame
      if (lane < m) {
        filt_l[r0 + lane] = bj;
        if (r.filtered) r.filtered[(long long)b * a.T + f0 + lane] = (long long)bj;
      }
      const int mx = __builtin_amdgcn_readlane(bv, m - 1);
      d -= mx;
      offset += mx;
      __syncthreads();
    }
    if (LIVE) {
      const long long first = lo > lag ? lo - lag : 0, until = hi == end ? r.g1 : (hi > lag ? hi - lag : 0);
      for (long long g = first + lane; g < until; g += QT_WAVE) {
        const long long w = g + lag < last ? g + lag : last;
        int s = filt_l[(int)(w & (PLD_RING - 1))];
        for (long long f = w; f > g; --f) s = psi_l[(int)(f & (PLD_RING - 1)) * S + s];
        r.lag_path[(long long)b * count + (g - r.g0)] = (long long)s;
      }
    } else {
      unsigned char* __restrict__ wp = r.ws_psi + ((long long)b * a.T + f0) * S;
      for (int idx = lane; idx < m * S; idx += QT_WAVE) wp[idx] = psi_l[r0 * S + idx];
      if (lane < m) r.ws_filt[(long long)b * a.T + f0 + lane] = filt_l[r0 + lane];
    }
    lo = hi;
  } while (lo < end);
  if (lane < S) out.delta[lane] = d;
  if (lane == 0) *out.offset = offset;
  for (int k = 0; k < lag; ++k) {   // frames end - lag .. end - 1: all in the ring; zeros in front of the stream's start
    const long long g = end - lag + k;
    if (lane < S) out.psi[k * S + lane] = g >= 0 ? psi_l[(int)(g & (PLD_RING - 1)) * S + lane] : (unsigned char)0;
  }
}

// thread = (stream, emitted frame)
__global__ __launch_bounds__(PLD_WALK_THREADS) void pld_walk_kernel(PldArgs r, int batch) {
  const PcChain& a = r;
  const long long count = r.g1 - r.g0, idx = (long long)blockIdx.x * PLD_WALK_THREADS + threadIdx.x;
  if (idx >= count * batch) return;
  const int b = (int)(idx / count), S = a.S, lag = r.lag;
  const long long g = r.g0 + (idx - (long long)b * count), seen = r.seen, last = seen + a.T - 1;
  const long long w = g + lag < last ? g + lag : last;
  const PldCarry in = pld_carry(r.carry_in, r.carry_stride, b, S);
  int s = 0;
  if (w >= seen) {
    s = r.ws_filt[(long long)b * a.T + (w - seen)];
  } else {   // (a flush without new frames) the frame in front of the call: the lowest state at the carry's maximum
    int bv = in.delta[0];
    for (int j = 1; j < S; ++j) {
      const int v = in.delta[j];
      if (v > bv) bv = v, s = j;
    }
  }
  for (long long f = w; f > g; --f) {
    const unsigned char* __restrict__ row =
        f >= seen ? r.ws_psi + ((long long)b * a.T + (f - seen)) * S : in.psi + (f - (seen - lag)) * S;
    s = row[s];
  }
  r.lag_path[idx] = (long long)s;
}

}  // namespace

extern "C" long long qt_pose_lag_decode_carry_bytes(const qt_pose_lag_desc* desc) {
  if (pc_lag_check_desc("qt_pose_lag_decode_carry_bytes", desc) != QT_OK) return 0;
  return desc->batch * pld_carry_stride(desc->num_states, desc->lag);
}

extern "C" long long qt_pose_lag_decode_workspace_bytes(const qt_pose_lag_desc* desc) {
  if (pc_lag_check_desc("qt_pose_lag_decode_workspace_bytes", desc) != QT_OK) return 0;
  if (pc_lag_live(desc, PLD_LIVE_STEPS)) return 0;
  const long long rows = (long long)desc->batch * desc->frames;
  return ((rows * desc->num_states + 7) / 8 * 8) + (rows * 4 + 7) / 8 * 8;
}

extern "C" int qt_pose_lag_decode(const qt_pose_lag_desc* desc, const float* probs, long long ld, const int* state_class,
                                  const int* trans, const int* init, const void* carry_in, void* carry_out, long long* lag_path,
                                  long long* filtered, void* workspace, long long workspace_bytes, void* stream) {
  const char* const who = "qt_pose_lag_decode";
  if (const int rc = pc_lag_check_desc(who, desc)) return rc;
  const int B = desc->batch, T = desc->frames, C = desc->num_classes, S = desc->num_states, lag = desc->lag;
  const PcSpan span = pc_lag_span(desc);
  const long long count = span.count;
  QT_CHECK_ARG(ld >= C, "%s: row stride ld = %lld < C = %d", who, ld, C);
  QT_CHECK_ARG((probs != nullptr || T == 0) && state_class != nullptr && trans != nullptr && carry_out != nullptr, "%s: null %s",
               who, !probs && T ? "probs" : !state_class ? "state_class" : !trans ? "trans" : "carry_out");
  QT_CHECK_ARG(count == 0 || lag_path != nullptr, "%s: null lag_path (the call emits %lld frames)", who, count);
  QT_CHECK_ARG(desc->seen == 0 || carry_in != nullptr, "%s: null carry_in with seen = %lld", who, desc->seen);
  QT_CHECK_ARG(!misaligned(probs, 3) && !misaligned(state_class, 3) && !misaligned(trans, 3) && !misaligned(init, 3) &&
                   !misaligned(lag_path, 7) && !misaligned(filtered, 7) && !misaligned(carry_in, 7) &&
                   !misaligned(carry_out, 7) && !misaligned(workspace, 7),
               "%s: probs, state_class, trans and init must be 4-byte aligned, carry_in, carry_out, lag_path, filtered and the "
               "workspace 8-byte", who);
  const bool live = pc_lag_live(desc, PLD_LIVE_STEPS);
  const long long rows = (long long)B * T, psi_bytes = (rows * S + 7) / 8 * 8;
  const long long ws_bytes = live ? 0 : psi_bytes + (rows * 4 + 7) / 8 * 8;
  QT_CHECK_ARG(ws_bytes == 0 || (workspace != nullptr && workspace_bytes >= ws_bytes),
               "%s: workspace of %lld bytes; qt_pose_lag_decode_workspace_bytes asks for %lld", who,
               workspace ? workspace_bytes : 0LL, ws_bytes);
  const long long stride = pld_carry_stride(S, lag);
  const size_t carry_bytes = (size_t)(B * stride);
  if (desc->seen == 0) carry_in = nullptr;   // not read
  QT_CHECK_ARG(!overlap(carry_in, carry_bytes, carry_out, carry_bytes), "%s: carry_in must not overlap carry_out", who);
  const PcBuf in[] = {{probs, rows ? (size_t)((rows - 1) * ld + C) * 4 : 0, "probs"},
                      {state_class, (size_t)S * 4, "state_class"}, {trans, (size_t)S * S * 4, "trans"},
                      {init, (size_t)S * 4, "init"}, {carry_in, carry_bytes, "carry_in"}};
  const PcBuf out[] = {{carry_out, carry_bytes, "carry_out"}, {lag_path, (size_t)(B * count) * 8, "lag_path"},
                       {filtered, (size_t)rows * 8, "filtered"}, {workspace, (size_t)ws_bytes, "workspace"}};
  if (const int rc = pc_check_disjoint(who, in, out)) return rc;

  PldArgs r;
  pc_fill(r, probs, ld, state_class, trans, init, T, C, S);
  r.filtered = filtered;
  r.carry_in = static_cast<const char*>(carry_in);
  r.carry_out = static_cast<char*>(carry_out);
  r.lag_path = lag_path;
  r.ws_psi = static_cast<unsigned char*>(workspace);
  r.ws_filt = reinterpret_cast<int*>(static_cast<char*>(workspace) + psi_bytes);
  r.seen = desc->seen;
  r.g0 = span.g0;
  r.g1 = span.g1;
  r.carry_stride = stride;
  r.lag = lag;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool small = S <= 16;
  auto stream_kernel = small ? (live ? pld_stream_kernel<true, true> : pld_stream_kernel<true, false>)
                             : (live ? pld_stream_kernel<false, true> : pld_stream_kernel<false, false>);
  hipLaunchKernelGGL(stream_kernel, dim3((unsigned)B), dim3(QT_WAVE), pld_stream_lds_bytes(S), s, r);
  QT_CHECK_LAUNCH();
  if (!live && count > 0) {
    const unsigned grid = (unsigned)((B * count + PLD_WALK_THREADS - 1) / PLD_WALK_THREADS);
    hipLaunchKernelGGL(pld_walk_kernel, dim3(grid), dim3(PLD_WALK_THREADS), 0, s, r, B);
    QT_CHECK_LAUNCH();
  }
  return QT_OK;
}
