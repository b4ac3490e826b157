// The stream kernel of the chain with hold durations' forward-backward, shared by the posteriors (pose_duration_posterior.hip,
// LEARN = false) and the learner's E-step (pose_duration_prior.hip, LEARN = true), so that both walk the very same forward and
// backward sweeps: Z and the expected duration counts of the two are the same bits.  include/qtcnn.h states the rules in full.
// The arithmetic of a step (pp_group_L .. pp_class_sum below) stands apart from the kernel as device functions: the fixed-lag
// posteriors (pose_duration_lag_posterior.hip) walk a stream's forward sweep across calls and a backward sweep per emitted frame
// with the same functions, which is how their rows are this kernel's bits on the stream's prefix.
//
// The walk is pose_duration.hip's, from the pieces of pose_duration_chain.h: one workgroup of 256 per stream, a group of LPS
// lanes per state (16 for S <= 16, 4 above) with the state's slices of dur and dur_open in registers (lane l the lengths
// d = 1 + l + k LPS), the emissions staged PC_DUR_CHUNK frames at a time, the last D frames of history as a ring [D][S] in
// dynamic LDS.  A level (Bt, Al, Be, Bs, Z) is a
// double: it falls by up to 288 bits a frame.  An L = log2 sum 2^x is a group maximum in double and then a group sum of the f32
// terms 2^(x - m) over the same candidates, each lane its own in ascending order and the lanes by a butterfly, so the order
// depends on S and D alone.  With cum[f][j] the exact int64 prefix sum of the emissions:
//   forward, f = 1 .. T: the ring holds g[f][j] = Bt[f][j] - cum[f][j] / 256;
//     (A) Al[f][j] = cum[f][j] / 256 + L_d (g[f - d][j] + len(j, d, f))                                             barrier
//     (B) Bt[f][j] = L_i (Al[f][i] + T[i][j]); g[f] goes to ring row f mod D (row f - D was last read in (A))        barrier
//     Al[f] and g[f] also go to the workspace as doubles; after f = T every thread forms Z = L_j Al[T][j] in ascending j.
//   backward, f = T - 1 .. 0, after a barrier: the ring is reused for h[f][j] = Be[f][j] + cum[f][j] / 256, cum steps back
//     through the emissions staged in descending chunks;
//     (A') Lh = L_d (h[f + d][j] + len(j, d, f + d)), Bs[f][j] = Lh - cum[f][j] / 256; the state's owner lane forms
//          begin[f][j] = 2^(g[f][j] + Lh - Z), endp[f + 1][j] from the workspace's Al row and the Be it kept, and steps occ;   barrier
//     (B') Be[f][i] = L_j (T[i][j] + Bs[f][j]), h[f] to ring row f mod D (row f + D was last read in (A')); the owner sums
//          R in ascending j and writes the posterior row; each lane adds the count terms of its own (j, d) slots at this f,
//          2^(g[f - d][j] + Dur[j][d - 1] + h[f][j] - Z) with g from the workspace, into double registers;             barrier
//     the class posterior of frame f + 1 is summed in (A') from the row that (B') left in LDS, the one of frame 0 after the walk.
// LEARN: no posterior, begin or class rows and no occ.  In (B') lane l of group i, which visits j = l, l + LPS, .. for Be[f][i],
// also adds xi_f[i][j] = 2^((T[i][j] + Bs[f][j]) + (Al[f][i] - Z)) into the double register of its (i, j) slot, Al[f][i] from the
// workspace row the forward sweep stored (S / LPS <= 16 slots per lane); at f = 0 the owner of state i sums xi_0[i][j] with
// start[i] for Al over ascending j.  No LDS beyond the posterior's.
// A stream's partial counts (and, LEARN, its Z) go to the workspace; a second small launch of the including file adds the
// streams' partials in ascending stream order, from zero, onto the accumulators.  No workgroup waits for another, no atomics,
// no host synchronisation; every workspace slot that is read has been written in the same call (a workgroup reads its own
// stores behind barriers).
#pragma once
#include <float.h>
#include <stdint.h>

#include "pose_chain.h"
#include "pose_duration_chain.h"

namespace {

struct PpArgs : PcDurChain {   // T: the frames of the descriptor
  float* posterior;
  float* class_posterior;
  float* begin;
  double* evidence;
  double* g;                 // workspace [batch][T][S]: g[f][j], f = 0 .. T - 1
  double* al;                // workspace [batch][T][S]: Al[f][j] in row f - 1
  double* part;              // workspace [batch][S][D]: a stream's expected counts; null without dur_counts
  double* xi_part;           // LEARN: workspace [batch][S][S], a stream's expected transition counts
  double* start_part;        // LEARN: workspace [batch][S], a stream's xi_0 row sums; null without start_counts
  double* z_part;            // LEARN: workspace [batch], a stream's Z
};

// the ring, two rows of doubles (a level; Bs), trans, state_class, a posterior row, the staged emissions
inline size_t pp_lds_bytes(int S, int D) {
  return 8 * ((size_t)D * S + 2 * S) + 4 * ((size_t)S * S + 2 * S) + 2 * (size_t)PC_DUR_CHUNK * S;
}
inline long long pp_level_elems(const qt_pose_duration_desc* d) { return (long long)d->batch * d->frames * d->num_states; }
inline long long pp_workspace_bytes(const qt_pose_duration_desc* d) {
  return 8 * (2 * pp_level_elems(d) + (long long)d->batch * d->num_states * d->max_duration);
}

template <int LPS>
__device__ __forceinline__ double pp_group_max(double v) {
#pragma unroll
  for (int s = 1; s < LPS; s <<= 1) v = fmax(v, __shfl_xor(v, s, QT_WAVE));
  return v;
}
// the butterfly: every lane of the group receives the same bits (a + b == b + a)
template <int LPS>
__device__ __forceinline__ float pp_group_sum(float v) {
#pragma unroll
  for (int s = 1; s < LPS; s <<= 1) v += __shfl_xor(v, s, QT_WAVE);
  return v;
}
__device__ __forceinline__ double pp_bits(long long v) { return (double)v * 0x1p-8; }   // exact: |v| < 2^53
__device__ __forceinline__ float pp_term(double x) { return exp2f((float)x); }

// The arithmetic of the sweeps, one body for every kernel that walks them (pp_stream_kernel below and the fixed-lag posteriors
// of pose_duration_lag_posterior.hip, whose bits are the whole-video kernel's because they run these very functions).
// L over the group's share of `n` candidates x(i), i = l, l + LPS, ..: the maximum out in double, the terms and their sum f32
template <int LPS, typename X>
__device__ __forceinline__ double pp_group_L(int n, int l, X&& x) {
  double m = -DBL_MAX;
  for (int i = l; i < n; i += LPS) m = fmax(m, x(i));
  m = pp_group_max<LPS>(m);
  float s = 0.0f;
  for (int i = l; i < n; i += LPS) s += pp_term(x(i) - m);
  return m + (double)log2f(pp_group_sum<LPS>(s));
}
// L over the state's lengths d = 1 .. dmax, the row of length d of ring [D][S] being row0 - d (forward) or row0 + d (backward),
// wrapped; dur_open scores the length d_cut, and every length where `cut`
template <int LPS>
__device__ __forceinline__ double pp_length_L(const PcDurLane<LPS>& ln, const double* ring, int S, int D, int dmax, int row0,
                                              bool forward, int d_cut, bool cut) {
  double x[PcDurLane<LPS>::KMAX];
  double m = -DBL_MAX;
  pc_for_lengths<LPS>(dmax, ln.l, [&](int k, int d) {
    const int r = pc_ring_wrap(forward ? row0 - d : row0 + d, D);
    x[k] = ring[r * S + ln.jj] + pp_bits((cut || d == d_cut) ? ln.dop[k] : ln.du[k]);
    m = fmax(m, x[k]);
  });
  m = pp_group_max<LPS>(m);
  float s = 0.0f;
  pc_for_lengths<LPS>(dmax, ln.l, [&](int k, int) { s += pp_term(x[k] - m); });
  return m + (double)log2f(pp_group_sum<LPS>(s));
}
// Z = L_j lev[j] in ascending j, by one thread
__device__ __forceinline__ double pp_evidence(const double* lev, int S) {
  double m = lev[0];
  for (int s = 1; s < S; ++s) m = fmax(m, lev[s]);
  float sum = 0.0f;
  for (int s = 0; s < S; ++s) sum += pp_term(lev[s] - m);
  return m + (double)log2f(sum);
}
// the owner lane's step of the backward sweep at frame f: begin[f] from g[f] and Lh (the cum terms cancel), endp[f + 1] from
// Al[f + 1] and Be[f + 1]; occ[f + 1] becomes occ[f] (`last`: f is the sweep's last frame) and begin_next begin[f], returned
__device__ __forceinline__ float pp_owner_step(double g, double lh, double al_next, double be_next, double Z, bool last,
                                               double& occ, float& begin_next) {
  const float bg = pp_term(g + lh - Z);
  const float ep = pp_term(al_next + be_next - Z);
  occ = last ? (double)ep : occ + (double)ep - (double)begin_next;
  begin_next = bg;
  return bg;
}
// state j's entry of the posterior row from r = max(occ, 0) [S]: R in ascending j, double
__device__ __forceinline__ float pp_row(const double* r, int S, int j) {
  double R = 0.0;
  for (int i = 0; i < S; ++i) R += r[i];
  return R > 0.0 ? (float)(r[j] / R) : (float)(1.0 / S);
}
// class c's entry of the class posterior from the posterior row pst [S]: ascending j, f32
__device__ __forceinline__ float pp_class_sum(const float* pst, const int* sc, int S, int c) {
  float s = 0.0f;
  for (int i = 0; i < S; ++i)
    if (sc[i] == c) s += pst[i];
  return s;
}

template <bool SMALL, bool LEARN>
__global__ __launch_bounds__(PC_DUR_THREADS) void pp_stream_kernel(PpArgs a) {
  constexpr int LPS = PC_DUR_LPS<SMALL>;
  constexpr int KMAX = PcDurLane<LPS>::KMAX;     // lengths per lane
  constexpr int XMAX = SMALL ? 1 : PC_MAX_S / LPS;   // LEARN: (i, j) slots per lane, j = l + k LPS
  extern __shared__ __attribute__((aligned(16))) double pp_lds[];
  const int S = a.S, C = a.C, D = a.D, tid = threadIdx.x, b = blockIdx.x;
  double* ring = pp_lds;                                     // [D][S]: g, then h, of the last D frames, row f mod D
  double* lev = ring + D * S;                                // [S]: start, Al[f]; backward: r = max(occ, 0)
  double* vec = lev + S;                                     // [S]: Bs[f]
  int* tr = reinterpret_cast<int*>(vec + S);                 // [S][S]
  int* sc = tr + S * S;                                      // [S]
  float* pst = reinterpret_cast<float*>(sc + S);             // [S]: the posterior row of the frame (B') last passed
  short* e_l = reinterpret_cast<short*>(pst + S);            // [PC_DUR_CHUNK][S]
  const PcDurLane<LPS> ln(tid, S, D, a.dur, a.dur_open);
  const int j = ln.j, l = ln.l, jj = ln.jj;
  const bool own = ln.own;
  const int T = pc_stream_length(a.lengths, b, a.T);
  pc_stage_trans(a.trans, tr, S);
  if (tid < S) {
    lev[tid] = pp_bits(pc_init_score(a.init, tid));
    sc[tid] = a.state_class[tid];
  }
  __syncthreads();

  auto group_L = [&](int n, auto x) -> double { return pp_group_L<LPS>(n, l, x); };
  auto length_L = [&](int dmax, int row0, bool forward, int d_cut, bool cut) -> double {
    return pp_length_L<LPS>(ln, ring, S, D, dmax, row0, forward, d_cut, cut);
  };

  // ---- forward ---------------------------------------------------------------------------------------------------------------
  const long long base = (long long)b * a.T * S;
  double* __restrict__ gw = a.g + base;
  double* __restrict__ alw = a.al + base;
  long long cum = 0;
  double bt = group_L(S, [&](int i) { return lev[i] + pp_bits(tr[i * S + jj]); });       // Bt[0]; cum[0] = 0
  if (own) ring[j] = bt, gw[j] = bt;
  int row = 0;
  double Z = 0.0;
  for (int f = 1; f <= T; ++f) {
    const int g = f - 1;
    cum += pc_chunk_row(a, b, g, T, e_l, pc_chunk_start(g))[jj];
    row = pc_ring_next(row, D);                  // f mod D
    const double alv = length_L(min(D, f), row, true, f, f == T) + pp_bits(cum);
    if (own) lev[j] = alv, alw[(long long)g * S + j] = alv;
    __syncthreads();
    if (f < T) {
      bt = group_L(S, [&](int i) { return lev[i] + pp_bits(tr[i * S + jj]); });
      if (own) {
        const double gv = bt - pp_bits(cum);
        ring[row * S + j] = gv;
        gw[(long long)f * S + j] = gv;
      }
    } else {                                     // Z, by every thread, in ascending j
      Z = pp_evidence(lev, S);
      if (tid == 0 && a.evidence) a.evidence[b] = Z;
    }
    __syncthreads();
  }

  // ---- backward --------------------------------------------------------------------------------------------------------------
  const bool rows_out = a.posterior || a.class_posterior;
  const long long out_row = (long long)b * a.T;
  // the class posterior of frame t from the posterior row in pst: ascending j, f32
  auto class_row = [&](int t) {
    if (a.class_posterior && tid < C) a.class_posterior[(out_row + t) * C + tid] = pp_class_sum(pst, sc, S, tid);
  };
  double acc[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) acc[k] = 0.0;
  double xacc[XMAX];
#pragma unroll
  for (int k = 0; k < XMAX; ++k) xacc[k] = 0.0;
  if (own) ring[row * S + j] = pp_bits(cum);     // h[T] = cum[T] / 256: Be[T] = 0
  double be_next = 0.0, occ = 0.0;               // Be[f + 1][j], occ[f + 1][j]
  float begin_next = 0.0f;                       // begin[f + 1][j]
  __syncthreads();
  for (int f = T - 1; f >= 0; --f) {
    const short* e_f = pc_chunk_row(a, b, f, T, e_l, pc_chunk_start(f + 1) || f == T - 1);   // (descending: a chunk's last frame)
    if (f < T - 1) class_row(f + 1);
    cum -= e_f[jj];                              // cum[f]
    row = pc_ring_prev(row, D);                  // f mod D
    const double lh = length_L(min(D, T - f), row, false, T - f, f == 0);
    if constexpr (LEARN) {
      if (own) vec[j] = lh - pp_bits(cum);
    } else if (own) {
      const float bg =
          pp_owner_step(gw[(long long)f * S + j], lh, alw[(long long)f * S + j], be_next, Z, f == T - 1, occ, begin_next);
      if (a.begin) a.begin[(out_row + f) * S + j] = bg;
      vec[j] = lh - pp_bits(cum);
      lev[j] = fmax(occ, 0.0);
    }
    __syncthreads();
    double hv = 0.0;
    if (f >= 1) {
      be_next = group_L(S, [&](int i) { return pp_bits(tr[jj * S + i]) + vec[i]; });
      hv = be_next + pp_bits(cum);
      if (a.part && f >= 2) {                    // the uncut segments [f - d, f) of this state: f - d >= 1, f <= T - 1
        const int dmax = min(D, f - 1);          // (written out: through pc_for_lengths this loop costs two VGPRs at S <= 16)
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
          if (k * LPS >= dmax) break;
          const int d = 1 + l + k * LPS;
          if (d <= dmax) acc[k] += (double)pp_term(gw[(long long)(f - d) * S + jj] + pp_bits(ln.du[k]) + hv - Z);
        }
      }
      if (own) ring[row * S + j] = hv;
      if constexpr (LEARN) {                     // xi_f[jj][i] of this lane's slots i = l + k LPS
        const double alz = alw[(long long)(f - 1) * S + jj] - Z;
#pragma unroll
        for (int k = 0; k < XMAX; ++k) {
          const int i = l + k * LPS;
          if (i < S) xacc[k] += (double)pp_term((pp_bits(tr[jj * S + i]) + vec[i]) + alz);
        }
      }
    } else if constexpr (LEARN) {                // xi_0: start for Al, the row's sum over ascending j
      if (own && a.start_part) {
        const double stz = (a.init ? pp_bits(pc_clamp_trans(a.init[j])) : 0.0) - Z;
        double s0 = 0.0;
        for (int i = 0; i < S; ++i) s0 += (double)pp_term((pp_bits(tr[j * S + i]) + vec[i]) + stz);
        a.start_part[(long long)b * S + j] = s0;
      }
    }
    if (own && rows_out) {
      const float p = pp_row(lev, S, j);
      pst[j] = p;
      if (a.posterior) a.posterior[(out_row + f) * S + j] = p;
    }
    __syncthreads();
  }
  class_row(0);

  if constexpr (LEARN) {
    if (j < S) {
      double* __restrict__ xp = a.xi_part + ((long long)b * S + j) * S;
#pragma unroll
      for (int k = 0; k < XMAX; ++k)
        if (l + k * LPS < S) xp[l + k * LPS] = xacc[k];
    }
    if (tid == 0) a.z_part[b] = Z;
  }
  if (a.part && j < S) {
    double* __restrict__ part = a.part + ((long long)b * S + j) * D;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (l + k * LPS < D) part[l + k * LPS] = acc[k];
  }
  // rows at and beyond the stream's length are zeros
  for (int idx = T * S + tid; idx < a.T * S; idx += PC_DUR_THREADS) {
    if (a.posterior) a.posterior[out_row * S + idx] = 0.0f;
    if (a.begin) a.begin[out_row * S + idx] = 0.0f;
  }
  if (a.class_posterior)
    for (int idx = T * C + tid; idx < a.T * C; idx += PC_DUR_THREADS) a.class_posterior[out_row * C + idx] = 0.0f;
}

}  // namespace
