// The 2-layer LSTM of the CNN+LSTM sequence model (/root/reference/cnn+lstm/models.py:43-49,81-86) on a video STREAM:
// one row of h1 per frame, from the window of the last T frames, eval arithmetic, f32 (the rule: include/qtcnn.h).
//
// A frame's layer-0 input product does not depend on the window it is read through, so it exists once
// (xproj0 [S][T-1+n][4H]) and a window is an addressing rule: window f of a call reads rows f .. f+T-1.  What belongs to
// a window is the recurrence: T dependent steps through both layers.  ONE launch runs it for all S*n windows:
//   * a workgroup owns QT_LSTM_STREAM_TILE consecutive windows of one stream and walks them in lockstep, END-aligned:
//     at step j window w reads row f0 + w + j; a window shorter than T (the first T-1 frames of a stream) stays at its
//     zero state until step T - len and never reads the rows in front of the stream's start;
//   * H threads; thread `tid` owns the four gate columns 4*tid .. 4*tid+3 (one float4 stream over each transposed
//     weight matrix, read ONCE per step for the whole tile) and, for the cell arithmetic, unit `tid` of every window;
//     h0 / h1 of the tile live in LDS and are read as broadcast float4, the activations cross threads through LDS;
//   * layer 1's input product h0_t W_ih1^T is formed in the same step, so nothing of size windows x T exists anywhere;
//   * every accumulator is one k-ordered fmaf chain, written per window: a window's bits do not depend on its slot,
//     its neighbours, n or S.  No atomics, no workspace, no zero fill.
// The last workgroups of the grid copy the carry (the last T-1 rows of xproj0) for the next call.
// Budget at H = 256, tile 8: LDS 2*8*256*4 (h0, h1) + 8*1024*4 (activations) = 48 KB and 150 VGPRs (32 accumulators, 32
// weights of two unrolled k-steps, 24 of state) -> 3 workgroups of 4 waves per CU, no scratch.  A step is
// 3*H*4H*tile = 6.3 M fmaf against 3 MB of weights from L2: at 8 windows both cost about 20 us on one CU, so the tile is
// FMA-issue bound and the other workgroups' arithmetic covers a workgroup's weight loads.
#include "qt_common.h"

namespace {

constexpr int TILE = QT_LSTM_STREAM_TILE;
// The kernel is instantiated for W = TILE window slots per workgroup and, for the live step of ONE frame per stream
// (n == 1), for W = 1: the same chains per window, nothing computed for seven slots that hold no window.

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + __expf(-x)); }

// acc[w][0..3] += sum_m h[w][m] * wT[m][4*tid + q], m ascending, one fmaf per term.  h: LDS [W][H].
template <int H, int W>
__device__ __forceinline__ void tile_product(float (&acc)[W][4], const float* __restrict__ wT, const float* h, int tid) {
  const float4* w4 = reinterpret_cast<const float4*>(wT) + tid;  // row m: w4[m * H]
#pragma unroll 2
  for (int m = 0; m < H; m += 4) {
    const float4 r0 = w4[(m + 0) * H], r1 = w4[(m + 1) * H], r2 = w4[(m + 2) * H], r3 = w4[(m + 3) * H];
#pragma unroll
    for (int w = 0; w < W; ++w) {
      const float4 x = *reinterpret_cast<const float4*>(h + w * H + m);
      acc[w][0] = fmaf(x.x, r0.x, acc[w][0]); acc[w][1] = fmaf(x.x, r0.y, acc[w][1]);
      acc[w][2] = fmaf(x.x, r0.z, acc[w][2]); acc[w][3] = fmaf(x.x, r0.w, acc[w][3]);
      acc[w][0] = fmaf(x.y, r1.x, acc[w][0]); acc[w][1] = fmaf(x.y, r1.y, acc[w][1]);
      acc[w][2] = fmaf(x.y, r1.z, acc[w][2]); acc[w][3] = fmaf(x.y, r1.w, acc[w][3]);
      acc[w][0] = fmaf(x.z, r2.x, acc[w][0]); acc[w][1] = fmaf(x.z, r2.y, acc[w][1]);
      acc[w][2] = fmaf(x.z, r2.z, acc[w][2]); acc[w][3] = fmaf(x.z, r2.w, acc[w][3]);
      acc[w][0] = fmaf(x.w, r3.x, acc[w][0]); acc[w][1] = fmaf(x.w, r3.y, acc[w][1]);
      acc[w][2] = fmaf(x.w, r3.z, acc[w][2]); acc[w][3] = fmaf(x.w, r3.w, acc[w][3]);
    }
  }
}

// post-activation gates of the tile -> LDS act [W][4H]; columns 4*tid.. lie in ONE gate block (H % 4 == 0)
template <int H, int W>
__device__ __forceinline__ void tile_activate(const float (&acc)[W][4], float* act, int tid) {
  const bool is_g = 4 * tid >= 2 * H && 4 * tid < 3 * H;
#pragma unroll
  for (int w = 0; w < W; ++w) {
    float4 a;
    a.x = is_g ? tanhf(acc[w][0]) : sigmoidf_(acc[w][0]);
    a.y = is_g ? tanhf(acc[w][1]) : sigmoidf_(acc[w][1]);
    a.z = is_g ? tanhf(acc[w][2]) : sigmoidf_(acc[w][2]);
    a.w = is_g ? tanhf(acc[w][3]) : sigmoidf_(acc[w][3]);
    *reinterpret_cast<float4*>(act + w * 4 * H + 4 * tid) = a;
  }
}

template <int H, int W>
__global__ __launch_bounds__(H, 3) void lstm_stream_kernel(const float* __restrict__ xproj0, const float* __restrict__ whh0T,
                                                        const float* __restrict__ bhh0, const float* __restrict__ wih1T,
                                                        const float* __restrict__ bih1, const float* __restrict__ whh1T,
                                                        const float* __restrict__ bhh1, float* __restrict__ hlast,
                                                        float* __restrict__ carry_out, long long seen, int n, int T,
                                                        int tiles, int recurrence_blocks) {
  const int tid = threadIdx.x;
  const long long rows = (long long)T - 1 + n;  // rows of xproj0 per stream
  if ((int)blockIdx.x >= recurrence_blocks) {
    // ---- carry: row k of the next call's carry is row n + k of this call's buffer; a row in front of the stream's start
    //      (global frame seen + n - (T-1) + k < 0) is never read, here or later, and is handed on as zeros ----
    const int s = blockIdx.x - recurrence_blocks;
    const float4* src = reinterpret_cast<const float4*>(xproj0 + ((long long)s * rows + n) * 4 * H);
    float4* dst = reinterpret_cast<float4*>(carry_out + (long long)s * (T - 1) * 4 * H);
    for (int k = 0; k < T - 1; ++k) {
      const bool real = seen + n - (T - 1) + k >= 0;
      dst[(long long)k * H + tid] = real ? src[(long long)k * H + tid] : make_float4(0.f, 0.f, 0.f, 0.f);  // H float4 per row
    }
    return;
  }
  __shared__ __attribute__((aligned(16))) float sh0[W * H];
  __shared__ __attribute__((aligned(16))) float sh1[W * H];
  __shared__ __attribute__((aligned(16))) float act[W * 4 * H];
  const int s = blockIdx.x / tiles, f0 = (blockIdx.x % tiles) * W;
  const int nw = n - f0 < W ? n - f0 : W;  // windows of this tile (the first nw slots)
  // window w = frame f0 + w, global index g = seen + f0 + w, len = min(T, g + 1): active from step T - len on
  int first[W];
#pragma unroll
  for (int w = 0; w < W; ++w) {
    const long long g = seen + f0 + w;
    first[w] = g + 1 >= T ? 0 : T - (int)(g + 1);
  }
  float c0[W], c1[W], h1[W];
#pragma unroll
  for (int w = 0; w < W; ++w) {
    c0[w] = c1[w] = h1[w] = 0.f;
    sh0[w * H + tid] = 0.f;
    sh1[w * H + tid] = 0.f;
  }
  const float4 b0 = reinterpret_cast<const float4*>(bhh0)[tid];
  const float4 bi1 = reinterpret_cast<const float4*>(bih1)[tid];
  const float4 bh1 = reinterpret_cast<const float4*>(bhh1)[tid];
  const float* xs = xproj0 + (long long)s * rows * 4 * H;
  __syncthreads();
  float acc[W][4];
  for (int j = 0; j < T; ++j) {
    // ---- layer 0: gates = (xproj0 row + b_hh0) + h0 W_hh0^T ----
#pragma unroll
    for (int w = 0; w < W; ++w) {
      float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
      if (w < nw && j >= first[w]) x = reinterpret_cast<const float4*>(xs + ((long long)f0 + w + j) * 4 * H)[tid];
      acc[w][0] = x.x + b0.x; acc[w][1] = x.y + b0.y; acc[w][2] = x.z + b0.z; acc[w][3] = x.w + b0.w;
    }
    tile_product<H, W>(acc, whh0T, sh0, tid);
    tile_activate<H, W>(acc, act, tid);
    __syncthreads();  // activations complete; every read of sh0 of this step is done
#pragma unroll
    for (int w = 0; w < W; ++w) {
      if (w < nw && j >= first[w]) {
        const float gi = act[w * 4 * H + tid], gf = act[w * 4 * H + H + tid], gg = act[w * 4 * H + 2 * H + tid],
                    go = act[w * 4 * H + 3 * H + tid];
        c0[w] = fmaf(gf, c0[w], gi * gg);
        sh0[w * H + tid] = go * tanhf(c0[w]);
      }
    }
    __syncthreads();  // h0_t of the tile is in LDS; act may be rewritten
    // ---- layer 1: gates = (b_ih1 + b_hh1) + h0_t W_ih1^T + h1 W_hh1^T ----
#pragma unroll
    for (int w = 0; w < W; ++w) {
      acc[w][0] = bi1.x + bh1.x; acc[w][1] = bi1.y + bh1.y; acc[w][2] = bi1.z + bh1.z; acc[w][3] = bi1.w + bh1.w;
    }
    tile_product<H, W>(acc, wih1T, sh0, tid);
    tile_product<H, W>(acc, whh1T, sh1, tid);
    tile_activate<H, W>(acc, act, tid);
    __syncthreads();  // activations complete; every read of sh1 of this step is done
#pragma unroll
    for (int w = 0; w < W; ++w) {
      if (w < nw && j >= first[w]) {
        const float gi = act[w * 4 * H + tid], gf = act[w * 4 * H + H + tid], gg = act[w * 4 * H + 2 * H + tid],
                    go = act[w * 4 * H + 3 * H + tid];
        c1[w] = fmaf(gf, c1[w], gi * gg);
        h1[w] = go * tanhf(c1[w]);
        sh1[w * H + tid] = h1[w];
      }
    }
    __syncthreads();  // h1_t is in LDS; act may be rewritten by the next step
  }
#pragma unroll
  for (int w = 0; w < W; ++w)
    if (w < nw) hlast[((long long)s * n + f0 + w) * H + tid] = h1[w];
}

// xproj0 [S][T-1+n][4H] <- carry_in [S][T-1][4H] (rows 0 .. T-2) and xnew [S][n][4H] (rows T-1 ..)
__global__ void lstm_stream_stage_kernel(const float4* __restrict__ carry_in, const float4* __restrict__ xnew,
                                         float4* __restrict__ xproj0, int n, int T, int H, long long total) {
  const long long rows = (long long)T - 1 + n;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long row = i / H, s = row / rows, r = row % rows;
    const int c = (int)(i % H);
    xproj0[i] = r < T - 1 ? carry_in[(s * (T - 1) + r) * H + c] : xnew[(s * n + (r - (T - 1))) * H + c];
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the shapes the kernel is instantiated for; everything else is refused before any launch
int check_shape(const char* who, int S, int n, int T, int H) {
  QT_CHECK_ARG(S > 0 && n > 0, "%s: streams (%d) and frames per call (%d) must be positive", who, S, n);
  if (H != 256 && H != 64) {
    qt_set_error("%s: hidden size %d is not instantiated (256, 64)", who, H);
    return QT_ERR_UNSUPPORTED;
  }
  if (T < 1 || T > 64) {
    qt_set_error("%s: window of %d frames is outside 1 .. 64", who, T);
    return QT_ERR_UNSUPPORTED;
  }
  return QT_OK;
}

}  // namespace

extern "C" size_t qt_lstm_stream_workspace_bytes(int S, int n, int T, int H) {
  (void)S; (void)n; (void)T; (void)H;
  return 0;  // both layers and every window's state stay in registers / LDS
}

extern "C" int qt_lstm_stream_forward(const float* xproj0, const float* whh0_t, const float* bhh0, const float* wih1_t,
                                      const float* bih1, const float* whh1_t, const float* bhh1, float* hlast,
                                      float* carry_out, void* workspace, size_t workspace_bytes, long long seen, int S,
                                      int n, int T, int H, void* stream) {
  (void)workspace;
  const int st = check_shape("qt_lstm_stream_forward", S, n, T, H);
  if (st != QT_OK) return st;
  QT_CHECK_ARG(xproj0 && whh0_t && bhh0 && wih1_t && bih1 && whh1_t && bhh1 && hlast, "qt_lstm_stream_forward: null argument");
  QT_CHECK_ARG(seen >= 0, "qt_lstm_stream_forward: seen (%lld) must not be negative", seen);
  QT_CHECK_ARG(workspace_bytes >= qt_lstm_stream_workspace_bytes(S, n, T, H), "qt_lstm_stream_forward: workspace too small");
  QT_CHECK_ARG(carry_out != xproj0, "qt_lstm_stream_forward: carry_out must not alias xproj0 (swap two buffers)");
  QT_CHECK_ARG(aligned16(xproj0) && aligned16(whh0_t) && aligned16(bhh0) && aligned16(wih1_t) && aligned16(bih1) &&
                   aligned16(whh1_t) && aligned16(bhh1) && aligned16(carry_out),
               "qt_lstm_stream_forward: xproj0, the weights, the biases and carry_out must be 16-byte aligned");
  const int W = n == 1 ? 1 : TILE, tiles = qt_cdiv(n, W);
  const long long blocks = (long long)S * tiles, carry_blocks = carry_out && T > 1 ? S : 0;
  QT_CHECK_ARG(blocks + carry_blocks <= 0x7fffffffLL, "qt_lstm_stream_forward: %lld windows are too many for one launch",
               (long long)S * n);
  hipStream_t hs = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)(blocks + carry_blocks));
  auto launch = [&](auto kernel, int threads) {
    hipLaunchKernelGGL(kernel, grid, dim3(threads), 0, hs, xproj0, whh0_t, bhh0, wih1_t, bih1, whh1_t, bhh1, hlast, carry_out,
                       seen, n, T, tiles, (int)blocks);
  };
  if (H == 256 && W == TILE) launch(lstm_stream_kernel<256, TILE>, 256);
  else if (H == 256) launch(lstm_stream_kernel<256, 1>, 256);
  else if (W == TILE) launch(lstm_stream_kernel<64, TILE>, 64);
  else launch(lstm_stream_kernel<64, 1>, 64);
  QT_CHECK_LAUNCH();
  return QT_OK;
}

extern "C" int qt_lstm_stream_stage(const float* carry_in, const float* xnew, float* xproj0, int S, int n, int T, int H,
                                    void* stream) {
  const int st = check_shape("qt_lstm_stream_stage", S, n, T, H);
  if (st != QT_OK) return st;
  QT_CHECK_ARG(xnew && xproj0 && (carry_in || T == 1), "qt_lstm_stream_stage: null argument");
  QT_CHECK_ARG(aligned16(carry_in) && aligned16(xnew) && aligned16(xproj0), "qt_lstm_stream_stage: buffers must be 16-byte aligned");
  const long long total = (long long)S * ((long long)T - 1 + n) * H;  // float4 elements
  hipLaunchKernelGGL(lstm_stream_stage_kernel, dim3(qt_grid_for(total, 256, 8192)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), reinterpret_cast<const float4*>(carry_in),
                     reinterpret_cast<const float4*>(xnew), reinterpret_cast<float4*>(xproj0), n, T, H, total);
  QT_CHECK_LAUNCH();
  return QT_OK;
}
