// Data gradient of the clip models' first Conv3d (3 -> 32 channels, 3x3x3, pad 1) down to the f32 clip:
//   dx[b][t][c][h][w] = sum over (o, kt, kh, kw) of dy[t - kt + 1][b][h - kh + 1][w - kw + 1][o] * W[o][c][kt][kh][kw]
// with zero outside the clip in t, h and w -- the gradient torch gives `image_sequence.grad` through conv3d_block1[0]
// (/root/reference/3dcnn/models.py:108, reached from Quadtree3DCNN.forward, models.py:189-193) and visual_stream[0][0] of
// Ji3DCNN (/root/reference/cnn+lstm/models.py:99).  dy is [T][B][H][W][32] (what qt_pool3d_bn_bwd_apply writes with
// dy_channels = 32), W the f32 master filter in nn.Conv3d's own layout, dx the clip's layout [B][T][3][H][W], every element
// written exactly once by one thread: no zero fill, no atomics, the same bits on every run.
//
// Fast form (bf16 dy, the shapes qt_conv3d_first_fwd takes): the forward kernel's walk turned round.  A workgroup walks
// the frames of one (clip, 4-row slab, column tile of <= 112 pixels); each dy frame slab -- 6 rows with the row halo, the
// tile's pixels + 1 on either side -- is staged in LDS ONCE and serves the three dx frames it reaches.  One MFMA
// (16x16x32 bf16, f32 accumulation) per (kh, kw) contracts the 32 channels for 16 dx pixels; its 16 rows are
// (kt, c) = 4 kt + c, so lane group kt of the accumulator holds the part of dy frame f that belongs to dx frame f + kt - 1.
// The three parts of a dx frame meet in the accumulator itself: before dy frame f is multiplied, the accumulator moves
// down one lane group (group k takes group k + 1, the last takes zero) and is the MFMA's C input, so that
//   acc_f[k] = S_f[k] + acc_(f-1)[k + 1]   =>   acc_f[0] = S_f[0] + S_(f-1)[1] + S_(f-2)[2] = dx frame f - 1, complete.
// Lane group 0 writes frame f - 1 after dy frame f; after the last dy frame, lane group 1 holds frame T - 1.  The kw shift is
// only an address (lane `li` of tap kw reads staged pixel li + 2 - kw), as in the forward.  The LDS image is
// [row][8-channel group][pixel] x 16 B with pixel planes a multiple of 256 B apart: every ds_read_b128 lane group
// covers 16 distinct 16-byte slots whatever the shift.  The filter is rounded to bf16 in the kernel (the rounding
// qt_pack_conv3d_block applies for the forward) and lives in registers (9 fragments).
// Bound: the dy read (0.8 GB at 32 clips x 8 frames of 224 x 224, 1.5x with the row halo, mostly from L2 / Infinity Cache)
// and the 0.15 GB dx write; 9 MFMAs per 16 pixels and dy frame are ~0.1 ms of matrix pipe for that batch.
//
// General form (every other shape, f32 dy): one thread per dx pixel, 27 x 32 x 3 FMAs in f32 in a fixed order; the filter
// sits in LDS (rounded to bf16 for bf16 dy, as the forward of that build uses it).
#include <atomic>
#include <stdint.h>

#include "qt_common.h"

namespace {

constexpr int D1_R = 4;                 // dx rows per work item, one per wave
constexpr int D1_ROWS = D1_R + 2;       // staged dy rows: h0 - 1 .. h0 + 4
constexpr int D1_MAXBLK = 7;            // 16-pixel blocks per column tile (8 would spill registers)

struct D1Args {
  const bf16_t* dy;       // [T][B][H][W][32]
  const float* w;         // [32][3][3][3][3]
  float* dx;              // [B][T][3][H][W]
  int B, T, H, W;
  int tiles;              // column tiles per row, NB blocks each (the last may reach past W: nothing is written there)
  int items;              // B * (H / 4) * tiles
};

template <int NB>
__global__ __launch_bounds__(256, 2) void conv3d_first_dgrad_kernel(D1Args p) {
  constexpr int NPX = NB * 16 + 2;                       // staged pixels per row: columns c0 - 1 .. c0 + 16 NB
  constexpr int PWB = (NB * 16 + 16) * 16;               // bytes of one (row, channel group) pixel plane: k * 256
  constexpr int NGRP = (D1_ROWS * NPX + 15) / 16;        // groups of 16 staged pixels (x 4 channel groups = 64 lanes)
  constexpr int PER = (NGRP * 64 + 255) / 256;           // 16-byte chunks a thread stages per frame
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lg = lane >> 4;
  const int T = p.T, H = p.H, W = p.W;

  // filter fragments (A operand): MFMA row li = 4 kt + c (rows with kt = 3 or c = 3 are zero), k = output channel lg * 8 + j
  uint4 wf[9];
  {
    const int kt = li >> 2, c = li & 3;
    const bool ok = kt < 3 && c < 3;
#pragma unroll
    for (int s = 0; s < 9; ++s) {          // s = kh * 3 + kw
      bf16x8 e;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int o = lg * 8 + j;
        const int idx = ok ? ((o * 3 + c) * 3 + kt) * 9 + s : 0;
        const float v = p.w[idx];
        e[j] = ok ? (bf16_t)v : (bf16_t)0.f;
      }
      wf[s] = __builtin_bit_cast(uint4, e);
    }
  }

  const int slabs_per_img = H / D1_R;
  const size_t frame = (size_t)p.B * H * W * 32;          // dy elements per frame
  const size_t plane = (size_t)H * W;
  // B operand of tap (kh, kw), block blk: 16 bytes at row wave + 2 - kh, channel group lg, staged pixel blk * 16 + li + 2 - kw
  const unsigned char* bbase = smem + ((wave + 2) * 4 + lg) * PWB + (li + 2) * 16;

  for (int item = blockIdx.x; item < p.items; item += gridDim.x) {
    const int tile = item % p.tiles, rest = item / p.tiles;
    const int b = rest / slabs_per_img, h0 = (rest - b * slabs_per_img) * D1_R;
    const int c0 = tile * NB * 16;

    // staging plan of this item: lane l of chunk group g moves channel group l >> 4 of staged pixel g * 16 + (l & 15)
    int goff[PER], loff[PER];             // element offset inside a (frame, clip) image (-1: zero), LDS byte offset (-1: none)
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int i = tid + k * 256;
      const int pp = (i >> 6) * 16 + (i & 15), q = (i & 63) >> 4;
      const int row = pp / NPX, px = pp - row * NPX;
      const int hh = h0 - 1 + row, ww = c0 - 1 + px;
      const bool slot = pp < D1_ROWS * NPX;
      const bool in = slot && (unsigned)hh < (unsigned)H && (unsigned)ww < (unsigned)W;
      loff[k] = slot ? (row * 4 + q) * PWB + px * 16 : -1;
      goff[k] = in ? (hh * W + ww) * 32 + q * 8 : -1;
    }
    uint4 pre[PER];
    auto load = [&](int f) {
      const bf16_t* src = p.dy + (size_t)f * frame + (size_t)b * plane * 32;
#pragma unroll
      for (int k = 0; k < PER; ++k) {
        pre[k] = make_uint4(0u, 0u, 0u, 0u);
        if (goff[k] >= 0) pre[k] = *reinterpret_cast<const uint4*>(src + goff[k]);
      }
    };

    f32x4 acc[NB];
#pragma unroll
    for (int blk = 0; blk < NB; ++blk) acc[blk] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float* orow = p.dx + ((size_t)b * T * 3) * plane + (size_t)(h0 + wave) * W + c0 + li;

    load(0);
    for (int f = 0; f < T; ++f) {
      __syncthreads();                    // every wave is done with the previous frame slab
#pragma unroll
      for (int k = 0; k < PER; ++k)
        if (loff[k] >= 0) *reinterpret_cast<uint4*>(smem + loff[k]) = pre[k];
      __syncthreads();
      if (f + 1 < T) load(f + 1);         // in flight under the MFMAs below

      // the accumulator moves down one lane group: what frame f - 1 left for dx frames f - 1 and f becomes the C input
#pragma unroll
      for (int blk = 0; blk < NB; ++blk)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float v = __shfl(acc[blk][r], (lane + 16) & 63);
          acc[blk][r] = lg < 3 ? v : 0.f;
        }
#pragma unroll
      for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw)
#pragma unroll
          for (int blk = 0; blk < NB; ++blk) {
            const uint4 d = *reinterpret_cast<const uint4*>(bbase - kh * 4 * PWB - kw * 16 + blk * 256);
            acc[blk] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wf[kh * 3 + kw]),
                                                               __builtin_bit_cast(bf16x8, d), acc[blk], 0, 0, 0);
          }
      // lane group 0 holds dx frame f - 1 (channel r of pixel c0 + 16 blk + li); after the last dy frame group 1 holds frame f
      const int wg = (f >= 1 && lg == 0) ? f - 1 : ((f == T - 1 && lg == 1) ? f : -1);
      if (wg >= 0) {
        float* o = orow + (size_t)wg * 3 * plane;
#pragma unroll
        for (int blk = 0; blk < NB; ++blk)
          if (c0 + blk * 16 < W) {
            o[blk * 16] = acc[blk][0];
            o[plane + blk * 16] = acc[blk][1];
            o[2 * plane + blk * 16] = acc[blk][2];
          }
      }
    }
  }
}

// ---- general form ------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void conv3d_first_dgrad_direct_kernel(const T* __restrict__ dy, const float* __restrict__ w,
                                                                       float* __restrict__ dx, int B, int frames, int H,
                                                                       int W, long long total) {
  __shared__ float ws[27 * 32 * 3];       // [tap = (kt * 3 + kh) * 3 + kw][o][c]
  for (int i = threadIdx.x; i < 27 * 32 * 3; i += 256) {
    const int tap = i / 96, rem = i - tap * 96;
    const int o = rem / 3, c = rem - o * 3;
    float v = w[(o * 3 + c) * 27 + tap];
    if (sizeof(T) == 2) v = (float)(bf16_t)v;   // the filter the bf16 forward multiplied by
    ws[i] = v;
  }
  __syncthreads();
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;   // (b, t, h, w)
  if (idx >= total) return;
  const int x = (int)(idx % W);
  const long long r1 = idx / W;
  const int h = (int)(r1 % H);
  const long long r2 = r1 / H;
  const int t = (int)(r2 % frames), b = (int)(r2 / frames);
  float a0 = 0.f, a1 = 0.f, a2 = 0.f;
  for (int kt = 0; kt < 3; ++kt) {
    const int ft = t - kt + 1;
    if ((unsigned)ft >= (unsigned)frames) continue;
    for (int kh = 0; kh < 3; ++kh) {
      const int hh = h - kh + 1;
      if ((unsigned)hh >= (unsigned)H) continue;
      for (int kw = 0; kw < 3; ++kw) {
        const int xx = x - kw + 1;
        if ((unsigned)xx >= (unsigned)W) continue;
        const T* src = dy + ((((size_t)ft * B + b) * H + hh) * W + xx) * 32;
        const float* wt = ws + ((kt * 3 + kh) * 3 + kw) * 96;
#pragma unroll 8
        for (int o = 0; o < 32; ++o) {
          const float g = (float)src[o];
          a0 += g * wt[o * 3];
          a1 += g * wt[o * 3 + 1];
          a2 += g * wt[o * 3 + 2];
        }
      }
    }
  }
  const size_t plane = (size_t)H * W;
  float* o = dx + ((size_t)(b * frames + t) * 3) * plane + (size_t)h * W + x;
  o[0] = a0;
  o[plane] = a1;
  o[2 * plane] = a2;
}

int d1_grid(int items) {
  static const int cus = [] {
    int dev = 0, n = 256;
    if (hipGetDevice(&dev) == hipSuccess) {
      hipDeviceProp_t pr;
      if (hipGetDeviceProperties(&pr, dev) == hipSuccess && pr.multiProcessorCount > 0) n = pr.multiProcessorCount;
    }
    return n;
  }();
  return items < 2 * cus ? items : 2 * cus;
}

template <int NB>
int d1_launch(D1Args a, hipStream_t s) {
  constexpr int lds = D1_ROWS * 4 * (NB * 16 + 16) * 16;
  static_assert(lds <= 64 * 1024, "two workgroups per CU");
  const int nblk = a.W / 16;
  a.tiles = (nblk + NB - 1) / NB;
  a.items = a.B * (a.H / D1_R) * a.tiles;
  static std::atomic<unsigned long long> done{0};
  if (int rc = qt_raise_lds_limit((const void*)conv3d_first_dgrad_kernel<NB>, lds, done)) return rc;
  hipLaunchKernelGGL(conv3d_first_dgrad_kernel<NB>, dim3(d1_grid(a.items)), dim3(256), lds, s, a);
  QT_CHECK_LAUNCH();
  return QT_OK;
}

template <typename T>
int d1_launch_direct(const void* dy, const float* w, float* dx, int B, int frames, int H, int W, hipStream_t s) {
  const long long total = (long long)B * frames * H * W;
  const long long blocks = (total + 255) / 256;
  if (blocks > 0x7fffffffLL) {
    qt_set_error("qt_conv3d_first_dgrad: %lld pixels are more than one launch covers", total);
    return QT_ERR_INVALID_ARG;
  }
  hipLaunchKernelGGL(conv3d_first_dgrad_direct_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, s, static_cast<const T*>(dy), w,
                     dx, B, frames, H, W, total);
  QT_CHECK_LAUNCH();
  return QT_OK;
}

}  // namespace

extern "C" int qt_conv3d_first_dgrad(int dtype, const void* dy, const float* w_oidhw, float* dclips, int batch, int frames,
                                     int h, int w, void* stream) {
  QT_CHECK_ARG(dy && w_oidhw && dclips && batch > 0 && frames > 0 && h > 0 && w > 0, "qt_conv3d_first_dgrad: bad argument");
  if (dtype != QT_BF16 && dtype != QT_F32) {
    qt_set_error("qt_conv3d_first_dgrad: dtype %d (bf16 or f32 dy only)", dtype);
    return QT_ERR_UNSUPPORTED;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  // (a dtype branch: f32 has the direct kernel only, the staged kernel below is bf16)
  if (dtype == QT_F32) return d1_launch_direct<float>(dy, w_oidhw, dclips, batch, frames, h, w, s);
  // (the staging plan keeps 32-bit element offsets inside one image)
  const bool fast = h % D1_R == 0 && w % 16 == 0 && w <= 256 && ((uintptr_t)dy % 16) == 0 && (long long)h * w * 32 < (1LL << 31);
  if (!fast) return d1_launch_direct<bf16_t>(dy, w_oidhw, dclips, batch, frames, h, w, s);
  D1Args a;
  a.dy = static_cast<const bf16_t*>(dy); a.w = w_oidhw; a.dx = dclips;
  a.B = batch; a.T = frames; a.H = h; a.W = w; a.tiles = 0; a.items = 0;
  // balanced column tiles of at most D1_MAXBLK blocks: 224 pixels = 2 x 7 blocks, 256 = 3 x 6 (the last tile two blocks short)
  const int nblk = w / 16, tiles = (nblk + D1_MAXBLK - 1) / D1_MAXBLK;
  switch ((nblk + tiles - 1) / tiles) {
    case 1: return d1_launch<1>(a, s);
    case 2: return d1_launch<2>(a, s);
    case 3: return d1_launch<3>(a, s);
    case 4: return d1_launch<4>(a, s);
    case 5: return d1_launch<5>(a, s);
    case 6: return d1_launch<6>(a, s);
    default: return d1_launch<7>(a, s);
  }
}
