// Frame preprocessing on the device (qt_preprocess_u8): uint8 HWC frames -> the f32 NCHW tensor every model here takes.
// Per image: crop box, left-right flip, antialiased bilinear resize (torch's interpolate(mode='bilinear', antialias=True),
// which is what transforms.Resize / RandomResizedCrop compute, without PIL's uint8 rounding between the passes), /255,
// (v - mean) * inv_std.  The reference's loaders do all of it per image on a CPU core (Resize -> ToTensor -> Normalize).
//
// One launch.  A workgroup owns a 16-row x 64-column tile of one image's output, all three channels:
//   1. it reads the image's box and flip from device memory; a box that is not inside the frame makes the tile NaN and
//      nothing of the frame is read;
//   2. threads 0..63 form the normalised column weights of their column, threads 64..79 the row weights, in LDS.  With
//      center * 2 out = in (2i + 1) both window ends and every raw weight are exact integers:
//          lo = floor((in (2i+1) - 2 max(in,out) + out) / (2 out)),  hi = floor((in (2i+1) + 2 max(in,out) + out) / (2 out)),
//          m_j = max(0, 2 max(in,out) - |2 out j + out - in (2i+1)|),   w_j = float(m_j) / float(sum_j m_j)
//      (the same numbers as max(0, 1 - |(j - center + 0.5) / support|) divided by their sum), so no tap set depends on f32
//      rounding and a weight carries two roundings;
//   3. the source rows the tile needs pass through LDS eight at a time: staged as bytes (aligned dwords inside the
//      needed span, single bytes at its ends: nothing outside the box is read), resampled horizontally into f32 rows in
//      LDS, and added into the 12 accumulators (4 rows x 3 channels) each thread keeps, in ascending row order;
//   4. the normalised tile goes through LDS once more so that output rows leave as 16-byte stores with scalar ends.
// No intermediate in HBM, no atomics, no zero fill, every summation order fixed: the same bits on every run.
#include <math.h>
#include <stdint.h>

#include "qt_common.h"

namespace {

constexpr int PP_THREADS = 256;
constexpr int PP_TW = 64;          // output columns per tile = lanes of a wave
constexpr int PP_TH = 16;          // output rows per tile, four per wave
constexpr int PP_R = 8;            // source rows per pass through LDS, two per wave
constexpr int PP_MAX_SCALE = 24;   // largest per-axis downscale (frame size / output size)
constexpr int PP_MAX_DIM = 1 << 22;   // 2 max(in, out) and every raw weight stay exact in f32
constexpr int PP_MAX_LDS = 64 * 1024;
constexpr int PP_OUT_BYTES = 3 * PP_TH * PP_TW * 4;

struct PreArgs {
  const unsigned char* src;
  const int* boxes;
  const unsigned char* flips;
  float* dst;
  long long src_row_stride, src_image_stride, dst_image_stride;
  int src_h, src_w, out_h, out_w, bgr;
  int tiles_x, tiles_y;
  int kx, ky;      // taps reserved per column / per row
  int pitch;       // bytes per staged source row (a multiple of 4)
  float scale[3], shift[3];   // out = v * scale + shift = (v / 255 - mean) * inv_std
};

__device__ __forceinline__ long long floordiv(long long a, long long b) {   // b > 0
  const long long q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}

// Window and normalised weights of output index i on an axis of crop length `in` and output length `out`.
// w[k * stride], k < *n, belongs to crop index *lo + k.
__device__ __forceinline__ void axis_weights(int i, int in, int out, float* w, int stride, int kmax, int* lo_out, int* n_out) {
  const long long c2 = (long long)in * (2 * i + 1);
  const long long sup2 = 2LL * (in > out ? in : out);
  long long lo = floordiv(c2 - sup2 + out, 2LL * out);
  long long hi = floordiv(c2 + sup2 + out, 2LL * out);
  if (lo < 0) lo = 0;
  if (hi > in) hi = in;
  int n = (int)(hi - lo);
  if (n > kmax) n = kmax;   // never taken: kmax is the launcher's bound for every box inside the frame
  long long M = 0;
  for (int k = 0; k < n; ++k) {
    long long d = 2LL * out * (lo + k) + out - c2;
    if (d < 0) d = -d;
    long long m = sup2 - d;
    if (m < 0) m = 0;
    M += m;
    w[k * stride] = (float)m;
  }
  const float fM = (float)M;
  for (int k = 0; k < n; ++k) w[k * stride] = w[k * stride] / fM;
  *lo_out = (int)lo;
  *n_out = n;
}

__global__ __launch_bounds__(PP_THREADS) void preprocess_u8_kernel(PreArgs a) {
  extern __shared__ __align__(16) unsigned char pp_smem[];
  float* wx = reinterpret_cast<float*>(pp_smem);   // [kx][64]
  float* wy = wx + a.kx * PP_TW;                   // [ky][16]
  float* H = wy + a.ky * PP_TH;                    // [R][3][64] horizontally resampled rows
  int* xlo = reinterpret_cast<int*>(H + PP_R * 3 * PP_TW);
  int* xn = xlo + PP_TW;
  int* ylo = xn + PP_TW;
  int* yn = ylo + PP_TH;
  unsigned char* stage = reinterpret_cast<unsigned char*>(yn + PP_TH);   // [R][pitch] source bytes, later the output tile

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int bid = blockIdx.x;
  const int tx = bid % a.tiles_x;
  const int ty = (bid / a.tiles_x) % a.tiles_y;
  const long long b = bid / (a.tiles_x * a.tiles_y);
  const int p0 = tx * PP_TW, oy0 = ty * PP_TH;
  const int ntw = min(PP_TW, a.out_w - p0), nth = min(PP_TH, a.out_h - oy0);
  float* __restrict__ dimg = a.dst + b * a.dst_image_stride;
  const long long plane = (long long)a.out_h * a.out_w;

  int top = 0, left = 0, bh = a.src_h, bw = a.src_w;
  if (a.boxes) {
    top = a.boxes[4 * b + 0];
    left = a.boxes[4 * b + 1];
    bh = a.boxes[4 * b + 2];
    bw = a.boxes[4 * b + 3];
  }
  const bool flip = a.flips && a.flips[b] != 0;
  const bool valid = top >= 0 && left >= 0 && bh >= 1 && bw >= 1 && (long long)top + bh <= a.src_h && (long long)left + bw <= a.src_w;
  if (!valid) {   // the same for every thread of the workgroup
    const float nan = __uint_as_float(0x7fc00000u);
    for (int e = tid; e < 3 * nth * ntw; e += PP_THREADS) {
      const int c = e / (nth * ntw), rem = e % (nth * ntw);
      dimg[c * plane + (long long)(oy0 + rem / ntw) * a.out_w + p0 + rem % ntw] = nan;
    }
    return;
  }

  if (tid < ntw) {
    const int p = p0 + tid;
    axis_weights(flip ? a.out_w - 1 - p : p, bw, a.out_w, wx + tid, PP_TW, a.kx, &xlo[tid], &xn[tid]);
  } else if (tid >= PP_TW && tid < PP_TW + nth) {
    const int q = tid - PP_TW;
    axis_weights(oy0 + q, bh, a.out_h, wy + q, PP_TH, a.ky, &ylo[q], &yn[q]);
  }
  __syncthreads();

  // the span of crop columns / rows the tile reads (window ends are monotone in the output index)
  const int xa = flip ? xlo[ntw - 1] : xlo[0];
  const int xb = flip ? xlo[0] + xn[0] : xlo[ntw - 1] + xn[ntw - 1];
  int nbytes = 3 * (xb - xa);
  if (nbytes > a.pitch - 4) nbytes = a.pitch - 4;   // never taken (launcher's bound), keeps LDS writes inside a row
  const int ya = ylo[0], yb = ylo[nth - 1] + yn[nth - 1];
  const int my_x = lane < ntw ? 3 * (xlo[lane] - xa) : 0;
  const int my_xn = lane < ntw ? xn[lane] : 0;
  int my_ylo[4], my_yn[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = wv * 4 + q;
    my_ylo[q] = r < nth ? ylo[r] : 0;
    my_yn[q] = r < nth ? yn[r] : 0;
  }
  const int c0 = a.bgr ? 2 : 0, c2 = a.bgr ? 0 : 2;   // source byte of output channels R and B
  const unsigned char* __restrict__ base = a.src + b * a.src_image_stride + (long long)top * a.src_row_stride + 3LL * (left + xa);

  float acc[4][3];
#pragma unroll
  for (int q = 0; q < 4; ++q) acc[q][0] = acc[q][1] = acc[q][2] = 0.f;

  for (int rs = ya; rs < yb; rs += PP_R) {
    // stage: wave wv brings rows rs + wv and rs + wv + 4
    for (int rl = wv; rl < PP_R; rl += 4) {
      const int r = rs + rl;
      if (r >= yb) break;
      const unsigned char* __restrict__ rowp = base + (long long)r * a.src_row_stride;
      const int sh = (int)(reinterpret_cast<uintptr_t>(rowp) & 3);
      const int ndw = (sh + nbytes + 3) >> 2;
      unsigned* __restrict__ srow = reinterpret_cast<unsigned*>(stage + rl * a.pitch);
      for (int d = lane; d < ndw; d += 64) {
        const int off = 4 * d - sh;   // of the dword's first byte inside the span
        unsigned v;
        if (off >= 0 && off + 4 <= nbytes) {
          v = *reinterpret_cast<const unsigned*>(rowp + off);
        } else {
          v = 0;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int o = off + e;
            if (o >= 0 && o < nbytes) v |= (unsigned)rowp[o] << (8 * e);
          }
        }
        srow[d] = v;
      }
    }
    __syncthreads();
    // horizontal pass: lane = output column, wave wv resamples its two rows with one read of each weight
    {
      const int r0 = rs + wv, r1 = r0 + 4;
      if (r0 < yb && lane < ntw) {
        const bool two = r1 < yb;
        const int sh0 = (int)(reinterpret_cast<uintptr_t>(base + (long long)r0 * a.src_row_stride) & 3);
        const int sh1 = (int)(reinterpret_cast<uintptr_t>(base + (long long)r1 * a.src_row_stride) & 3);
        const unsigned char* s0 = stage + wv * a.pitch + sh0 + my_x;
        const unsigned char* s1 = two ? stage + (wv + 4) * a.pitch + sh1 + my_x : s0;
        float h0[3] = {0.f, 0.f, 0.f}, h1[3] = {0.f, 0.f, 0.f};
        for (int k = 0; k < my_xn; ++k) {
          const float w = wx[k * PP_TW + lane];
          h0[0] = fmaf(w, (float)s0[3 * k + c0], h0[0]);
          h0[1] = fmaf(w, (float)s0[3 * k + 1], h0[1]);
          h0[2] = fmaf(w, (float)s0[3 * k + c2], h0[2]);
          h1[0] = fmaf(w, (float)s1[3 * k + c0], h1[0]);
          h1[1] = fmaf(w, (float)s1[3 * k + 1], h1[1]);
          h1[2] = fmaf(w, (float)s1[3 * k + c2], h1[2]);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          H[(wv * 3 + c) * PP_TW + lane] = h0[c];
          if (two) H[((wv + 4) * 3 + c) * PP_TW + lane] = h1[c];
        }
      }
    }
    __syncthreads();
    // vertical pass: wave wv owns output rows 4 wv .. 4 wv + 3 of the tile
    for (int rl = 0; rl < PP_R; ++rl) {
      const int r = rs + rl;
      if (r >= yb) break;
      const float h0 = H[(rl * 3 + 0) * PP_TW + lane], h1 = H[(rl * 3 + 1) * PP_TW + lane], h2 = H[(rl * 3 + 2) * PP_TW + lane];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int k = r - my_ylo[q];
        if (k >= 0 && k < my_yn[q]) {
          const float w = wy[k * PP_TH + wv * 4 + q];
          acc[q][0] = fmaf(w, h0, acc[q][0]);
          acc[q][1] = fmaf(w, h1, acc[q][1]);
          acc[q][2] = fmaf(w, h2, acc[q][2]);
        }
      }
    }
    // the next pass's first barrier stands between these reads of H and its next writes
  }

  // the staging rows were last read before the loop's second barrier: they now hold the output tile [3][16][64]
  float* O = reinterpret_cast<float*>(stage);
  if (lane < ntw) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (wv * 4 + q < nth) {
#pragma unroll
        for (int c = 0; c < 3; ++c) O[(c * PP_TH + wv * 4 + q) * PP_TW + lane] = fmaf(acc[q][c], a.scale[c], a.shift[c]);
      }
    }
  }
  __syncthreads();
  // 16 lanes per output row segment: scalar stores up to the first 16-byte boundary, float4 stores, scalar tail
  const int j = tid & 15;
  for (int s = tid >> 4; s < 3 * nth; s += PP_THREADS / 16) {
    const int c = s / nth, row = s % nth;
    float* __restrict__ drow = dimg + c * plane + (long long)(oy0 + row) * a.out_w + p0;
    const float* __restrict__ orow = O + (c * PP_TH + row) * PP_TW;
    int head = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(drow) & 15u)) & 15u) >> 2);
    if (head > ntw) head = ntw;
    const int groups = (ntw - head) >> 2;   // <= 16
    const int tail0 = head + 4 * groups;
    if (j < head) drow[j] = orow[j];
    if (j < groups) {
      const float* o4 = orow + head + 4 * j;
      *reinterpret_cast<float4*>(drow + head + 4 * j) = make_float4(o4[0], o4[1], o4[2], o4[3]);
    }
    if (j < ntw - tail0) drow[tail0 + j] = orow[tail0 + j];
  }
}

// taps one output index can have on an axis whose crop is at most `src` long: floor(2 support) + 1 with
// support = max(in / out, 1) <= ceil(max(src, out) / out), and never more than the crop itself
inline int max_taps(int src, int out) {
  const int big = src > out ? src : out;
  const long long t = 2LL * ((big + out - 1) / out) + 1;
  return (int)(t < src ? t : src);
}

}  // namespace

extern "C" int qt_preprocess_u8(const qt_preprocess_desc* d, const unsigned char* src, const int* boxes, const unsigned char* flips,
                                float* dst, long long dst_image_stride, void* stream) {
  QT_CHECK_ARG(d, "qt_preprocess_u8: null descriptor");
  QT_CHECK_ARG(d->batch >= 1 && d->src_h >= 1 && d->src_w >= 1 && d->out_h >= 1 && d->out_w >= 1,
               "qt_preprocess_u8: sizes must be positive (batch %d, source %d x %d, output %d x %d)", d->batch, d->src_h, d->src_w,
               d->out_h, d->out_w);
  QT_CHECK_ARG(d->bgr == 0 || d->bgr == 1, "qt_preprocess_u8: bgr must be 0 or 1 (got %d)", d->bgr);
  if (d->src_h > PP_MAX_DIM || d->src_w > PP_MAX_DIM || d->out_h > PP_MAX_DIM || d->out_w > PP_MAX_DIM) {
    qt_set_error("qt_preprocess_u8: source %d x %d -> output %d x %d: at most %d lines or columns are handled", d->src_h, d->src_w,
                 d->out_h, d->out_w, PP_MAX_DIM);
    return QT_ERR_UNSUPPORTED;
  }
  QT_CHECK_ARG(d->src_row_stride >= 3LL * d->src_w, "qt_preprocess_u8: source row stride %lld < 3 * src_w = %lld bytes",
               d->src_row_stride, 3LL * d->src_w);
  QT_CHECK_ARG(d->src_image_stride / d->src_h >= d->src_row_stride,
               "qt_preprocess_u8: source image stride %lld < src_h * row stride = %d * %lld bytes", d->src_image_stride, d->src_h,
               d->src_row_stride);
  QT_CHECK_ARG(dst_image_stride >= 3LL * d->out_h * d->out_w, "qt_preprocess_u8: destination image stride %lld < 3 * out_h * out_w = %lld",
               dst_image_stride, 3LL * d->out_h * d->out_w);
  QT_CHECK_ARG(src && dst, "qt_preprocess_u8: null source / destination");
  QT_CHECK_ARG((reinterpret_cast<uintptr_t>(dst) & 3) == 0 && (reinterpret_cast<uintptr_t>(boxes) & 3) == 0,
               "qt_preprocess_u8: destination and boxes must be 4-byte aligned");
  for (int c = 0; c < 3; ++c)
    QT_CHECK_ARG(isfinite(d->mean[c]) && isfinite(d->inv_std[c]), "qt_preprocess_u8: mean / inv_std of channel %d is not finite", c);
  if (d->src_h > (long long)PP_MAX_SCALE * d->out_h || d->src_w > (long long)PP_MAX_SCALE * d->out_w) {
    qt_set_error("qt_preprocess_u8: downscale limit: source %d x %d -> output %d x %d is more than %d x on an axis", d->src_h, d->src_w,
                 d->out_h, d->out_w, PP_MAX_SCALE);
    return QT_ERR_UNSUPPORTED;
  }
  PreArgs a;
  a.src = src;
  a.boxes = boxes;
  a.flips = flips;
  a.dst = dst;
  a.src_row_stride = d->src_row_stride;
  a.src_image_stride = d->src_image_stride;
  a.dst_image_stride = dst_image_stride;
  a.src_h = d->src_h;
  a.src_w = d->src_w;
  a.out_h = d->out_h;
  a.out_w = d->out_w;
  a.bgr = d->bgr;
  a.tiles_x = qt_cdiv(d->out_w, PP_TW);
  a.tiles_y = qt_cdiv(d->out_h, PP_TH);
  a.kx = max_taps(d->src_w, d->out_w);
  a.ky = max_taps(d->src_h, d->out_h);
  // crop columns under one tile: floor(scale (64 - 1) + 2 support) + 1 with scale <= src_w / out_w
  const int big_w = d->src_w > d->out_w ? d->src_w : d->out_w;
  long long cols = (long long)d->src_w * (PP_TW - 1) / d->out_w + 2LL * ((big_w + d->out_w - 1) / d->out_w) + 1;
  if (cols > d->src_w) cols = d->src_w;
  a.pitch = (int)((3 * cols + 3 + 3) & ~3LL) + 4;   // up to 3 bytes in front of an unaligned row; + 4: rows start on different banks
  const long long stage_bytes = (long long)PP_R * a.pitch > PP_OUT_BYTES ? (long long)PP_R * a.pitch : PP_OUT_BYTES;
  const long long lds = 4LL * ((long long)a.kx * PP_TW + (long long)a.ky * PP_TH + PP_R * 3 * PP_TW + 2 * PP_TW + 2 * PP_TH) + stage_bytes;
  if (lds > PP_MAX_LDS) {
    qt_set_error("qt_preprocess_u8: downscale limit: source %d x %d -> output %d x %d needs %lld bytes of LDS per workgroup (%d at most)",
                 d->src_h, d->src_w, d->out_h, d->out_w, lds, PP_MAX_LDS);
    return QT_ERR_UNSUPPORTED;
  }
  const long long blocks = (long long)d->batch * a.tiles_x * a.tiles_y;
  if (blocks > (long long)INT32_MAX) {
    qt_set_error("qt_preprocess_u8: %lld output tiles in one call; at most %d are handled", blocks, INT32_MAX);
    return QT_ERR_UNSUPPORTED;
  }
  for (int c = 0; c < 3; ++c) {
    a.scale[c] = (float)((double)d->inv_std[c] / 255.0);
    a.shift[c] = (float)(-(double)d->mean[c] * (double)d->inv_std[c]);
  }
  hipLaunchKernelGGL(preprocess_u8_kernel, dim3((unsigned)blocks), dim3(PP_THREADS), (size_t)lds, static_cast<hipStream_t>(stream), a);
  QT_CHECK_LAUNCH();
  return QT_OK;
}
