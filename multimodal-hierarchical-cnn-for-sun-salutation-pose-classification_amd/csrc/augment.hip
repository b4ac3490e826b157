// Training augmentations on the device (qt_augment_f32): ColorJitter -> RandomRotation -> GaussianBlur -> Normalize on the
// f32 [batch][3][h][w] planes that qt_preprocess_u8 writes with mean 0 / std 1, the middle of the reference's training
// transform (Quadtree_from scratch/dataloader.py:29-37).  The rule is torchvision's float-tensor path; include/qtcnn.h
// states it in full.
//
// The jitter ops are pointwise once the contrast mean is known, so "jitter, then rotate by gathering" is "gather the source
// pixel, then jitter it": no intermediate image exists in HBM.  A workgroup owns a 16-row x 64-column output tile in all
// three channels:
//   1. it reads the image's parameter row from device memory; a malformed row makes the tile NaN and nothing else is read;
//   2. one thread per axis forms the normalised blur taps exp(-0.5 (d / sigma)^2) / sum in LDS;
//   3. for every position of the tile plus its blur halo (reflected at the image border, index -1 reads 1) it computes the
//      nearest-neighbour source pixel of the rotation, loads its three channels, applies the jitter chain (or the fill 0
//      outside the image, which is not jittered) and stores the result into LDS;
//   4. rows are blurred out of LDS into LDS, columns out of LDS into registers (four rows per wave, ascending taps);
//   5. the normalised tile goes through LDS once more so that output rows leave as 16-byte stores with scalar ends.
// The contrast mean (mean of the grey image as it stands when contrast is reached) takes a first launch, only when the
// descriptor says contrast can occur: AG_PARTS workgroups per image apply the ops in front of contrast to a fixed chunk of
// pixels each and write one partial sum; the main kernel adds an image's partials in ascending order.
// No atomics, no zero fill, no host synchronisation, every summation order fixed: the same bits on every run.
#include <math.h>
#include <stdint.h>

#include "qt_common.h"

namespace {

constexpr int AG_THREADS = 256;
constexpr int AG_TW = 64;            // output columns per tile = lanes of a wave
constexpr int AG_TH = 16;            // output rows per tile, four per wave
constexpr int AG_MAXK = 15;          // largest blur kernel per axis
constexpr int AG_PARTS = QT_AUGMENT_PARTS;   // workgroups (= partial sums) per image in the contrast-mean launch
constexpr int AG_MAX_DIM = 1 << 22;  // pixel-centre coordinates (multiples of 0.5) stay exact in f32
constexpr int AG_ROW = QT_AUGMENT_PARAMS;

struct AugArgs {
  const float* src;
  const float* params;
  float* dst;
  float* partial;        // [batch][AG_PARTS]
  long long src_image_stride, dst_image_stride;
  int h, w, tiles_x, tiles_y;
  int kx, ky;
  int use_contrast;
  float hw;              // float(h * w)
  float scale[3], shift[3];   // out = v * scale + shift = (v - mean) * inv_std
};

struct AugRow {
  float f[4];      // brightness, contrast, saturation factor, hue shift
  int op[4];       // -1 = skip
  float cs, sn, sigma;
  bool valid, has_contrast;
};

__device__ __forceinline__ bool finite32(float v) { return fabsf(v) <= 3.402823466e+38f; }   // false for NaN and inf

// every thread reads the twelve floats of its image's row (one address per wave: a broadcast)
__device__ __forceinline__ AugRow load_row(const float* __restrict__ p, bool blur_on, bool use_contrast) {
  AugRow R;
  bool ok = true;
  float v[AG_ROW];
#pragma unroll
  for (int i = 0; i < AG_ROW; ++i) {
    v[i] = p[i];
    ok = ok && finite32(v[i]);
  }
  unsigned seen = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float s = v[4 + k];
    int id = -1;
    if (s == 0.f || s == 1.f || s == 2.f || s == 3.f) {
      id = (int)s;
      if ((seen >> id) & 1u) ok = false;
      seen |= 1u << id;
    } else if (s != -1.f) {
      ok = false;
    }
    R.op[k] = id;
    R.f[k] = v[k];
  }
  R.cs = v[8];
  R.sn = v[9];
  R.sigma = v[10];
  R.has_contrast = (seen & 2u) != 0;
  if (blur_on && !(R.sigma > 0.f)) ok = false;
  if (!use_contrast && R.has_contrast) ok = false;
  R.valid = ok;
  return R;
}

// torch.clamp(v, 0, 1): a NaN stays a NaN (fminf / fmaxf would return the other operand)
__device__ __forceinline__ float clamp01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }

__device__ __forceinline__ float grey_of(float r, float g, float b) { return fmaf(0.114f, b, fmaf(0.587f, g, 0.2989f * r)); }

__device__ __forceinline__ void hue_shift(float shift, float& r, float& g, float& b) {
  if (!(r == r && g == g && b == b)) {   // torch's max / min carry a NaN channel into v, s and h: the whole pixel
    r = g = b = __uint_as_float(0x7fc00000u);
    return;
  }
  const float maxc = r > g ? (r > b ? r : b) : (g > b ? g : b);
  const float minc = r < g ? (r < b ? r : b) : (g < b ? g : b);
  const float cr = maxc - minc;
  const bool eq = cr == 0.f;   // maxc == minc
  const float s = cr / (eq ? 1.f : maxc);
  const float crd = eq ? 1.f : cr;
  const float rc = (maxc - r) / crd, gc = (maxc - g) / crd, bc = (maxc - b) / crd;
  float hh;
  if (maxc == r) hh = bc - gc;
  else if (maxc == g) hh = (2.f + rc) - bc;
  else hh = (4.f + gc) - rc;
  hh = hh / 6.f + 1.f;            // in [5/6, 11/6]
  hh = hh - floorf(hh);           // fmod(., 1) of a positive number
  hh = hh + shift;
  hh = hh - floorf(hh);           // (h + shift) mod 1, in [0, 1]
  const float h6 = 6.f * hh;
  const float fi = floorf(h6);
  const float f = h6 - fi;
  int i = (int)fi;                // 0 .. 6
  if (i >= 6) i -= 6;
  const float v = maxc;
  const float p = clamp01(v * (1.f - s));
  const float q = clamp01(v * (1.f - s * f));
  const float t = clamp01(v * (1.f - s * (1.f - f)));
  switch (i) {
    case 0: r = v; g = t; b = p; break;
    case 1: r = q; g = v; b = p; break;
    case 2: r = p; g = v; b = t; break;
    case 3: r = p; g = q; b = v; break;
    case 4: r = t; g = p; b = v; break;
    default: r = v; g = p; b = q; break;
  }
}

// The jitter chain in the slots' order.  contrast_term = (1 - f_contrast) * mean; with stop_at_contrast the ops in front of
// contrast only (what the mean is taken of).  The branches are the same for every thread of a workgroup.
__device__ __forceinline__ void jitter(const AugRow& R, float contrast_term, bool stop_at_contrast, float& r, float& g, float& b) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int op = R.op[k];
    if (op == 0) {
      const float f = R.f[0];
      r = clamp01(f * r);
      g = clamp01(f * g);
      b = clamp01(f * b);
    } else if (op == 1) {
      if (stop_at_contrast) return;
      const float f = R.f[1];
      r = clamp01(fmaf(f, r, contrast_term));
      g = clamp01(fmaf(f, g, contrast_term));
      b = clamp01(fmaf(f, b, contrast_term));
    } else if (op == 2) {
      const float f = R.f[2];
      const float t = (1.f - f) * grey_of(r, g, b);
      r = clamp01(fmaf(f, r, t));
      g = clamp01(fmaf(f, g, t));
      b = clamp01(fmaf(f, b, t));
    } else if (op == 3) {
      hue_shift(R.f[3], r, g, b);
    }
  }
}

// One partial sum of the grey image per workgroup: partial[b * AG_PARTS + part] over the pixels
// [part * chunk, min((part + 1) * chunk, h w)), chunk = ceil(h w / AG_PARTS).  Thread t adds its pixels t, t + 256, ... in
// ascending order, then a binary tree over the 256 threads in LDS.  Every slot is written (no zero fill beforehand).
__global__ __launch_bounds__(AG_THREADS) void augment_grey_partial_kernel(AugArgs a) {
  __shared__ float red[AG_THREADS];
  const int tid = threadIdx.x;
  const long long b = blockIdx.x / AG_PARTS;
  const int part = blockIdx.x % AG_PARTS;
  const AugRow R = load_row(a.params + b * AG_ROW, a.kx * a.ky > 1, true);
  if (!R.valid || !R.has_contrast) {   // the same for every thread; the main kernel does not read the slot
    if (tid == 0) a.partial[blockIdx.x] = 0.f;
    return;
  }
  const long long plane = (long long)a.h * a.w;
  const long long chunk = (plane + AG_PARTS - 1) / AG_PARTS;
  const long long lo = part * chunk;
  const long long hi = lo + chunk < plane ? lo + chunk : plane;
  const float* __restrict__ simg = a.src + b * a.src_image_stride;
  float sum = 0.f;
  for (long long p = lo + tid; p < hi; p += AG_THREADS) {
    float r = simg[p], g = simg[plane + p], bl = simg[2 * plane + p];
    jitter(R, 0.f, true, r, g, bl);
    sum += grey_of(r, g, bl);
  }
  red[tid] = sum;
  __syncthreads();
  for (int s = AG_THREADS / 2; s >= 1; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) a.partial[blockIdx.x] = red[0];
}

__device__ __forceinline__ int reflect(int i, int n) {   // n > |overhang|: one reflection is enough
  if (i < 0) i = -i;
  if (i >= n) i = 2 * (n - 1) - i;
  return i;
}

__global__ __launch_bounds__(AG_THREADS) void augment_f32_kernel(AugArgs a) {
  extern __shared__ __align__(16) unsigned char ag_smem[];
  const int rx = a.kx >> 1, ry = a.ky >> 1;
  const int pitch = AG_TW + 2 * rx;         // floats per staged row
  const int rows_max = AG_TH + 2 * ry;
  float* wx = reinterpret_cast<float*>(ag_smem);   // [16] normalised taps along a row
  float* wy = wx + 16;                             // [16] along a column
  float* T = wy + 16;                              // [3][rows_max][pitch] jittered, rotated tile with halo; later the output tile
  float* H = T + 3 * rows_max * pitch;             // [3][rows_max][64] row-blurred

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int bid = blockIdx.x;
  const int tx = bid % a.tiles_x;
  const int ty = (bid / a.tiles_x) % a.tiles_y;
  const long long b = bid / (a.tiles_x * a.tiles_y);
  const int p0 = tx * AG_TW, oy0 = ty * AG_TH;
  const int ntw = min(AG_TW, a.w - p0), nth = min(AG_TH, a.h - oy0);
  float* __restrict__ dimg = a.dst + b * a.dst_image_stride;
  const float* __restrict__ simg = a.src + b * a.src_image_stride;
  const long long plane = (long long)a.h * a.w;

  const AugRow R = load_row(a.params + b * AG_ROW, a.kx * a.ky > 1, a.use_contrast != 0);
  if (!R.valid) {   // the same for every thread of the workgroup
    const float nan = __uint_as_float(0x7fc00000u);
    for (int e = tid; e < 3 * nth * ntw; e += AG_THREADS) {
      const int c = e / (nth * ntw), rem = e % (nth * ntw);
      dimg[c * plane + (long long)(oy0 + rem / ntw) * a.w + p0 + rem % ntw] = nan;
    }
    return;
  }

  // blur taps: thread 0 the row taps, thread 64 the column taps (first thread of another wave)
  if (tid == 0 || tid == 64) {
    float* wk = tid == 0 ? wx : wy;
    const int n = tid == 0 ? a.kx : a.ky;
    const int rr = n >> 1;
    float raw[AG_MAXK];
    float S = 0.f;
#pragma unroll
    for (int k = 0; k < AG_MAXK; ++k) {
      if (k < n) {
        const float q = (float)(k - rr) / R.sigma;
        raw[k] = n > 1 ? expf(-0.5f * (q * q)) : 1.f;
        S += raw[k];
      }
    }
#pragma unroll
    for (int k = 0; k < AG_MAXK; ++k)
      if (k < n) wk[k] = raw[k] / S;
  }

  // contrast mean: the image's partial sums in ascending order
  float contrast_term = 0.f;
  if (R.has_contrast) {
    const float* __restrict__ part = a.partial + b * AG_PARTS;
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < AG_PARTS; ++k) sum += part[k];
    contrast_term = (1.f - R.f[1]) * (sum / a.hw);
  }

  // the tile plus its halo: source pixel of the rotation, jitter, into LDS
  const int nrows = nth + 2 * ry, ncols = ntw + 2 * rx;
  const float half_w = 0.5f * (float)a.w, half_h = 0.5f * (float)a.h;
  const float last_x = (float)(a.w - 1), last_y = (float)(a.h - 1);
  for (int e = tid; e < nrows * ncols; e += AG_THREADS) {
    const int lr = e / ncols, lc = e - lr * ncols;
    const int i = reflect(oy0 - ry + lr, a.h), j = reflect(p0 - rx + lc, a.w);
    const float x = ((float)j + 0.5f) - half_w, y = ((float)i + 0.5f) - half_h;   // exact: multiples of 0.5 below 2^22
    const float xs = fmaf(R.cs, x, -(R.sn * y));
    const float ys = fmaf(R.sn, x, R.cs * y);
    const float sx = rintf(xs + (half_w - 0.5f)), sy = rintf(ys + (half_h - 0.5f));
    float r = 0.f, g = 0.f, bl = 0.f;
    if (sx >= 0.f && sx <= last_x && sy >= 0.f && sy <= last_y) {   // false for a NaN coordinate as well
      const long long off = (long long)(int)sy * a.w + (int)sx;
      r = simg[off];
      g = simg[plane + off];
      bl = simg[2 * plane + off];
      jitter(R, contrast_term, false, r, g, bl);
    }
    const int o = lr * pitch + lc;
    T[o] = r;
    T[rows_max * pitch + o] = g;
    T[2 * rows_max * pitch + o] = bl;
  }
  __syncthreads();

  // rows: H[c][lr][x] = sum_k wx[k] T[c][lr][x + k], ascending k
  for (int e = tid; e < 3 * nrows * AG_TW; e += AG_THREADS) {
    const int x = e & (AG_TW - 1), s = e >> 6;   // s = c * nrows + lr
    const int c = s / nrows, lr = s - c * nrows;
    if (x < ntw) {
      const float* __restrict__ t = T + (c * rows_max + lr) * pitch + x;
      float acc = 0.f;
      for (int k = 0; k < a.kx; ++k) acc = fmaf(wx[k], t[k], acc);
      H[(c * rows_max + lr) * AG_TW + x] = acc;
    }
  }
  __syncthreads();

  // columns: wave wv owns output rows 4 wv .. 4 wv + 3 of the tile, lane = column; T is free and takes the output tile
  float* O = T;   // [3][16][64]
  if (lane < ntw) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int row = wv * 4 + q;
      if (row < nth) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float* __restrict__ hcol = H + (c * rows_max + row) * AG_TW + lane;
          float acc = 0.f;
          for (int k = 0; k < a.ky; ++k) acc = fmaf(wy[k], hcol[k * AG_TW], acc);
          O[(c * AG_TH + row) * AG_TW + lane] = fmaf(acc, a.scale[c], a.shift[c]);
        }
      }
    }
  }
  __syncthreads();
  // 16 lanes per output row segment: scalar stores up to the first 16-byte boundary, float4 stores, scalar tail
  const int j = tid & 15;
  for (int s = tid >> 4; s < 3 * nth; s += AG_THREADS / 16) {
    const int c = s / nth, row = s % nth;
    float* __restrict__ drow = dimg + c * plane + (long long)(oy0 + row) * a.w + p0;
    const float* __restrict__ orow = O + (c * AG_TH + row) * AG_TW;
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

}  // namespace

extern "C" size_t qt_augment_workspace_bytes(int batch, int use_contrast) {
  if (batch < 1 || !use_contrast) return 0;
  return (size_t)batch * AG_PARTS * sizeof(float);
}

extern "C" int qt_augment_f32(const qt_augment_desc* d, const float* src, const float* params, float* dst, void* workspace,
                              size_t workspace_bytes, void* stream) {
  QT_CHECK_ARG(d, "qt_augment_f32: null descriptor");
  QT_CHECK_ARG(d->batch >= 1 && d->h >= 1 && d->w >= 1, "qt_augment_f32: sizes must be positive (batch %d, image %d x %d)", d->batch,
               d->h, d->w);
  if (d->h > AG_MAX_DIM || d->w > AG_MAX_DIM) {
    qt_set_error("qt_augment_f32: image %d x %d: at most %d lines or columns are handled", d->h, d->w, AG_MAX_DIM);
    return QT_ERR_UNSUPPORTED;
  }
  QT_CHECK_ARG(d->blur_kx >= 1 && d->blur_kx <= AG_MAXK && (d->blur_kx & 1) && d->blur_ky >= 1 && d->blur_ky <= AG_MAXK && (d->blur_ky & 1),
               "qt_augment_f32: blur kernel %d x %d: both sizes must be odd and at most %d", d->blur_kx, d->blur_ky, AG_MAXK);
  QT_CHECK_ARG(d->w > d->blur_kx / 2 && d->h > d->blur_ky / 2,
               "qt_augment_f32: blur kernel %d x %d reflects further than the %d x %d image reaches (needs w > kx / 2, h > ky / 2)",
               d->blur_kx, d->blur_ky, d->h, d->w);
  QT_CHECK_ARG(d->use_contrast == 0 || d->use_contrast == 1, "qt_augment_f32: use_contrast must be 0 or 1 (got %d)", d->use_contrast);
  const long long image = 3LL * d->h * d->w;
  QT_CHECK_ARG(d->src_image_stride >= image, "qt_augment_f32: source image stride %lld < 3 * h * w = %lld", d->src_image_stride, image);
  QT_CHECK_ARG(d->dst_image_stride >= image, "qt_augment_f32: destination image stride %lld < 3 * h * w = %lld", d->dst_image_stride,
               image);
  QT_CHECK_ARG(src && params && dst, "qt_augment_f32: null source / parameter rows / destination");
  QT_CHECK_ARG(((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(params) | reinterpret_cast<uintptr_t>(dst) |
                 reinterpret_cast<uintptr_t>(workspace)) & 3) == 0,
               "qt_augment_f32: source, parameter rows, destination and workspace must be 4-byte aligned");
  for (int c = 0; c < 3; ++c)
    QT_CHECK_ARG(isfinite(d->mean[c]) && isfinite(d->inv_std[c]), "qt_augment_f32: mean / inv_std of channel %d is not finite", c);
  {
    // rotation and blur gather: the destination must not be the source
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(src), d0 = reinterpret_cast<uintptr_t>(dst);
    const unsigned long long s_bytes = 4ULL * ((unsigned long long)(d->batch - 1) * d->src_image_stride + image);
    const unsigned long long d_bytes = 4ULL * ((unsigned long long)(d->batch - 1) * d->dst_image_stride + image);
    QT_CHECK_ARG(s0 + s_bytes <= d0 || d0 + d_bytes <= s0, "qt_augment_f32: source and destination overlap");
  }
  if (d->use_contrast) {
    const size_t need = qt_augment_workspace_bytes(d->batch, 1);
    QT_CHECK_ARG(workspace && workspace_bytes >= need, "qt_augment_f32: workspace of %zu bytes needed for the contrast mean (got %zu)",
                 need, workspace_bytes);
  }
  AugArgs a;
  a.src = src;
  a.params = params;
  a.dst = dst;
  a.partial = static_cast<float*>(workspace);
  a.src_image_stride = d->src_image_stride;
  a.dst_image_stride = d->dst_image_stride;
  a.h = d->h;
  a.w = d->w;
  a.tiles_x = qt_cdiv(d->w, AG_TW);
  a.tiles_y = qt_cdiv(d->h, AG_TH);
  a.kx = d->blur_kx;
  a.ky = d->blur_ky;
  a.use_contrast = d->use_contrast;
  a.hw = (float)((long long)d->h * d->w);
  for (int c = 0; c < 3; ++c) {
    a.scale[c] = d->inv_std[c];
    a.shift[c] = (float)(-(double)d->mean[c] * (double)d->inv_std[c]);
  }
  const long long blocks = (long long)d->batch * a.tiles_x * a.tiles_y;
  if (blocks > (long long)INT32_MAX || (long long)d->batch * AG_PARTS > (long long)INT32_MAX) {
    qt_set_error("qt_augment_f32: %lld output tiles in one call; at most %d are handled", blocks, INT32_MAX);
    return QT_ERR_UNSUPPORTED;
  }
  const int rows_max = AG_TH + (d->blur_ky & ~1), pitch = AG_TW + (d->blur_kx & ~1);
  const size_t lds = 4u * (32u + 3u * rows_max * pitch + 3u * rows_max * AG_TW);   // 51 KiB at 15 x 15
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (d->use_contrast) {
    hipLaunchKernelGGL(augment_grey_partial_kernel, dim3((unsigned)(d->batch * AG_PARTS)), dim3(AG_THREADS), 0, st, a);
    QT_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(augment_f32_kernel, dim3((unsigned)blocks), dim3(AG_THREADS), lds, st, a);
  QT_CHECK_LAUNCH();
  return QT_OK;
}
