// Grad-CAM on the device: activations and gradients of the hooked layer to the normalised class map (qt_gradcam_map), and
// the map drawn over uint8 frames (qt_gradcam_overlay_u8).  The rule is the reference's (resnet/grad_cam_analysis.py:306-343,
// grad_cam/5_grad_cam_visualizer.py:220-275, Quadtree_from scratch/grad_cam.py:70-96); include/qtcnn.h states it in full.
//
// qt_gradcam_map, per image:  w_c = mean_p grad[c][p],  s_p = sum_c w_c act[c][p],  r_p = max(s_p, 0),  peak = max_p r_p,
// cam_p = r_p / peak (all zeros when peak == 0).
//   1. A workgroup owns one image and one chunk of GC_CHUNK channels.  Each wave pools the gradients of its channels (lane l
//      adds positions l, l + 64, ... in ascending order, then the 64 lane sums in a fixed tree) and leaves w_c in LDS.
//      The 256 threads then form `groups` channel groups of `lanes` position lanes each (lanes = the power of two >= P,
//      at most 256): group g adds w_c act[c][p] over its channels g, g + groups, ... in ascending order, and the group
//      sums of a position are added in ascending g.
//   2. With one chunk (C <= GC_CHUNK) the same workgroup finishes the image: one launch.  Otherwise the chunk sums go to
//      the caller's workspace, [image][chunk][P], and a second launch of one workgroup per image adds a position's chunks
//      in ascending order and finishes.  Measured on the MI355X (EXPERIMENTS.md, "Grad-CAM"): one workgroup per image
//      for every C takes 2.3 to 12 times as long at C = 512 / 1024, from a single image to a full batch; of 16, 32, 64 and
//      128 channels per workgroup, 32 is the best or within 3 us of it at every shape tried.
// The order of every sum depends on (C, P) only: no atomics, no zero fill, the same bits on every run and for an image on
// its own or inside a batch.
//
// qt_gradcam_overlay_u8: one launch.  A thread owns 16 consecutive pixels of the flat [B H W] pixel array = 48 bytes = three
// 16-byte stores; the first group starts at the first pixel whose byte address in `out` is a multiple of 16 (3 q + m = 0
// mod 16 has the solution q = 5 m mod 16), so every group is aligned whatever the row width.  The pixels in front of it
// and behind the last whole group (fewer than 16 each) go one per thread with byte accesses.  Frames whose address differs
// from out's modulo 16 are read bytewise.  The colour table sits in LDS, one packed word per entry.
#include <math.h>
#include <stdint.h>

#include "qt_common.h"

namespace {

#ifndef GC_CHUNK
#define GC_CHUNK 32                  // channels per workgroup of the map's first stage (EXPERIMENTS.md, "Grad-CAM")
#endif
constexpr int GC_THREADS = 256;
constexpr int GC_MAX_P = QT_GRADCAM_MAX_POSITIONS;
constexpr int GC_MAX_DIM = 1 << 22;  // pixel-centre coordinates (multiples of 0.5) stay exact in f32

struct CamArgs {
  const float* act;
  const float* grad;
  float* cam;
  float* peak;
  float* partial;      // [B][nchunks][P], only with nchunks > 1
  int C, P, nchunks;
  int lanes, groups;   // lanes * groups == GC_THREADS
  float fP;            // float(P)
};

// max that carries a NaN (fmaxf would drop it)
__device__ __forceinline__ float nan_max(float a, float b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }

// sum over the 64 lanes of a wave in a fixed order; every lane holds the result
__device__ __forceinline__ float wave_sum(float v) {
  v = qt_row16_sum(v);
  const int i = __builtin_bit_cast(int, v);
  const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(i, 0));
  const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(i, 16));
  const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(i, 32));
  const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(i, 48));
  return ((r0 + r1) + r2) + r3;
}

// s[0 .. P) in LDS holds s_p: ReLU, the NaN-carrying maximum, the division; written by all threads of the workgroup
__device__ __forceinline__ void cam_finish(float* s, float* red, int P, float* __restrict__ cam, float* __restrict__ peak) {
  const int tid = threadIdx.x;
  float m = 0.f;
  for (int p = tid; p < P; p += GC_THREADS) {
    const float v = s[p];
    const float r = v > 0.f ? v : (v == v ? 0.f : v);   // max(v, 0); a NaN stays, -0 becomes +0
    s[p] = r;
    m = nan_max(m, r);
  }
  red[tid] = m;
  __syncthreads();
  for (int k = GC_THREADS / 2; k >= 1; k >>= 1) {
    if (tid < k) red[tid] = nan_max(red[tid], red[tid + k]);
    __syncthreads();
  }
  const float pk = red[0];
  if (tid == 0) *peak = pk;
  for (int p = tid; p < P; p += GC_THREADS) cam[p] = pk == 0.f ? 0.f : s[p] / pk;   // own entries of s only
}

template <bool FUSED>
__global__ __launch_bounds__(GC_THREADS) void gradcam_chunk_kernel(CamArgs a) {
  __shared__ float w[GC_CHUNK];
  __shared__ float red[GC_THREADS];
  __shared__ float s[FUSED ? GC_MAX_P : 1];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long long b = blockIdx.x / a.nchunks;
  const int chunk = blockIdx.x % a.nchunks;
  const int c0 = chunk * GC_CHUNK;
  const int nc = min(GC_CHUNK, a.C - c0);
  const int P = a.P;
  const long long base = (b * a.C + c0) * (long long)P;
  const float* __restrict__ grad = a.grad + base;
  const float* __restrict__ act = a.act + base;

  // pooled weights: wave wv takes channels wv, wv + 4, ...
  for (int c = wv; c < nc; c += GC_THREADS / 64) {
    const float* __restrict__ g = grad + (long long)c * P;
    float acc = 0.f;
    for (int p = lane; p < P; p += 64) acc += g[p];
    const float sum = wave_sum(acc);
    if (lane == 0) w[c] = sum / a.fP;
  }
  __syncthreads();

  // weighted channel sum: thread = (group g, position lane pl)
  const int pl = tid & (a.lanes - 1), g = tid / a.lanes;
  float* __restrict__ dst = FUSED ? s : a.partial + (b * a.nchunks + chunk) * (long long)P;
  for (int p0 = 0; p0 < P; p0 += a.lanes) {   // one pass unless P > 256 (then groups == 1)
    const int p = p0 + pl;
    float acc = 0.f;
    if (p < P)
      for (int c = g; c < nc; c += a.groups) acc = fmaf(w[c], act[(long long)c * P + p], acc);
    if (a.groups == 1) {
      if (p < P) dst[p] = acc;
    } else {
      red[tid] = acc;
      __syncthreads();
      if (g == 0 && p < P) {
        float t = acc;
        for (int k = 1; k < a.groups; ++k) t += red[k * a.lanes + pl];
        dst[p] = t;
      }
    }
  }
  if constexpr (FUSED) {
    __syncthreads();
    cam_finish(s, red, P, a.cam + b * P, a.peak + b);
  }
}

__global__ __launch_bounds__(GC_THREADS) void gradcam_finish_kernel(CamArgs a) {
  __shared__ float red[GC_THREADS];
  __shared__ float s[GC_MAX_P];
  const long long b = blockIdx.x;
  const int P = a.P;
  const float* __restrict__ part = a.partial + b * a.nchunks * (long long)P;
  for (int p = threadIdx.x; p < P; p += GC_THREADS) {
    float t = part[p];
    for (int k = 1; k < a.nchunks; ++k) t += part[(long long)k * P + p];
    s[p] = t;   // read back by this thread only
  }
  cam_finish(s, red, P, a.cam + b * P, a.peak + b);
}

// ---- overlay -------------------------------------------------------------------------------------------------------------
struct OverlayArgs {
  const float* cam;
  const unsigned char* frames;
  const unsigned char* lut;
  unsigned char* out;
  float* heat;            // or nullptr
  unsigned char* index;   // or nullptr
  int h, w, H, W;
  long long groups;       // whole 16-pixel groups behind the head
  int head, tail;         // pixels in front of the first group / behind the last one
  int src_vec, heat_vec, index_vec;   // 16-byte accesses possible for frames / heat / index
  float sy, sx;           // h / H, w / W
  float alpha, beta;      // beta = 1 - alpha
};

struct Axis {
  int i0, i1;
  float t;
};
// source taps and weight of destination index d: f = (d + 0.5) scale - 0.5, taps floor(f) and floor(f) + 1 clamped
__device__ __forceinline__ Axis axis_of(int d, float scale, int n) {
  const float f = fmaf((float)d + 0.5f, scale, -0.5f);
  const float fl = floorf(f);
  Axis A;
  A.t = f - fl;
  const int i = (int)fl;
  A.i0 = min(max(i, 0), n - 1);
  A.i1 = min(max(i + 1, 0), n - 1);
  return A;
}

struct Shade {
  float v;
  unsigned idx;
};
__device__ __forceinline__ Shade shade_of(const float* __restrict__ cam, const Axis& Y, const Axis& X, int w) {
  const float* __restrict__ r0 = cam + (long long)Y.i0 * w;
  const float* __restrict__ r1 = cam + (long long)Y.i1 * w;
  // a + t (b - a): two equal taps (a 1 x 1 map, a clamped border, t == 0) give that value exactly
  const float top = fmaf(X.t, r0[X.i1] - r0[X.i0], r0[X.i0]);
  const float bot = fmaf(X.t, r1[X.i1] - r1[X.i0], r1[X.i0]);
  Shade S;
  S.v = fmaf(Y.t, bot - top, top);
  S.idx = S.v > 0.f ? (unsigned)(int)fminf(255.f * S.v, 255.f) : 0u;   // a NaN gives 0
  return S;
}
// uint8(floor(alpha colour + (1 - alpha) pixel)); both terms are >= 0 and the sum is <= 255 for alpha in [0, 1]
__device__ __forceinline__ unsigned blend(float alpha, float beta, unsigned colour, unsigned pixel) {
  return (unsigned)(int)fmaf(alpha, (float)colour, beta * (float)pixel) & 0xffu;
}

__global__ __launch_bounds__(GC_THREADS) void gradcam_overlay_kernel(OverlayArgs a) {
  __shared__ unsigned lut[256];   // channel k of entry i in bits 8k .. 8k+7
  {
    const unsigned char* __restrict__ e = a.lut + 3 * threadIdx.x;
    lut[threadIdx.x] = (unsigned)e[0] | ((unsigned)e[1] << 8) | ((unsigned)e[2] << 16);
  }
  __syncthreads();
  const long long gid = (long long)blockIdx.x * GC_THREADS + threadIdx.x;
  const long long plane = (long long)a.H * a.W;
  if (gid < a.groups) {
    const long long q0 = a.head + gid * 16;
    long long b = q0 / plane;
    const int rem = (int)(q0 - b * plane);
    int y = rem / a.W, x = rem - y * a.W;
    unsigned in[12], o[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, ix[4] = {0, 0, 0, 0};
    float hv[16];
    if (a.src_vec) {
      const uint4* __restrict__ src = reinterpret_cast<const uint4*>(a.frames + 3 * q0);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const uint4 u = src[k];
        in[4 * k] = u.x; in[4 * k + 1] = u.y; in[4 * k + 2] = u.z; in[4 * k + 3] = u.w;
      }
    } else {
      const unsigned char* __restrict__ src = a.frames + 3 * q0;
#pragma unroll
      for (int k = 0; k < 12; ++k)
        in[k] = (unsigned)src[4 * k] | ((unsigned)src[4 * k + 1] << 8) | ((unsigned)src[4 * k + 2] << 16) |
                ((unsigned)src[4 * k + 3] << 24);
    }
    Axis Y = axis_of(y, a.sy, a.h);
    const float* __restrict__ cam = a.cam + b * a.h * (long long)a.w;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const Axis X = axis_of(x, a.sx, a.w);
      const Shade S = shade_of(cam, Y, X, a.w);
      const unsigned col = lut[S.idx];
      hv[j] = S.v;
      ix[j >> 2] |= S.idx << (8 * (j & 3));
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int byte = 3 * j + c;
        const unsigned pix = (in[byte >> 2] >> (8 * (byte & 3))) & 0xffu;
        o[byte >> 2] |= blend(a.alpha, a.beta, (col >> (8 * c)) & 0xffu, pix) << (8 * (byte & 3));
      }
      if (++x == a.W) {   // next row, possibly of the next image
        x = 0;
        if (++y == a.H) {
          y = 0;
          ++b;
          cam += a.h * (long long)a.w;   // (not read when this was the last pixel of the batch)
        }
        Y = axis_of(y, a.sy, a.h);
      }
    }
    uint4* __restrict__ dst = reinterpret_cast<uint4*>(a.out + 3 * q0);
    dst[0] = make_uint4(o[0], o[1], o[2], o[3]);
    dst[1] = make_uint4(o[4], o[5], o[6], o[7]);
    dst[2] = make_uint4(o[8], o[9], o[10], o[11]);
    if (a.heat) {
      float* __restrict__ hp = a.heat + q0;
      if (a.heat_vec) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          reinterpret_cast<float4*>(hp)[k] = make_float4(hv[4 * k], hv[4 * k + 1], hv[4 * k + 2], hv[4 * k + 3]);
      } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) hp[j] = hv[j];
      }
    }
    if (a.index) {
      unsigned char* __restrict__ ip = a.index + q0;
      if (a.index_vec) {
        *reinterpret_cast<uint4*>(ip) = make_uint4(ix[0], ix[1], ix[2], ix[3]);
      } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) ip[j] = (unsigned char)((ix[j >> 2] >> (8 * (j & 3))) & 0xffu);
      }
    }
    return;
  }
  // the pixels in front of the first group and behind the last one: one per thread
  const long long e = gid - a.groups;
  if (e >= a.head + a.tail) return;
  const long long q = e < a.head ? e : a.head + a.groups * 16 + (e - a.head);
  const long long b = q / plane;
  const int rem = (int)(q - b * plane);
  const int y = rem / a.W, x = rem - y * a.W;
  const Shade S = shade_of(a.cam + b * a.h * (long long)a.w, axis_of(y, a.sy, a.h), axis_of(x, a.sx, a.w), a.w);
  const unsigned col = lut[S.idx];
#pragma unroll
  for (int c = 0; c < 3; ++c)
    a.out[3 * q + c] = (unsigned char)blend(a.alpha, a.beta, (col >> (8 * c)) & 0xffu, a.frames[3 * q + c]);
  if (a.heat) a.heat[q] = S.v;
  if (a.index) a.index[q] = (unsigned char)S.idx;
}

int cam_chunks(int C) { return qt_cdiv(C, GC_CHUNK); }

}  // namespace

extern "C" size_t qt_gradcam_workspace_bytes(int batch, int C, int P) {
  if (batch < 1 || C < 1 || P < 1 || P > GC_MAX_P) return 0;
  const int nchunks = cam_chunks(C);
  return nchunks > 1 ? (size_t)batch * nchunks * P * sizeof(float) : 0;
}

extern "C" int qt_gradcam_map(const float* act, const float* grad, int batch, int C, int P, float* cam, float* peak,
                              void* workspace, size_t workspace_bytes, void* stream) {
  QT_CHECK_ARG(batch >= 1 && C >= 1 && P >= 1, "qt_gradcam_map: sizes must be positive (batch %d, C %d, P %d)", batch, C, P);
  if (P > GC_MAX_P) {
    qt_set_error("qt_gradcam_map: %d positions per image; at most %d are handled", P, GC_MAX_P);
    return QT_ERR_UNSUPPORTED;
  }
  const int nchunks = cam_chunks(C);
  if ((long long)batch * nchunks > (long long)INT32_MAX) {
    qt_set_error("qt_gradcam_map: %lld workgroups in one call; at most %d are handled", (long long)batch * nchunks, INT32_MAX);
    return QT_ERR_UNSUPPORTED;
  }
  QT_CHECK_ARG(act && grad && cam && peak, "qt_gradcam_map: null activations / gradients / map / peak");
  QT_CHECK_ARG(((reinterpret_cast<uintptr_t>(act) | reinterpret_cast<uintptr_t>(grad) | reinterpret_cast<uintptr_t>(cam) |
                 reinterpret_cast<uintptr_t>(peak) | reinterpret_cast<uintptr_t>(workspace)) & 3) == 0,
               "qt_gradcam_map: activations, gradients, map, peak and workspace must be 4-byte aligned");
  const size_t need = qt_gradcam_workspace_bytes(batch, C, P);
  QT_CHECK_ARG(need == 0 || (workspace && workspace_bytes >= need),
               "qt_gradcam_map: workspace of %zu bytes needed (qt_gradcam_workspace_bytes), got %zu", need, workspace_bytes);
  CamArgs a;
  a.act = act;
  a.grad = grad;
  a.cam = cam;
  a.peak = peak;
  a.partial = static_cast<float*>(workspace);
  a.C = C;
  a.P = P;
  a.nchunks = nchunks;
  int lanes = 1;
  while (lanes < P && lanes < GC_THREADS) lanes <<= 1;
  a.lanes = lanes;
  a.groups = GC_THREADS / lanes;
  a.fP = (float)P;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (nchunks == 1) {
    hipLaunchKernelGGL(gradcam_chunk_kernel<true>, dim3((unsigned)batch), dim3(GC_THREADS), 0, st, a);
    QT_CHECK_LAUNCH();
    return QT_OK;
  }
  hipLaunchKernelGGL(gradcam_chunk_kernel<false>, dim3((unsigned)(batch * nchunks)), dim3(GC_THREADS), 0, st, a);
  QT_CHECK_LAUNCH();
  hipLaunchKernelGGL(gradcam_finish_kernel, dim3((unsigned)batch), dim3(GC_THREADS), 0, st, a);
  QT_CHECK_LAUNCH();
  return QT_OK;
}

extern "C" int qt_gradcam_overlay_u8(const float* cam, int h, int w, const unsigned char* frames, int batch, int H, int W,
                                     const unsigned char* lut, float alpha, unsigned char* out, float* heat,
                                     unsigned char* index, void* stream) {
  QT_CHECK_ARG(batch >= 1 && h >= 1 && w >= 1 && H >= 1 && W >= 1,
               "qt_gradcam_overlay_u8: sizes must be positive (batch %d, map %d x %d, frames %d x %d)", batch, h, w, H, W);
  QT_CHECK_ARG(alpha >= 0.f && alpha <= 1.f, "qt_gradcam_overlay_u8: alpha must be in [0, 1] (got %g)", (double)alpha);   // NaN fails too
  if (h > GC_MAX_DIM || w > GC_MAX_DIM || H > GC_MAX_DIM || W > GC_MAX_DIM) {
    qt_set_error("qt_gradcam_overlay_u8: map %d x %d, frames %d x %d: at most %d lines or columns are handled", h, w, H, W,
                 GC_MAX_DIM);
    return QT_ERR_UNSUPPORTED;
  }
  QT_CHECK_ARG(cam && frames && lut && out, "qt_gradcam_overlay_u8: null map / frames / colour table / output");
  QT_CHECK_ARG(((reinterpret_cast<uintptr_t>(cam) | reinterpret_cast<uintptr_t>(heat)) & 3) == 0,
               "qt_gradcam_overlay_u8: map and heat plane must be 4-byte aligned");
  const long long total = (long long)batch * H * W;
  OverlayArgs a;
  a.cam = cam;
  a.frames = frames;
  a.lut = lut;
  a.out = out;
  a.heat = heat;
  a.index = index;
  a.h = h;
  a.w = w;
  a.H = H;
  a.W = W;
  const int m = (int)(reinterpret_cast<uintptr_t>(out) & 15u);
  const int head = (5 * m) & 15;   // first q with 3 q + m = 0 (mod 16)
  a.head = total < head ? (int)total : head;
  a.groups = (total - a.head) / 16;
  a.tail = (int)(total - a.head - a.groups * 16);
  a.src_vec = ((reinterpret_cast<uintptr_t>(frames) ^ reinterpret_cast<uintptr_t>(out)) & 15u) == 0;
  a.heat_vec = ((reinterpret_cast<uintptr_t>(heat) + 4u * (unsigned)a.head) & 15u) == 0;
  a.index_vec = ((reinterpret_cast<uintptr_t>(index) + (unsigned)a.head) & 15u) == 0;
  a.sy = (float)h / (float)H;
  a.sx = (float)w / (float)W;
  a.alpha = alpha;
  a.beta = 1.f - alpha;
  const long long threads = a.groups + a.head + a.tail;
  const long long blocks = (threads + GC_THREADS - 1) / GC_THREADS;
  if (blocks > (long long)INT32_MAX) {
    qt_set_error("qt_gradcam_overlay_u8: %lld pixels in one call; at most %lld are handled", total, 16LL * GC_THREADS * INT32_MAX);
    return QT_ERR_UNSUPPORTED;
  }
  hipLaunchKernelGGL(gradcam_overlay_kernel, dim3((unsigned)blocks), dim3(GC_THREADS), 0, static_cast<hipStream_t>(stream), a);
  QT_CHECK_LAUNCH();
  return QT_OK;
}
