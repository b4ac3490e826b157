// Data gradient of the stem convolution (7x7 / stride 2 / pad 3, 3 -> 64 channels) down to the f32 NCHW image:
// dx[B][3][224][224] = conv_transpose2d(dy, W, stride 2, padding 3), the gradient torch gives `image_input.grad` of
// /root/reference/resnet/grad_cam_analysis.py:247 (image.requires_grad_(True)) through resnet18.conv1.
//
// The 2 x 2 image pixels (2y + py, 2x + px) of block (y, x) are reached by conv1 outputs (y + wy - 1, x + wx - 1),
// wy, wx in 0..3, through filter tap (py + 5 - 2 wy, px + 5 - 2 wx) where that lies inside the 7 x 7 filter.  So the whole
// operation is one GEMM: M = B * 112 * 112 blocks, K = 16 window taps x 64 channels = 1024, N = 3 channels x 4 parities =
// 12 (padded to 16; 49 of the 64 window-tap x parity pairs are real filter taps, the others multiply zeros).
//   * A operand (16 rows n = 4 c + 2 py + px) = the flipped filter, built per workgroup from the f32 OIHW master weight in
//     LDS, laid out [K-step][lane] so that every lane reads its fragment with one conflict-free ds_read_b128.  bf16: the
//     weight is split into hi + lo bf16 halves (two MFMAs per K-step on the same dy fragment), so the product carries the
//     f32 weight to ~2^-17 and the only rounding of the bf16 build is the one dy already has.
//   * B operand (16 columns = 16 consecutive blocks of one row) = dy rows of the tile plus their 3-pixel halo in LDS
//     (each dy element is read from memory about 1.3 times: tiles overlap by the halo).  The next tile's rows are loaded
//     into registers while the current tile is multiplied (persistent grid).
//   * epilogue: lane (column x, row group c) holds the four parities of channel c of block x: two 8-byte stores, 16 lanes
//     of a row group fill 128 contiguous bytes of an image row.
// Bound: the dy read (411 MB at B = 256, bf16) and the 154 MB dx write (HBM); the MFMA work is ~105 GFLOP (bf16: x2 for
// the hi / lo weight halves).
#include <atomic>

#include "qt_common.h"

namespace {

constexpr int SD_TX = 16;              // blocks per tile row (one MFMA's columns)
constexpr int SD_HX = SD_TX + 3;       // halo columns: ox in [x0 - 1, x0 + 18)
constexpr int SD_TILES_X = 112 / SD_TX;

template <typename T> struct SdCfg;
template <> struct SdCfg<bf16_t> {
  static constexpr int kWaves = 8;     // 16 block rows per tile, 2 per wave
  static constexpr int kSplit = 2;     // hi + lo weight halves
};
template <> struct SdCfg<float> {
  static constexpr int kWaves = 4;     // 8 block rows per tile (the f32 halo of 16 rows would not fit beside the weights)
  static constexpr int kSplit = 1;
};

template <typename T> struct SdGeom {
  static constexpr int kThreads = SdCfg<T>::kWaves * 64;
  static constexpr int kTY = 2 * SdCfg<T>::kWaves;          // block rows per tile
  static constexpr int kHY = kTY + 3;                        // halo rows: oy in [y0 - 1, y0 + kTY + 2)
  static constexpr int kTilesY = 112 / kTY;
  static constexpr int kCH = 16 / (int)sizeof(T);            // channels per 16-byte chunk: 8 bf16 / 4 f32
  static constexpr int kChunks = 64 / kCH;                   // 16-byte chunks per dy pixel
  static constexpr int kSPT = kChunks / 4;                   // K-steps per window tap (4 lane groups per step)
  static constexpr int kSteps = 16 * kSPT;
  static constexpr int kPix = 64 * (int)sizeof(T) + 16;      // LDS bytes per halo pixel (16 B pad against bank conflicts)
  static constexpr int kWBytes = SdCfg<T>::kSplit * kSteps * 64 * 16;
  static constexpr int kHBytes = kHY * SD_HX * kPix;
  static constexpr int kLds = kWBytes + kHBytes;
  static constexpr int kLoads = kHY * SD_HX * kChunks;
  static constexpr int kPer = (kLoads + kThreads - 1) / kThreads;
  static_assert(112 % kTY == 0 && 112 % SD_TX == 0, "tiles cover the 112 x 112 map");
  static_assert(kLds <= 160 * 1024, "LDS of one workgroup");
};

template <typename T>
__device__ __forceinline__ uint4 sd_pack(const float (&v)[16 / sizeof(T)]);
template <> __device__ __forceinline__ uint4 sd_pack<float>(const float (&v)[4]) {
  return make_uint4(__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3]));
}
template <> __device__ __forceinline__ uint4 sd_pack<bf16_t>(const float (&v)[8]) {
  bf16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = (bf16_t)v[j];
  return __builtin_bit_cast(uint4, o);
}

template <typename T>
__global__ __launch_bounds__(SdGeom<T>::kThreads) void stem_dgrad_kernel(const T* __restrict__ dy,
                                                                        const float* __restrict__ w,
                                                                        float* __restrict__ dx, int ntiles) {
  using G = SdGeom<T>;
  constexpr int CH = G::kCH;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint4* wl = reinterpret_cast<uint4*>(smem);                // [split][step][lane]
  unsigned char* hl = smem + G::kWBytes;                     // [halo row][halo column][kPix]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = tid >> 6;
  const int li = lane & 15, lg = lane >> 4;

  // ---- filter fragments: row n = 4 c + 2 py + px, k = (window tap, channel) ----
  for (int i = tid; i < G::kSteps * 64; i += G::kThreads) {
    const int s = i >> 6, l = i & 63;
    const int n = l & 15, g = l >> 4;
    const int tap = s / G::kSPT, part = s % G::kSPT;
    const int wy = tap >> 2, wx = tap & 3;
    const int c = n >> 2, py = (n >> 1) & 1, px = n & 1;
    const int ky = py + 5 - 2 * wy, kx = px + 5 - 2 * wx;  // <= 6 always
    const bool valid = n < 12 && ky >= 0 && kx >= 0;
    float hi[CH], lo[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      const int ch = (part * 4 + g) * CH + j;
      const float v = valid ? w[((ch * 3 + c) * 7 + ky) * 7 + kx] : 0.f;
      if constexpr (sizeof(T) == 2) {
        const float h = (float)(bf16_t)v;
        hi[j] = h;
        lo[j] = v - h;
      } else {
        hi[j] = v;
        lo[j] = 0.f;
      }
    }
    wl[i] = sd_pack<T>(hi);
    if constexpr (SdCfg<T>::kSplit == 2) wl[G::kSteps * 64 + i] = sd_pack<T>(lo);
  }

  // ---- dy halo of a tile: global -> registers (issued a tile ahead) -> LDS ----
  uint4 pre[G::kPer];
  auto load = [&](int t) {
    const int per_img = G::kTilesY * SD_TILES_X;
    const int b = t / per_img, r = t - b * per_img;
    const int y0 = (r / SD_TILES_X) * G::kTY, x0 = (r % SD_TILES_X) * SD_TX;
#pragma unroll
    for (int k = 0; k < G::kPer; ++k) {
      const int i = tid + k * G::kThreads;
      const int p = i / G::kChunks, q = i - p * G::kChunks;
      const int oy = y0 - 1 + p / SD_HX, ox = x0 - 1 + p % SD_HX;
      pre[k] = make_uint4(0u, 0u, 0u, 0u);
      if (i < G::kLoads && oy >= 0 && oy < 112 && ox >= 0 && ox < 112)
        pre[k] = *reinterpret_cast<const uint4*>(dy + (((size_t)b * 112 + oy) * 112 + ox) * 64 + q * CH);
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int k = 0; k < G::kPer; ++k) {
      const int i = tid + k * G::kThreads;
      const int p = i / G::kChunks, q = i - p * G::kChunks;
      if (i < G::kLoads) *reinterpret_cast<uint4*>(hl + p * G::kPix + q * 16) = pre[k];
    }
  };

  int t = blockIdx.x;
  if (t < ntiles) load(t);
  for (; t < ntiles; t += gridDim.x) {
    __syncthreads();  // the previous tile's LDS reads (and, the first time, the filter fill) are done
    store();
    __syncthreads();
    if (t + (int)gridDim.x < ntiles) load(t + gridDim.x);

    f32x4 acc[2];
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) acc[rr] = f32x4{0.f, 0.f, 0.f, 0.f};
    const unsigned char* hrow = hl + ((2 * wave) * SD_HX + li) * G::kPix + lg * 16;
#pragma unroll 4
    for (int s = 0; s < G::kSteps; ++s) {
      const int tap = s / G::kSPT, part = s % G::kSPT;
      const int wy = tap >> 2, wx = tap & 3;
      const uint4 whi = wl[s * 64 + lane];
      uint4 wlo;
      if constexpr (SdCfg<T>::kSplit == 2) wlo = wl[G::kSteps * 64 + s * 64 + lane];
#pragma unroll
      for (int rr = 0; rr < 2; ++rr) {
        const uint4 d = *reinterpret_cast<const uint4*>(hrow + ((rr + wy) * SD_HX + wx) * G::kPix + part * 64);
        QtMma<T>::run(acc[rr], whi, d);
        if constexpr (SdCfg<T>::kSplit == 2) QtMma<T>::run(acc[rr], wlo, d);
      }
    }

    // ---- epilogue: lane (block x0 + li, channel lg) holds parities (py, px) = (r >> 1, r & 1) ----
    if (lg < 3) {
      const int per_img = G::kTilesY * SD_TILES_X;
      const int b = t / per_img, r = t - b * per_img;
      const int y0 = (r / SD_TILES_X) * G::kTY, x0 = (r % SD_TILES_X) * SD_TX;
#pragma unroll
      for (int rr = 0; rr < 2; ++rr) {
        const int y = y0 + 2 * wave + rr, x = x0 + li;
        float* o = dx + (((size_t)b * 3 + lg) * 224 + 2 * y) * 224 + 2 * x;
        *reinterpret_cast<float2*>(o) = make_float2(acc[rr][0], acc[rr][1]);
        *reinterpret_cast<float2*>(o + 224) = make_float2(acc[rr][2], acc[rr][3]);
      }
    }
  }
}

template <typename T>
int launch_stem_dgrad(const void* dy, const float* w, float* dx, int batch, void* stream) {
  using G = SdGeom<T>;
  const int ntiles = batch * G::kTilesY * SD_TILES_X;
  static std::atomic<unsigned long long> lds_limit_set{0};  // per device
  if (int rc = qt_raise_lds_limit(reinterpret_cast<const void*>(stem_dgrad_kernel<T>), G::kLds, lds_limit_set)) return rc;
  const int cap = G::kLds * 2 <= 160 * 1024 ? 512 : 256;   // persistent: the workgroups that fit at once on 256 CUs
  const int grid = ntiles < cap ? ntiles : cap;
  hipLaunchKernelGGL(stem_dgrad_kernel<T>, dim3(grid), dim3(G::kThreads), G::kLds, static_cast<hipStream_t>(stream),
                     static_cast<const T*>(dy), w, dx, ntiles);
  QT_CHECK_LAUNCH();
  return QT_OK;
}

}  // namespace

extern "C" int qt_stem_dgrad(int dtype, const void* dy, const float* w_oihw, float* dx, int batch, void* stream) {
  QT_CHECK_ARG(dy && w_oihw && dx && batch > 0, "qt_stem_dgrad: bad argument");
  if ((dtype != QT_BF16 && dtype != QT_F32) || ((uintptr_t)dy % 16) != 0 || ((uintptr_t)dx % 8) != 0) {
    qt_set_error("qt_stem_dgrad: bf16 or f32 dy with 16-byte aligned dy and 8-byte aligned dx only");
    return QT_ERR_UNSUPPORTED;
  }
  return qt_by_dtype(dtype, [&](auto* t) { return launch_stem_dgrad<QT_T(t)>(dy, w_oihw, dx, batch, stream); });
}
