// Global 2-norm of a list of f32 tensors and the clip coefficient of torch.nn.utils.clip_grad_norm_, both left in device
// memory (qt_grad_norm_multi).  The Adam kernels of pack.hip multiply the gradient by that coefficient as they read it,
// so clipping costs one read of the gradients and no write (the reference clips between backward() and
// optimizer.step(): 3dcnn/train_3D_Quadtree_cnn_model.py:111-125).
//
// Two stages, no atomics, no zero fill, every order fixed -> the same bits on every run:
//   1. a workgroup owns one GN_CHUNK-element chunk of one tensor and writes its sum of squares to its own slot of the
//      caller's workspace; up to GN_MAX_ITEMS tensors per launch, as qt_adam_multi;
//   2. one workgroup adds the slots, takes the square root and writes {total_norm, clip_coef}.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "qt_common.h"

namespace {

constexpr int GN_MAX_ITEMS = 48, GN_THREADS = 256;
constexpr int GN_VEC_PER_THREAD = 8;                                // float4 loads in flight per thread
constexpr int GN_CHUNK = GN_THREADS * GN_VEC_PER_THREAD * 4;        // 8192 elements = 32 KB per workgroup

struct GradNormArgs {
  const float* g[GN_MAX_ITEMS];
  long long numel[GN_MAX_ITEMS];
  int first_block[GN_MAX_ITEMS + 1];
  int n;
  int slot0;   // this launch's first slot in the workspace
};

// elements in front of the first 16-byte boundary (0..3; f32 tensors are at least 4-byte aligned), capped by numel
__host__ __device__ inline int gn_head(const float* g, long long numel) {
  const int h = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(g) & 15u)) & 15u) >> 2);
  return numel < h ? (int)numel : h;
}
// chunks of the 16-byte aligned body; a tensor that is all head still gets one workgroup
inline long long gn_blocks(const float* g, long long numel) {
  const long long body = numel - gn_head(g, numel);
  const long long b = (body + GN_CHUNK - 1) / GN_CHUNK;
  return b < 1 ? 1 : b;
}

// Sum over the workgroup's 256 threads in a fixed order: DPP row sums, then the 16 row totals through LDS, added
// serially by thread 0 (the only thread that holds the result).
__device__ __forceinline__ float gn_block_sum(float acc) {
  __shared__ float rows[GN_THREADS / 16];
  acc = qt_row16_sum(acc);
  if ((threadIdx.x & 15) == 0) rows[threadIdx.x >> 4] = acc;
  __syncthreads();
  float s = 0.f;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int r = 0; r < GN_THREADS / 16; ++r) s += rows[r];
  }
  return s;
}

__global__ __launch_bounds__(GN_THREADS) void grad_sumsq_kernel(GradNormArgs a, float* __restrict__ partial) {
  int it = 0;
  while (it + 1 < a.n && (int)blockIdx.x >= a.first_block[it + 1]) ++it;
  const int chunk = blockIdx.x - a.first_block[it];
  const float* __restrict__ g = a.g[it];
  const long long n = a.numel[it];
  const int head = gn_head(g, n);
  const long long nvec = (n - head) >> 2;                      // whole float4s of the aligned body
  const float4* __restrict__ body = reinterpret_cast<const float4*>(g + head);
  const long long q0 = (long long)chunk * (GN_CHUNK / 4) + threadIdx.x;
  float4 v[GN_VEC_PER_THREAD];
  // all loads first, then the arithmetic; a whole chunk (uniform test) issues its eight loads back to back
  if ((long long)(chunk + 1) * (GN_CHUNK / 4) <= nvec) {
#pragma unroll
    for (int k = 0; k < GN_VEC_PER_THREAD; ++k) v[k] = body[q0 + k * GN_THREADS];
  } else {
#pragma unroll
    for (int k = 0; k < GN_VEC_PER_THREAD; ++k) {
      const long long q = q0 + k * GN_THREADS;
      v[k] = q < nvec ? body[q] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < GN_VEC_PER_THREAD; ++k) {
    acc = __builtin_fmaf(v[k].x, v[k].x, acc);
    acc = __builtin_fmaf(v[k].y, v[k].y, acc);
    acc = __builtin_fmaf(v[k].z, v[k].z, acc);
    acc = __builtin_fmaf(v[k].w, v[k].w, acc);
  }
  if (chunk == 0) {   // the tensor's first workgroup also takes the unaligned head and the tail (< 4 elements each)
    const int tail = (int)((n - head) & 3);
    const int t = threadIdx.x;
    if (t < head) {
      const float x = g[t];
      acc = __builtin_fmaf(x, x, acc);
    } else if (t >= 4 && t - 4 < tail) {
      const float x = g[head + nvec * 4 + (t - 4)];
      acc = __builtin_fmaf(x, x, acc);
    }
  }
  const float s = gn_block_sum(acc);
  if (threadIdx.x == 0) partial[a.slot0 + blockIdx.x] = s;
}

// clip_coef exactly as torch.nn.utils.clip_grad_norm_ evaluates `max_norm / (total_norm + 1e-6)` and clamps it: the
// scalar divided by a tensor is reciprocal-times-scalar, and clamp(max=1) lets a NaN through (an infinite norm gives 0).
__global__ __launch_bounds__(GN_THREADS) void grad_norm_finish_kernel(const float* __restrict__ partial, int count,
                                                                      float max_norm, float* __restrict__ out2) {
  float acc = 0.f;
  for (int i = threadIdx.x; i < count; i += GN_THREADS) acc += partial[i];
  const float s = gn_block_sum(acc);
  if (threadIdx.x == 0) {
    const float total = sqrtf(s);
    float inv = 1.0f / (total + 1e-6f);
    asm volatile("" : "+v"(inv));   // keep the two roundings apart
    const float coef = inv * max_norm;
    out2[0] = total;
    out2[1] = coef > 1.0f ? 1.0f : coef;
  }
}

int check_items(const qt_adam_item* items, int n, const char* who) {
  QT_CHECK_ARG(items && n > 0, "%s: no tensors", who);
  for (int j = 0; j < n; ++j)
    QT_CHECK_ARG(items[j].grad && items[j].numel > 0 && (reinterpret_cast<uintptr_t>(items[j].grad) & 3) == 0,
                 "%s: item %d: needs a 4-byte aligned gradient pointer and numel > 0", who, j);
  return QT_OK;
}

}  // namespace

extern "C" size_t qt_grad_norm_workspace_bytes(const qt_adam_item* items, int n) {
  if (check_items(items, n, "qt_grad_norm_workspace_bytes") != QT_OK) return 0;
  long long blocks = 0;
  for (int j = 0; j < n; ++j) blocks += gn_blocks(items[j].grad, items[j].numel);
  return (size_t)blocks * sizeof(float);
}

extern "C" int qt_grad_norm_multi(const qt_adam_item* items, int n, float max_norm, void* workspace, size_t workspace_bytes,
                                  float* out2, void* stream) {
  if (int st = check_items(items, n, "qt_grad_norm_multi")) return st;
  QT_CHECK_ARG(max_norm > 0.f, "qt_grad_norm_multi: max_norm must be positive (got %g)", (double)max_norm);   // NaN fails too
  QT_CHECK_ARG(workspace && out2, "qt_grad_norm_multi: null workspace / output");
  QT_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 3) == 0 && (reinterpret_cast<uintptr_t>(out2) & 3) == 0,
               "qt_grad_norm_multi: workspace and output must be 4-byte aligned");
  const size_t need = qt_grad_norm_workspace_bytes(items, n);
  QT_CHECK_ARG(workspace_bytes >= need, "qt_grad_norm_multi: workspace of %zu bytes, %zu needed (qt_grad_norm_workspace_bytes)",
               workspace_bytes, need);
  QT_CHECK_ARG(need / sizeof(float) <= (size_t)INT32_MAX, "qt_grad_norm_multi: too many elements for one call");
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* partial = static_cast<float*>(workspace);
  int slot0 = 0;
  for (int j0 = 0; j0 < n; j0 += GN_MAX_ITEMS) {
    GradNormArgs a;
    memset(&a, 0, sizeof(a));
    const int cnt = n - j0 < GN_MAX_ITEMS ? n - j0 : GN_MAX_ITEMS;
    int blocks = 0;
    for (int j = 0; j < cnt; ++j) {
      a.g[j] = items[j0 + j].grad;
      a.numel[j] = items[j0 + j].numel;
      a.first_block[j] = blocks;
      blocks += (int)gn_blocks(items[j0 + j].grad, items[j0 + j].numel);
    }
    a.first_block[cnt] = blocks;
    a.n = cnt;
    a.slot0 = slot0;
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(blocks), dim3(GN_THREADS), 0, s, a, partial);
    QT_CHECK_LAUNCH();
    slot0 += blocks;
  }
  hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(GN_THREADS), 0, s, partial, slot0, max_norm, out2);
  QT_CHECK_LAUNCH();
  return QT_OK;
}
