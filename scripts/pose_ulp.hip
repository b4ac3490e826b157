// The device's atan2f and sqrtf on given arguments (developer aid of scripts/measure_pose_ulp.py, not part of the library):
//   pose_ulp <in> <out>     in: int32 n, int32 m, f32 y[n], x[n], q[m];   out: f32 atan2f(y, x)[n], sqrtf(q)[m]
// Built with the library's compiler flags (csrc/Makefile), so the functions are the ones csrc/pose.hip gets.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#define CHECK(call)                                                              \
  do {                                                                           \
    hipError_t e_ = (call);                                                      \
    if (e_ != hipSuccess) {                                                      \
      fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); \
      return 1;                                                                  \
    }                                                                            \
  } while (0)

__global__ void eval_kernel(const float* y, const float* x, const float* q, float* at, float* sq, int n, int m) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) at[i] = atan2f(y[i], x[i]);
  if (i < m) sq[i] = sqrtf(q[i]);
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: pose_ulp <in> <out>\n");
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  int nm[2];
  if (!f || fread(nm, sizeof(int), 2, f) != 2 || nm[0] < 1 || nm[1] < 1) {
    fprintf(stderr, "pose_ulp: cannot read %s\n", argv[1]);
    return 2;
  }
  const int n = nm[0], m = nm[1];
  std::vector<float> in(2 * (size_t)n + m), out((size_t)n + m);
  if (fread(in.data(), sizeof(float), in.size(), f) != in.size()) {
    fprintf(stderr, "pose_ulp: %s is short\n", argv[1]);
    return 2;
  }
  fclose(f);
  float *din = nullptr, *dout = nullptr;
  CHECK(hipMalloc(&din, in.size() * sizeof(float)));
  CHECK(hipMalloc(&dout, out.size() * sizeof(float)));
  CHECK(hipMemcpy(din, in.data(), in.size() * sizeof(float), hipMemcpyHostToDevice));
  const int top = n > m ? n : m;
  hipLaunchKernelGGL(eval_kernel, dim3((top + 255) / 256), dim3(256), 0, 0, din, din + n, din + 2 * (size_t)n, dout, dout + n, n, m);
  CHECK(hipGetLastError());
  CHECK(hipMemcpy(out.data(), dout, out.size() * sizeof(float), hipMemcpyDeviceToHost));
  CHECK(hipFree(din));
  CHECK(hipFree(dout));
  f = fopen(argv[2], "wb");
  if (!f || fwrite(out.data(), sizeof(float), out.size(), f) != out.size()) {
    fprintf(stderr, "pose_ulp: cannot write %s\n", argv[2]);
    return 2;
  }
  fclose(f);
  return 0;
}
