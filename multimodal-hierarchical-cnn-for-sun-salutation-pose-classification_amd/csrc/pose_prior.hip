// Learning the pose-order prior on the device, the parts that are not forward-backward: the hard counts of state paths
// (qt_pose_prior_count_paths) and the M-step (qt_pose_prior_update).  The E-step, qt_pose_prior_expect, extends the posterior's
// kernels and lives beside them in pose_posterior.hip; include/qtcnn.h states the rule in full.  The limits and the floor of a
// transition score (PC_MAX_S, PC_MAX_FRAMES, PC_TRANS_FLOOR) and the overlap check are pose_chain.h's.
// count_paths, two launches: (a) a workgroup of 256 per (stream, chunk of PR_CHUNK frames) counts its transitions
// path[f - 1] -> path[f] into an int histogram [S][S] in LDS (integer atomics on LDS: the result does not depend on their
// order) and writes it to the workspace; (b) one thread per entry adds the chunks of every stream in int64 and adds the sum, an
// exact integer, onto the double accumulator; the start counts are read off path[b][0] there.  No float atomics, no zero fill
// of caller memory, no workgroup waits for another; every slot of the workspace that is read has been written in the same call.
// update, one launch of one workgroup: thread i forms row i of the new table in double (log2 of the double library), thread S
// the new init, both by pose_chain.h's pc_update_row, which the learner of the chain with durations shares.
#include <stdint.h>

#include "pose_chain.h"

namespace {

constexpr int PR_CHUNK = 1024;                   // frames per workgroup of (a); a histogram entry stays below 2^10
constexpr int PR_THREADS = 256;

__global__ __launch_bounds__(PR_THREADS) void pr_count_kernel(const long long* __restrict__ path, int* __restrict__ partial, int T,
                                                              int chunks, int S) {
  __shared__ int hist[PC_MAX_S * PC_MAX_S];
  const int SS = S * S, tid = threadIdx.x;
  const int b = blockIdx.x / chunks, chunk = blockIdx.x - b * chunks;
  const int f0 = chunk * PR_CHUNK, f1 = min(f0 + PR_CHUNK, T);
  for (int idx = tid; idx < SS; idx += PR_THREADS) hist[idx] = 0;
  __syncthreads();
  const long long* __restrict__ p = path + (long long)b * T;
  for (int f = max(f0, 1) + tid; f < f1; f += PR_THREADS) {
    const long long from = p[f - 1], to = p[f];
    if (from >= 0 && from < S && to >= 0 && to < S) atomicAdd(&hist[(int)from * S + (int)to], 1);
  }
  __syncthreads();
  int* __restrict__ out = partial + (long long)blockIdx.x * SS;
  for (int idx = tid; idx < SS; idx += PR_THREADS) out[idx] = hist[idx];
}

__global__ __launch_bounds__(PR_THREADS) void pr_count_reduce_kernel(const long long* __restrict__ path,
                                                                     const int* __restrict__ partial, double* __restrict__ counts,
                                                                     double* __restrict__ start_counts,
                                                                     double* __restrict__ totals, int batch, int T, int chunks,
                                                                     int S) {
  const int SS = S * S, idx = blockIdx.x * PR_THREADS + threadIdx.x;
  if (idx < SS) {
    long long s = 0;
    for (long long k = 0; k < (long long)batch * chunks; ++k) s += partial[k * SS + idx];
    counts[idx] += (double)s;
  } else if (idx < SS + S) {
    long long s = 0;
    for (int b = 0; b < batch; ++b) s += path[(long long)b * T] == idx - SS;
    start_counts[idx - SS] += (double)s;
  } else if (idx == SS + S) {
    totals[1] += (double)batch * (double)T;
  }
}

__global__ __launch_bounds__(2 * PC_MAX_S) void pr_update_kernel(const double* __restrict__ counts,
                                                                 const double* __restrict__ start_counts,
                                                                 const int* __restrict__ allowed, double pseudo, const int* trans_in,
                                                                 const int* init_in, int* trans_out, int* init_out, int S) {
  const int i = threadIdx.x;   // (a row is read and written by its own thread alone: trans_out may be trans_in)
  if (i < S) pc_update_row(counts + i * S, allowed + i * S, pseudo, trans_in + i * S, trans_out + i * S, S);
  else if (i == S && init_out) pc_update_row(start_counts, nullptr, pseudo, init_in, init_out, S);
}

}  // namespace

extern "C" int qt_pose_prior_count_paths(const qt_pose_order_desc* desc, const long long* path, double* counts,
                                         double* start_counts, double* totals, void* workspace, long long workspace_bytes,
                                         void* stream) {
  const char* const who = "qt_pose_prior_count_paths";
  QT_CHECK_ARG(desc != nullptr, "%s: null descriptor", who);
  QT_CHECK_ARG(desc->batch >= 1, "%s: batch must be positive (got %d)", who, desc->batch);
  QT_CHECK_ARG(desc->frames >= 1, "%s: frames must be positive (got %d)", who, desc->frames);
  QT_CHECK_ARG(desc->num_states >= 1 && desc->num_states <= PC_MAX_S, "%s: num_states = %d; 1 .. %d are handled", who,
               desc->num_states, PC_MAX_S);
  const long long rows = (long long)desc->batch * desc->frames;
  if (rows > PC_MAX_FRAMES) {
    qt_set_error("%s: %lld frames in one call; at most %lld are handled", who, rows, PC_MAX_FRAMES);
    return QT_ERR_UNSUPPORTED;
  }
  const int B = desc->batch, T = desc->frames, S = desc->num_states, chunks = qt_cdiv(T, PR_CHUNK);
  QT_CHECK_ARG(path != nullptr && counts != nullptr && start_counts != nullptr && totals != nullptr, "%s: null %s", who,
               !path ? "path" : !counts ? "counts" : !start_counts ? "start_counts" : "totals");
  QT_CHECK_ARG(!misaligned(path, 7) && !misaligned(counts, 7) && !misaligned(start_counts, 7) && !misaligned(totals, 7) &&
                   !misaligned(workspace, 7),
               "%s: path, counts, start_counts, totals and the workspace must be 8-byte aligned", who);
  // the histograms, int32 [batch][chunks][S][S], take the front of what qt_pose_prior_workspace_bytes asks for (a chunk is
  // sixteen tiles); a descriptor whose num_classes that query would refuse needs them alone
  const long long own = (long long)B * chunks * S * S * 4, asked = qt_pose_prior_workspace_bytes(desc);
  const long long need = asked > own ? asked : own;
  QT_CHECK_ARG(workspace != nullptr && workspace_bytes >= need,
               "%s: workspace of %lld bytes; qt_pose_prior_workspace_bytes asks for %lld", who, workspace ? workspace_bytes : 0LL,
               need);
  const PcBuf in[] = {{path, (size_t)rows * 8, "path"}};
  const PcBuf out[] = {{counts, (size_t)S * S * 8, "counts"}, {start_counts, (size_t)S * 8, "start_counts"},
                       {totals, 16, "totals"}, {workspace, (size_t)need, "workspace"}};
  if (const int rc = pc_check_disjoint(who, in, out)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  int* partial = static_cast<int*>(workspace);
  hipLaunchKernelGGL(pr_count_kernel, dim3((unsigned)(B * chunks)), dim3(PR_THREADS), 0, s, path, partial, T, chunks, S);
  QT_CHECK_LAUNCH();
  hipLaunchKernelGGL(pr_count_reduce_kernel, dim3((unsigned)qt_cdiv(S * S + S + 1, PR_THREADS)), dim3(PR_THREADS), 0, s, path,
                     (const int*)partial, counts, start_counts, totals, B, T, chunks, S);
  QT_CHECK_LAUNCH();
  return QT_OK;
}

extern "C" int qt_pose_prior_update(int num_states, const double* counts, const double* start_counts, const int* allowed,
                                    double pseudo_count, const int* trans_in, const int* init_in, int* trans_out, int* init_out,
                                    void* stream) {
  const char* const who = "qt_pose_prior_update";
  const int S = num_states;
  QT_CHECK_ARG(S >= 1 && S <= PC_MAX_S, "%s: num_states = %d; 1 .. %d are handled", who, S, PC_MAX_S);
  QT_CHECK_ARG(pseudo_count >= 0.0 && pseudo_count <= 1.7976931348623157e308,
               "%s: pseudo_count must be a finite number that is not negative (got %g)", who, pseudo_count);
  QT_CHECK_ARG(counts != nullptr && allowed != nullptr && trans_in != nullptr && trans_out != nullptr, "%s: null %s", who,
               !counts ? "counts" : !allowed ? "allowed" : !trans_in ? "trans_in" : "trans_out");
  QT_CHECK_ARG(init_out == nullptr || start_counts != nullptr, "%s: null start_counts with an init_out", who);
  QT_CHECK_ARG(!misaligned(counts, 7) && !misaligned(start_counts, 7) && !misaligned(allowed, 3) && !misaligned(trans_in, 3) &&
                   !misaligned(init_in, 3) && !misaligned(trans_out, 3) && !misaligned(init_out, 3),
               "%s: counts and start_counts must be 8-byte aligned, allowed, trans_in, init_in, trans_out and init_out 4-byte", who);
  const size_t tb = (size_t)S * S * 4, ib = (size_t)S * 4;
  const PcBuf in[] = {
      {counts, 2 * tb, "counts"}, {start_counts, 2 * ib, "start_counts"}, {allowed, tb, "allowed"},
      {trans_in, tb, "trans_in"}, {init_in, ib, "init_in"}},
    out[] = {{trans_out, tb, "trans_out"}, {init_out, ib, "init_out"}};
  for (const auto& o : out)
    for (const auto& i : in) {
      const bool in_place = (o.p == trans_out && i.p == trans_in && trans_out == trans_in) ||
                            (o.p == init_out && i.p == init_in && init_out == init_in);
      QT_CHECK_ARG(in_place || !overlap(o.p, o.bytes, i.p, i.bytes),
                   "%s: %s must not overlap %s (trans_out may be trans_in itself, init_out init_in itself)", who, o.name, i.name);
    }
  QT_CHECK_ARG(!overlap(trans_out, tb, init_out, ib), "%s: trans_out must not overlap init_out", who);
  hipLaunchKernelGGL(pr_update_kernel, dim3(1), dim3(2 * PC_MAX_S), 0, static_cast<hipStream_t>(stream), counts, start_counts,
                     allowed, pseudo_count, trans_in, init_in, trans_out, init_out, S);
  QT_CHECK_LAUNCH();
  return QT_OK;
}
