// Pose-order posteriors with hold durations (qt_pose_duration_posterior): the marginals of the explicit-duration (semi-Markov)
// chain that qt_pose_duration_decode maximises, by forward-backward over segments, and the expected duration counts that fit
// its table.  include/qtcnn.h states the rule in full; the reference has no such step.  pose_chain.h supplies the limits, the
// emission rule and the buffer checks; pose_duration_chain.h the chain's inputs PcDurChain, the descriptor check, the seven
// inputs as a list and the stream kernel's launch.
//
// The stream kernel, one workgroup per stream walking a forward and a backward sweep, is pose_duration_sweep.h's, which states
// the walk; the learner's E-step (pose_duration_prior.hip) runs the same kernel in its second mode.  A stream's [S][D] partial
// counts go to the workspace; pp_counts_kernel adds the streams' partials in ascending stream order, from zero, onto dur_counts.
// No workgroup waits for another, no atomics, no host synchronisation; every workspace slot that is read has been written in
// the same call (a workgroup reads its own stores behind barriers).
#include "pose_chain.h"
#include "pose_duration_chain.h"
#include "pose_duration_sweep.h"

namespace {

// dur_counts[idx] += the streams' partials in ascending stream order, from zero
__global__ __launch_bounds__(PC_DUR_THREADS) void pp_counts_kernel(const double* __restrict__ part, double* counts, int batch,
                                                                   int n) {
  const int idx = blockIdx.x * PC_DUR_THREADS + threadIdx.x;
  if (idx >= n) return;
  double s = 0.0;
  for (int b = 0; b < batch; ++b) s += part[(long long)b * n + idx];
  counts[idx] += s;
}

}  // namespace

extern "C" long long qt_pose_duration_posterior_workspace_bytes(const qt_pose_duration_desc* desc) {
  if (pc_duration_check_desc("qt_pose_duration_posterior_workspace_bytes", desc) != QT_OK) return 0;
  return pp_workspace_bytes(desc);
}

extern "C" int qt_pose_duration_posterior(const qt_pose_duration_desc* desc, const float* probs, long long ld,
                                          const int* state_class, const int* trans, const int* init, const int* dur,
                                          const int* dur_open, const int* lengths, float* posterior, float* class_posterior,
                                          float* begin, double* log2_evidence, double* dur_counts, void* workspace,
                                          long long workspace_bytes, void* stream) {
  const char* const who = "qt_pose_duration_posterior";
  if (const int rc = pc_duration_check_desc(who, desc)) return rc;
  const int B = desc->batch, T = desc->frames, C = desc->num_classes, S = desc->num_states, D = desc->max_duration;
  QT_CHECK_ARG(ld >= C, "%s: row stride ld = %lld < C = %d", who, ld, C);
  const long long need = pp_workspace_bytes(desc), rows = (long long)B * T;
  const PcDurInputs in =
      pc_dur_inputs(probs, rows, ld, C, S, D, state_class, trans, init, dur, dur_open, {lengths, (size_t)B * 4, "lengths", 3});
  const PcBuf out[] = {{posterior, (size_t)rows * S * 4, "posterior", 3}, {class_posterior, (size_t)rows * C * 4, "class_posterior", 3},
                       {begin, (size_t)rows * S * 4, "begin", 3}, {log2_evidence, (size_t)B * 8, "log2_evidence", 7},
                       {dur_counts, (size_t)S * D * 8, "dur_counts", 7}, {workspace, (size_t)need, "workspace", 7}};
  if (const int rc = pc_check_present(who, in.v, out)) return rc;
  QT_CHECK_ARG(posterior != nullptr || dur_counts != nullptr, "%s: null posterior and null dur_counts; one of them is required",
               who);
  if (const int rc = pc_check_layout(who, in.v, out,
                                     {workspace, workspace_bytes, need, "qt_pose_duration_posterior_workspace_bytes asks for %lld"}))
    return rc;

  PpArgs a;
  pc_dur_fill(a, probs, ld, state_class, trans, init, dur, dur_open, lengths, T, C, S, D);
  a.posterior = posterior;
  a.class_posterior = class_posterior;
  a.begin = begin;
  a.evidence = log2_evidence;
  a.g = static_cast<double*>(workspace);
  a.al = a.g + pp_level_elems(desc);
  a.part = dur_counts ? a.al + pp_level_elems(desc) : nullptr;
  a.xi_part = a.start_part = a.z_part = nullptr;
  if (const int rc = pc_launch_stream<pp_stream_kernel<true, false>, pp_stream_kernel<false, false>>(
          S, pp_lds_bytes(S, D), pp_lds_bytes(PC_MAX_S, PC_MAX_D), B, stream, a))
    return rc;
  if (dur_counts) {
    hipLaunchKernelGGL(pp_counts_kernel, dim3((unsigned)qt_cdiv((long long)S * D, PC_DUR_THREADS)), dim3(PC_DUR_THREADS), 0,
                       static_cast<hipStream_t>(stream), a.part, dur_counts, B, S * D);
    QT_CHECK_LAUNCH();
  }
  return QT_OK;
}
