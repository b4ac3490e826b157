// Pose-order posteriors with hold durations (qt_pose_duration_posterior): the marginals of the explicit-duration (semi-Markov)
// chain that qt_pose_duration_decode maximises, by forward-backward over segments, and the expected duration counts that fit
// its table.  include/qtcnn.h states the rule in full; the reference has no such step.  pose_chain.h supplies the limits, the
// emission rule, the chain's inputs PcChain, the descriptor and overlap checks and the S <= 16 switch.
//
// The stream kernel, one workgroup per stream walking a forward and a backward sweep, is pose_duration_sweep.h's, which states
// the walk; the learner's E-step (pose_duration_prior.hip) runs the same kernel in its second mode.  A stream's [S][D] partial
// counts go to the workspace; pp_counts_kernel adds the streams' partials in ascending stream order, from zero, onto dur_counts.
// No workgroup waits for another, no atomics, no host synchronisation; every workspace slot that is read has been written in
// the same call (a workgroup reads its own stores behind barriers).
#include "pose_chain.h"
#include "pose_duration_sweep.h"

namespace {

// dur_counts[idx] += the streams' partials in ascending stream order, from zero
__global__ __launch_bounds__(PP_THREADS) void pp_counts_kernel(const double* __restrict__ part, double* counts, int batch, int n) {
  const int idx = blockIdx.x * PP_THREADS + threadIdx.x;
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
  QT_CHECK_ARG(probs != nullptr && state_class != nullptr && trans != nullptr && dur != nullptr, "%s: null %s", who,
               !probs ? "probs" : !state_class ? "state_class" : !trans ? "trans" : "dur");
  QT_CHECK_ARG(posterior != nullptr || dur_counts != nullptr, "%s: null posterior and null dur_counts; one of them is required",
               who);
  QT_CHECK_ARG(!misaligned(probs, 3) && !misaligned(state_class, 3) && !misaligned(trans, 3) && !misaligned(init, 3) &&
                   !misaligned(dur, 3) && !misaligned(dur_open, 3) && !misaligned(lengths, 3) && !misaligned(posterior, 3) &&
                   !misaligned(class_posterior, 3) && !misaligned(begin, 3) && !misaligned(log2_evidence, 7) &&
                   !misaligned(dur_counts, 7) && !misaligned(workspace, 7),
               "%s: probs, state_class, trans, init, dur, dur_open, lengths, posterior, class_posterior and begin must be "
               "4-byte aligned, log2_evidence, dur_counts and the workspace 8-byte", who);
  const long long need = pp_workspace_bytes(desc);
  QT_CHECK_ARG(workspace != nullptr && workspace_bytes >= need,
               "%s: workspace of %lld bytes; qt_pose_duration_posterior_workspace_bytes asks for %lld", who,
               workspace ? workspace_bytes : 0LL, need);
  const long long rows = (long long)B * T;
  const PcBuf in[] = {{probs, (size_t)((rows - 1) * ld + C) * 4, "probs"}, {state_class, (size_t)S * 4, "state_class"},
                      {trans, (size_t)S * S * 4, "trans"}, {init, (size_t)S * 4, "init"}, {dur, (size_t)S * D * 4, "dur"},
                      {dur_open, (size_t)S * D * 4, "dur_open"}, {lengths, (size_t)B * 4, "lengths"}};
  const PcBuf out[] = {{posterior, (size_t)rows * S * 4, "posterior"}, {class_posterior, (size_t)rows * C * 4, "class_posterior"},
                       {begin, (size_t)rows * S * 4, "begin"}, {log2_evidence, (size_t)B * 8, "log2_evidence"},
                       {dur_counts, (size_t)S * D * 8, "dur_counts"}, {workspace, (size_t)need, "workspace"}};
  if (const int rc = pc_check_disjoint(who, in, out)) return rc;

  PpArgs a;
  pc_fill(a, probs, ld, state_class, trans, init, T, C, S);
  a.dur = dur;
  a.dur_open = dur_open ? dur_open : dur;
  a.lengths = lengths;
  a.posterior = posterior;
  a.class_posterior = class_posterior;
  a.begin = begin;
  a.evidence = log2_evidence;
  a.g = static_cast<double*>(workspace);
  a.al = a.g + pp_level_elems(desc);
  a.part = dur_counts ? a.al + pp_level_elems(desc) : nullptr;
  a.xi_part = a.start_part = a.z_part = nullptr;
  a.D = D;
  const size_t lds = pp_lds_bytes(S, D);
  const bool small = S <= 16;
  static std::atomic<unsigned long long> raised[2] = {{0}, {0}};
  if (lds > 64 * 1024)
    if (const int rc = qt_raise_lds_limit(reinterpret_cast<const void*>(small ? pp_stream_kernel<true, false> : pp_stream_kernel<false, false>),
                                          (int)pp_lds_bytes(PC_MAX_S, PP_MAX_D), raised[small]))
      return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  pc_by_small(S, [&](auto sm) {
    hipLaunchKernelGGL((pp_stream_kernel<PC_SMALL(sm), false>), dim3((unsigned)B), dim3(PP_THREADS), lds, s, a);
  });
  QT_CHECK_LAUNCH();
  if (dur_counts) {
    hipLaunchKernelGGL(pp_counts_kernel, dim3((unsigned)qt_cdiv((long long)S * D, PP_THREADS)), dim3(PP_THREADS), 0, s, a.part,
                       dur_counts, B, S * D);
    QT_CHECK_LAUNCH();
  }
  return QT_OK;
}
