// Functions defined in one .hip file and called from another.  Both the defining and the calling file include this
// header, so a changed signature is a compile error in either; no .hip file declares another file's function itself.
#pragma once
#include "conv_args.h"

// conv_pt.hip (3x3 stride-1 convolutions of the 28x28 / 14x14 / 7x7 stages: input patch resident in LDS, ping-pong MFMA
// schedule): does it take this problem, how many statistics rows (= pixel tiles) it writes, and its launch
bool qt_pt_eligible(const qtc::ConvArgs& a, int dtype, bool dgrad);
int qt_pt_stats_rows(const qtc::ConvArgs& a, bool dgrad);
int qt_pt_launch(const qtc::ConvArgs& a, int dtype, bool dgrad, hipStream_t stream);

// conv_patch.hip: 3x3 stride-1 convs of the 56x56 / 28x28 stages with the input patch held in LDS
bool qt_patch_eligible(const qt_conv_desc* d);
int qt_patch_stats_rows(const qt_conv_desc* d);
int qt_patch_launch(const qt_conv_desc* d, const qt_conv_io* io, void* stream);

// conv_stem.hip: the packed 7x7/2 stem convolution (bf16) with its input rows held in LDS
bool qt_stem_eligible(const qt_conv_desc* d, const qt_conv_io* io);
int qt_stem_stats_rows(const qt_conv_desc* d);
int qt_stem_launch(const qt_conv_desc* d, const qt_conv_io* io, void* stream);

// Weight gradients.  `sum_stream`: the stream the fixed-order sum of the partial filters runs on, ordered behind the
// kernel on `stream` by an event; nullptr = the kernel's own stream.
// conv_wgrad_patch.hip: streaming kernels for 3x3 / stride 1 / pad 1 (bf16).  oihw 0: dw [O][9][I] accumulated into,
// 1: written as OIHW (needs the workspace)
bool qt_wgrad_patch_eligible(const qt_conv_desc* d);
size_t qt_wgrad_patch_workspace_bytes(const qt_conv_desc* d);
int qt_wgrad_patch_launch(const qt_conv_desc* d, const void* dy, const void* x, float* dw, void* workspace,
                          size_t workspace_bytes, int oihw, void* stream, void* sum_stream);
// dw = sum over `nsplit` ranges of part[range][filt] in a fixed order.  layout 0: added to dw ([O][taps][I]);
// 1: j = (n*9 + tap)*KC + c written to OIHW element (n*KC + c)*9 + tap; 2: written as is ([N][1][KC] is OIHW already)
int qt_wgrad_partial_sum_launch(const float* part, float* dw, size_t filt, int nsplit, int KC, int layout, hipStream_t stream,
                                hipStream_t sum_stream);
// conv_wgrad_s2.hip: the stride-2 convolutions of a transition block (3x3 / 2 pad 1, 1x1 / 2) on parity planes (bf16);
// grad_oihw is written, not accumulated
bool qt_wgrad_s2_eligible(const qt_conv_desc* d);
size_t qt_wgrad_s2_workspace_bytes(const qt_conv_desc* d);
int qt_wgrad_s2_launch(const qt_conv_desc* d, const void* dy, const void* x, float* grad_oihw, void* workspace,
                       size_t workspace_bytes, void* stream, void* sum_stream);
