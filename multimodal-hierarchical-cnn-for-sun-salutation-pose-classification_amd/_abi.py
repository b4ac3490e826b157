"""The C ABI of libqtcnn_hip.so (include/qtcnn.h) as ctypes sees it: every struct mirror, one signature table, bind().

This is the only place that subclasses ctypes.Structure or sets argtypes / restype.  tests/test_abi_cpu.py parses the
header and compares it with the table (names, arity, types) and compiles a C program that prints sizeof / offsetof of
every struct for comparison with the mirrors, so a prototype or a field changed in qtcnn.h and forgotten here fails a
CPU test instead of shifting an argument.

Type mapping: int, long long, unsigned long long, size_t, float and double map directly; `const char*` (parameter or
return) is c_char_p; a void return is None; EVERY other pointer is c_void_p, which accepts None, Python ints,
c_void_p, byref(...), ctypes arrays and pointers alike.

`<module>.bind` of the modules that wrap one group of entry points (loss, metrics, pose_order, ...) and
`engine._bind_api` are this module's bind().
"""
import ctypes

I, LL, ULL, SZ, F, D = (ctypes.c_int, ctypes.c_longlong, ctypes.c_ulonglong, ctypes.c_size_t, ctypes.c_float,
                        ctypes.c_double)
P, S, UB = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_ubyte


class QtError(RuntimeError):
    pass


# ---- struct mirrors, in header order ----------------------------------------------------------------------------

class ConvDesc(ctypes.Structure):   # qt_conv_desc
    _fields_ = [("dtype", I), ("mode", I), ("batch", I), ("in_h", I), ("in_w", I), ("out_h", I), ("out_w", I),
                ("k_per_tap", I), ("n_out", I), ("kh", I), ("kw", I), ("stride", I), ("pad", I),
                ("src_img_stride", LL), ("src_row_stride", I), ("src_pix_stride", I), ("quad", I), ("relu", I),
                ("dst_sub", I), ("dst_h", I), ("dst_w", I), ("dst_off_h", I), ("dst_off_w", I), ("dst_merge", I),
                ("dst_merge_res0", I), ("kt", I), ("frames", I), ("dst_merge_extra", I)]


class ConvIO(ctypes.Structure):   # qt_conv_io
    _fields_ = [("src", P), ("weight", P), ("dst", P), ("scale", P), ("shift", P), ("residual", P),
                ("relu_mask", P), ("stats_partial", P), ("bn0_y", P), ("bn0_mean", P), ("bn0_invstd", P),
                ("bn0_partial", P), ("bn1_y", P), ("bn1_mean", P), ("bn1_invstd", P), ("bn1_partial", P),
                ("relu_mask_bits", P), ("extra_src", P)]


class ConvS2Desc(ctypes.Structure):   # qt_conv_s2_desc
    _fields_ = [("dtype", I), ("batch", I), ("in_h", I), ("in_w", I), ("c_in", I), ("c_out", I), ("relu_conv", I),
                ("relu_down", I)]


class ConvS2IO(ctypes.Structure):   # qt_conv_s2_io
    _fields_ = [("src", P), ("w_conv", P), ("w_down", P), ("y_conv", P), ("y_down", P), ("scale_conv", P),
                ("shift_conv", P), ("scale_down", P), ("shift_down", P), ("stats_conv", P), ("stats_down", P)]


class PackItem(ctypes.Structure):   # qt_pack_item
    _fields_ = [("w_oihw", P), ("w_fwd", P), ("w_dgrad", P), ("O", I), ("I", I), ("k", I), ("stride2_dgrad", I)]


class AdamDesc(ctypes.Structure):   # qt_adam_desc
    _fields_ = [("lr", F), ("beta1", F), ("beta2", F), ("eps", F), ("weight_decay", F), ("grad_scale", F),
                ("step", I)]


class AdamItem(ctypes.Structure):   # qt_adam_item
    _fields_ = [("param", P), ("grad", P), ("exp_avg", P), ("exp_avg_sq", P), ("numel", LL)]


class LossDesc(ctypes.Structure):   # qt_loss_desc
    _fields_ = [("dtype", I), ("kind", I), ("reduction", I), ("ignore_index", LL), ("label_smoothing", F),
                ("gamma", F), ("class_weight", P)]


class PreprocessDesc(ctypes.Structure):   # qt_preprocess_desc
    _fields_ = [("batch", I), ("src_h", I), ("src_w", I), ("src_row_stride", LL), ("src_image_stride", LL),
                ("out_h", I), ("out_w", I), ("bgr", I), ("mean", F * 3), ("inv_std", F * 3)]


class AugmentDesc(ctypes.Structure):   # qt_augment_desc
    _fields_ = [("batch", I), ("h", I), ("w", I), ("src_image_stride", LL), ("dst_image_stride", LL),
                ("blur_kx", I), ("blur_ky", I), ("mean", F * 3), ("inv_std", F * 3), ("use_contrast", I)]


class PoseDesc(ctypes.Structure):   # qt_pose_desc
    _fields_ = [("rows", LL), ("mode", I), ("rows_per_label", I), ("num_classes", I)]


class PoseSeqDesc(ctypes.Structure):   # qt_pose_seq_desc
    _fields_ = [("batch", I), ("frames", I), ("width", I), ("height", I), ("mode", I)]


class SeqWindowsDesc(ctypes.Structure):   # qt_seq_windows_desc
    _fields_ = [("frames", I), ("clips", I), ("seq_len", I), ("stride", I), ("num_classes", I), ("capacity", I),
                ("rule", I)]


class SeqGatherDesc(ctypes.Structure):   # qt_seq_gather_desc
    _fields_ = [("src_rows", LL), ("row_bytes", LL), ("windows", I), ("seq_len", I)]


class SeqFeaturesDesc(ctypes.Structure):   # qt_seq_features_desc
    _fields_ = [("src_rows", LL), ("features", I), ("windows", I), ("seq_len", I), ("mode", I), ("num_classes", I)]


class MetricsDesc(ctypes.Structure):   # qt_metrics_desc
    _fields_ = [("dtype", I), ("ignore_index", LL)]


class ScoresDesc(ctypes.Structure):   # qt_scores_desc
    _fields_ = [("dtype", I), ("kind", I), ("bits", I), ("cal_bins", I), ("route", I), ("ignore_index", LL)]


class AnnotateDesc(ctypes.Structure):   # qt_annotate_desc
    _fields_ = [("batch", I), ("H", I), ("W", I), ("n_segments", I), ("min_visibility", F), ("thick_major", I),
                ("thick_minor", I), ("radius_hi", I), ("radius_lo", I), ("line_hi", UB * 3), ("line_lo", UB * 3),
                ("point_hi", UB * 3), ("point_lo", UB * 3), ("num_classes", I), ("glyph_h", I), ("glyph_w", I),
                ("ox", I), ("oy", I), ("caption_colour", UB * 3)]


class TimelineDesc(ctypes.Structure):   # qt_timeline_desc
    _fields_ = [("batch", I), ("frames", I), ("num_classes", I), ("window", I), ("min_run", I),
                ("min_confidence", F), ("capacity", I), ("flush", I)]


class SegmentsDesc(ctypes.Structure):   # qt_segments_desc
    _fields_ = [("batch", I), ("frames", I), ("num_classes", I), ("num_thresholds", I), ("pct", I * 8),
                ("capacity", I)]


class PoseOrderDesc(ctypes.Structure):   # qt_pose_order_desc
    _fields_ = [("batch", I), ("frames", I), ("num_classes", I), ("num_states", I)]


class PoseLagDesc(ctypes.Structure):   # qt_pose_lag_desc
    _fields_ = [("batch", I), ("frames", I), ("num_classes", I), ("num_states", I), ("lag", I), ("flush", I),
                ("seen", LL)]


class PoseDurationDesc(ctypes.Structure):   # qt_pose_duration_desc
    _fields_ = [("batch", I), ("frames", I), ("num_classes", I), ("num_states", I), ("max_duration", I)]


class PoseDurationLagDesc(ctypes.Structure):   # qt_pose_duration_lag_desc
    _fields_ = [("batch", I), ("frames", I), ("num_classes", I), ("num_states", I), ("max_duration", I), ("lag", I),
                ("flush", I), ("seen", LL)]


class BnEvalItem(ctypes.Structure):   # qt_bn_eval_item
    _fields_ = [("gamma", P), ("beta", P), ("running_mean", P), ("running_var", P), ("scale", P), ("shift", P),
                ("C", I), ("mean", P), ("invstd", P)]


class GemmSmallDesc(ctypes.Structure):   # qt_gemm_small_desc
    _fields_ = [("M", I), ("N", I), ("K", I), ("a_dtype", I), ("b_dtype", I), ("c_dtype", I), ("a_row_stride", LL),
                ("a_k_stride", LL), ("b_row_stride", LL), ("b_k_stride", LL), ("c_row_stride", LL), ("relu", I),
                ("accumulate", I)]


class PlanDesc(ctypes.Structure):   # qt_plan_desc
    _fields_ = [("dtype", I), ("batch", I), ("num_classes", I), ("model", I), ("mode", I), ("numerical_dim", I),
                ("dropout_p", F), ("bn_eps", F), ("bn_momentum", F), ("seq_len", I), ("lstm_hidden", I)]


# ---- name -> (restype, [argtypes]) for all entry points of qtcnn.h, in header order ----------------------------

SIGNATURES = {
    "qt_version": (I, []),
    "qt_last_error": (S, []),
    "qt_set_patch_conv": (None, [I]),
    "qt_set_pt_conv": (None, [I]),
    "qt_set_pt_conv_max_workgroups": (None, [I]),
    "qt_set_stem_conv": (None, [I]),
    "qt_conv2d_stats_rows": (I, [P]),
    "qt_conv_s2_pair_supported": (I, [P]),
    "qt_conv_s2_pair_stats_rows": (I, [P]),
    "qt_conv_s2_pair": (I, [P, P, P]),
    "qt_set_conv_s2": (None, [I]),
    "qt_set_conv_s2_max_workgroups": (None, [I]),
    "qt_conv2d_igemm": (I, [P, P, P]),
    "qt_conv2d_wgrad": (I, [P, P, P, P, P]),
    "qt_linear_wgrad": (I, [I, P, P, P, I, I, I, P]),
    "qt_conv2d_wgrad_workspace_bytes": (SZ, [P]),
    "qt_conv2d_wgrad_ws": (I, [P, P, P, P, P, SZ, P]),
    "qt_conv2d_wgrad_oihw": (I, [P, P, P, P, P, SZ, P]),
    "qt_conv2d_wgrad_oihw_on": (I, [P, P, P, P, P, SZ, P, P]),
    "qt_set_wgrad_patch_min_width": (None, [I]),
    "qt_set_wgrad_patch_variant": (None, [I]),
    "qt_set_wgrad_s2": (None, [I]),
    "qt_pack_stem_input": (I, [I, P, P, I, P]),
    "qt_pack_conv_weight": (I, [I, P, P, P, I, I, I, I, P]),
    "qt_pack_weights_batched": (I, [I, P, I, P]),
    "qt_adam_multi": (I, [P, I, P, P]),
    "qt_adam_pack_weights_batched": (I, [I, P, P, P, I, P]),
    "qt_adam_multi_scaled": (I, [P, I, P, P, P]),
    "qt_adam_pack_weights_batched_scaled": (I, [I, P, P, P, P, I, P]),
    "qt_grad_norm_workspace_bytes": (SZ, [P, I]),
    "qt_grad_norm_multi": (I, [P, I, F, P, SZ, P, P]),
    "qt_loss_workspace_bytes": (SZ, [LL, I]),
    "qt_loss_forward": (I, [P, P, LL, P, LL, I, P, P, P, P, P, P, SZ, P]),
    "qt_loss_backward": (I, [P, P, LL, P, LL, I, P, P, P, P, LL, P]),
    "qt_preprocess_u8": (I, [P, P, P, P, P, LL, P]),
    "qt_augment_workspace_bytes": (SZ, [I, I]),
    "qt_augment_f32": (I, [P, P, P, P, P, SZ, P]),
    "qt_gradcam_workspace_bytes": (SZ, [I, I, I]),
    "qt_gradcam_map": (I, [P, P, I, I, I, P, P, P, SZ, P]),
    "qt_gradcam_overlay_u8": (I, [P, I, I, P, I, I, I, P, F, P, P, P, P]),
    "qt_pose_features": (I, [P, P, P, P, P, P, P, P, P]),
    "qt_pose_sequence_features": (I, [P, P, P, P, P, P, P, P, P, P]),
    "qt_seq_windows_workspace_bytes": (SZ, [P]),
    "qt_seq_windows_plan": (I, [P, P, P, P, P, P, P, SZ, P]),
    "qt_seq_gather_rows": (I, [P, P, P, P, P]),
    "qt_seq_gather_features": (I, [P, P, P, P, P, P, P, P]),
    "qt_metrics_state_bytes": (SZ, [I]),
    "qt_metrics_report_bytes": (SZ, [I]),
    "qt_metrics_update": (I, [P, P, LL, P, P, LL, I, P, P, LL, P, P, P]),
    "qt_metrics_finalize": (I, [P, I, P, P]),
    "qt_scores_state_bytes": (SZ, [I, I, I]),
    "qt_scores_report_bytes": (SZ, [I, I]),
    "qt_scores_update": (I, [P, P, LL, P, LL, I, P, P]),
    "qt_scores_finalize": (I, [P, I, I, I, P, P, P]),
    "qt_annotate_u8": (I, [P, P, P, P, P, P, P, P, P, P, P]),
    "qt_timeline_smooth": (I, [P, P, LL, P, P, P, P, P, LL, P, P, P]),
    "qt_timeline_decode": (I, [P, P, P, P, P, P, P]),
    "qt_segments_workspace_bytes": (SZ, [P]),
    "qt_segments_update": (I, [P, P, LL, P, LL, P, P, P, P, SZ, P]),
    "qt_segments_encode": (I, [P, P, LL, P, P, P, P]),
    "qt_pose_order_workspace_bytes": (LL, [P]),
    "qt_pose_order_decode": (I, [P, P, LL, P, P, P, P, P, P, P, P, LL, P]),
    "qt_pose_posterior_workspace_bytes": (LL, [P]),
    "qt_pose_posterior": (I, [P, P, LL, P, P, P, P, P, P, P, P, P, LL, P]),
    "qt_pose_prior_workspace_bytes": (LL, [P]),
    "qt_pose_prior_expect": (I, [P, P, LL, P, P, P, P, P, P, P, LL, P]),
    "qt_pose_prior_count_paths": (I, [P, P, P, P, P, P, LL, P]),
    "qt_pose_prior_update": (I, [I, P, P, P, D, P, P, P, P, P]),
    "qt_pose_lag_smooth_carry_bytes": (LL, [P]),
    "qt_pose_lag_smooth_workspace_bytes": (LL, [P]),
    "qt_pose_lag_smooth": (I, [P, P, LL, P, P, P, P, P, P, P, P, P, P, LL, P]),
    "qt_pose_lag_decode_carry_bytes": (LL, [P]),
    "qt_pose_lag_decode_workspace_bytes": (LL, [P]),
    "qt_pose_lag_decode": (I, [P, P, LL, P, P, P, P, P, P, P, P, LL, P]),
    "qt_pose_duration_workspace_bytes": (LL, [P]),
    "qt_pose_duration_decode": (I, [P, P, LL, P, P, P, P, P, P, P, P, P, P, LL, P]),
    "qt_pose_duration_count": (I, [P, P, LL, P, P, P]),
    "qt_pose_duration_posterior_workspace_bytes": (LL, [P]),
    "qt_pose_duration_posterior": (I, [P, P, LL, P, P, P, P, P, P, P, P, P, P, P, P, LL, P]),
    "qt_pose_duration_prior_workspace_bytes": (LL, [P]),
    "qt_pose_duration_prior_expect": (I, [P, P, LL, P, P, P, P, P, P, P, P, P, P, P, LL, P]),
    "qt_pose_duration_prior_count_paths": (I, [P, P, P, LL, P, P, P, P, P, P, LL, P]),
    "qt_pose_duration_prior_update": (I, [I, I, P, P, P, P, P, D, D, P, P, P, P, P, P, P, P]),
    "qt_pose_duration_lag_carry_bytes": (LL, [P]),
    "qt_pose_duration_lag_workspace_bytes": (LL, [P]),
    "qt_pose_duration_lag_decode": (I, [P, P, LL, P, P, P, P, P, P, P, P, P, P, P, P, LL, P]),
    "qt_pose_duration_lag_smooth_carry_bytes": (LL, [P]),
    "qt_pose_duration_lag_smooth_workspace_bytes": (LL, [P]),
    "qt_pose_duration_lag_smooth": (I, [P, P, LL, P, P, P, P, P, P, P, P, P, P, P, P, P, LL, P]),
    "qt_pack_dgrad_s2": (I, [I, P, P, I, I, I, P, P, P, P]),
    "qt_pack_dgrad_s2_merged": (I, [I, P, P, I, I, P]),
    "qt_pack_stem_weight": (I, [I, P, P, I, P]),
    "qt_unpack_conv_wgrad": (I, [P, P, I, I, I, I, I, P]),
    "qt_unpack_stem_wgrad": (I, [P, P, I, P]),
    "qt_stats_capacity_rows": (I, [I]),
    "qt_bn_finalize": (I, [P, I, I, LL, P, P, P, P, P, F, F, P, P, P, P, P]),
    "qt_bn_eval_affine": (I, [P, P, P, P, F, I, P, P, P]),
    "qt_bn_eval_affine_batched": (I, [P, I, F, P]),
    "qt_bn_act": (I, [I, P, P, P, P, P, P, I, P, LL, I, P]),
    "qt_bn_act_mask": (I, [I, P, P, P, P, P, P, I, P, P, LL, I, P]),
    "qt_bn_bwd_partial_rows": (I, [LL, I]),
    "qt_bn_bwd_reduce": (I, [I, P, P, P, P, P, P, LL, I, P]),
    "qt_bn_bwd_finalize": (I, [P, I, I, LL, P, P, P, P, I, P, P]),
    "qt_bn_bwd_apply": (I, [I, P, P, P, P, P, P, P, P, LL, I, P]),
    "qt_stem_pool": (I, [I, P, P, P, P, P, P, I, P]),
    "qt_stem_conv_pool": (I, [I, P, P, I, P, P, P, I, P]),
    "qt_stem_conv_pool_nchw": (I, [I, P, P, I, P, P, P, I, P]),
    "qt_stem_pool_bwd": (I, [I, P, P, P, P, P, P, I, P]),
    "qt_stem_bn_bwd_rows": (I, [I]),
    "qt_stem_bn_bwd_reduce": (I, [I, P, P, P, P, P, P, P, P, I, P]),
    "qt_stem_bn_bwd_sums_rows": (I, [I]),
    "qt_stem_bn_bwd_sums": (I, [I, P, P, P, P, P, P, P, I, P]),
    "qt_stem_bn_bwd_apply": (I, [I, P, P, P, P, P, P, P, P, P, I, P]),
    "qt_stem_bn_bwd_wgrad_workspace_bytes": (SZ, [I]),
    "qt_stem_bn_bwd_wgrad_ws": (I, [I, P, P, P, P, P, P, P, P, P, P, P, SZ, I, P]),
    "qt_stem_dgrad": (I, [I, P, P, P, I, P]),
    "qt_avgpool": (I, [I, P, P, I, I, I, I, I, P]),
    "qt_avgpool_bwd": (I, [I, P, P, P, I, I, I, I, I, P]),
    "qt_quad_pool": (I, [I, P, P, I, I, I, P]),
    "qt_quad_pool_bwd": (I, [I, P, P, P, I, I, I, P]),
    "qt_region_avgpool": (I, [I, P, P, I, I, I, I, I, I, I, P]),
    "qt_region_avgpool_bwd": (I, [I, P, I, P, P, I, I, I, I, I, I, P]),
    "qt_attention_gate": (I, [I, P, P, P, P, P, P, P, P, I, I, I, P]),
    "qt_attention_gate_bwd": (I, [I, P, P, P, P, P, P, P, P, P, I, I, I, P]),
    "qt_relu_mask_cols": (I, [I, P, P, P, LL, I, I, I, F, P]),
    "qt_lstm_forward": (I, [P, P, P, P, P, P, P, I, I, I, P]),
    "qt_lstm_backward": (I, [P, P, P, P, P, P, I, I, I, P]),
    "qt_transpose_f32": (I, [P, P, I, I, P]),
    "qt_scale_by_nonzero": (I, [P, P, LL, F, P]),
    "qt_cast_f32": (I, [I, P, P, LL, P]),
    "qt_lstm_stream_workspace_bytes": (SZ, [I, I, I, I]),
    "qt_lstm_stream_forward": (I, [P, P, P, P, P, P, P, P, P, P, SZ, LL, I, I, I, I, P]),
    "qt_lstm_stream_stage": (I, [P, P, P, I, I, I, I, P]),
    "qt_dropout": (I, [I, P, LL, I, I, ULL, F, P]),
    "qt_relu_mask_scale": (I, [I, P, P, LL, F, P]),
    "qt_col_sum": (I, [I, P, LL, I, I, P, I, P]),
    "qt_col_sum_workspace_bytes": (SZ, [LL, I]),
    "qt_col_sum_ws": (I, [I, P, LL, I, I, P, I, P, SZ, P]),
    "qt_linear_workspace_bytes": (SZ, [I, I, I]),
    "qt_linear_bf16": (I, [P, P, P, I, P, I, I, I, P, SZ, P]),
    "qt_gemm_small": (I, [P, P, P, P, P, P]),
    "qt_pack_clip27": (I, [I, P, P, I, I, I, I, P]),
    "qt_pack_conv3d_block": (I, [I, P, P, P, I, I, I, I, I, P, P, P]),
    "qt_unpack_conv3d_wgrad": (I, [P, P, I, I, I, I, I, P]),
    "qt_bn_stats_rows": (I, [LL, I]),
    "qt_bn_stats": (I, [I, P, LL, I, P, P]),
    "qt_pool3d_max": (I, [I, P, P, P, I, I, I, I, I, I, P]),
    "qt_pool3d_max_bwd": (I, [I, P, P, P, I, I, I, I, I, I, P]),
    "qt_pool3d_bn_relu_max": (I, [I, P, P, P, P, P, P, I, I, I, I, I, I, I, P]),
    "qt_set_pool3d_apply_light_min": (None, [LL]),
    "qt_pool3d_bn_bwd_apply": (I, [I, P, P, P, P, P, P, P, P, I, I, I, I, I, I, I, I, P]),
    "qt_conv3d_first_stats_rows": (I, [I, I, I, I]),
    "qt_conv3d_c32_stats_rows": (I, [I, I, I, I]),
    "qt_conv3d_c32_fwd": (I, [I, P, I, P, P, P, P, I, P, I, I, I, I, P]),
    "qt_conv3d_c32_dgrad_scratch_bytes": (SZ, [I, I, I, I]),
    "qt_conv3d_c32_dgrad": (I, [I, P, P, P, I, P, SZ, I, I, I, I, P]),
    "qt_conv3d_c32_wgrad_workspace_bytes": (SZ, [I, I, I, I]),
    "qt_conv3d_c32_wgrad": (I, [I, P, I, P, P, P, SZ, I, I, I, I, P]),
    "qt_conv3d_first_fwd_pool": (I, [I, P, P, P, I, P, P, I, I, I, I, P]),
    "qt_conv3d_first_wgrad_workspace_bytes": (SZ, [I, I, I, I]),
    "qt_conv3d_first_wgrad": (I, [I, P, P, P, P, SZ, I, I, I, I, P]),
    "qt_conv3d_first_wgrad_fused": (I, [I, P, P, P, P, I, P, P, P, P, P, P, P, SZ, I, I, I, I, P]),
    "qt_conv3d_first_fwd": (I, [I, P, P, P, P, P, I, P, I, I, I, I, P]),
    "qt_conv3d_first_dgrad": (I, [I, P, P, P, I, I, I, I, P]),
    "qt_avgpool_tb": (I, [I, P, P, I, I, I, I, I, I, P]),
    "qt_avgpool_tb_bwd": (I, [I, P, P, I, I, I, I, I, I, P]),
    "qt_plan_create": (I, [P, P]),
    "qt_plan_destroy": (None, [P]),
    "qt_plan_num_tensors": (I, [P]),
    "qt_plan_tensor_name": (S, [P, I]),
    "qt_plan_tensor_kind": (I, [P, I]),
    "qt_plan_tensor_shape": (I, [P, I, P]),
    "qt_plan_workspace_bytes": (SZ, [P]),
    "qt_plan_find_buffer": (I, [P, S, P]),
    "qt_plan_num_regions": (I, [P]),
    "qt_plan_region": (I, [P, I, P, P, P]),
    "qt_set_plan_guard_gap": (I, [SZ]),
    "qt_plan_profile_begin": (I, [P]),
    "qt_plan_profile_end": (I, [P, P, P, P]),
    "qt_plan_profile_bytes": (I, [P, P]),
    "qt_plan_side_fence": (I, [P, P]),
    "qt_plan_init_workspace": (I, [P, P, P]),
    "qt_plan_pack_weights": (I, [P, P, P, I, P]),
    "qt_plan_adam_step": (I, [P, P, P, P, P, P, P, I, P]),
    "qt_plan_adam_step_overlapped": (I, [P, P, P, P, P, P, P, I, P, P]),
    "qt_plan_adam_step_clipped": (I, [P, P, P, P, P, P, P, I, F, P, I, P, SZ, P, P]),
    "qt_plan_forward": (I, [P, P, P, P, P, P, I, I, ULL, P]),
    "qt_plan_features": (I, [P, P, P, P, P, I, P]),
    "qt_plan_stream_workspace_bytes": (SZ, [P, I, I, I]),
    "qt_plan_stream_forward": (I, [P, P, P, P, P, P, P, P, P, SZ, LL, I, I, I, P]),
    "qt_plan_backward": (I, [P, P, P, P, P, P, I, P]),
    "qt_plan_backward_dx": (I, [P, P, P, P, P, P, I, P, P]),
}


def bind(handle, signatures=None):
    """Type every entry point of `handle` (a ctypes.CDLL of the library) from the table; idempotent; returns the handle.
    A table name the library does not export is a stale build: QtError naming the symbol."""
    if signatures is None:
        if getattr(handle, "_qt_abi_bound", False):
            return handle
        signatures = SIGNATURES
    for name, (restype, argtypes) in signatures.items():
        try:
            fn = getattr(handle, name)
        except AttributeError:
            raise QtError(f"{name} is declared in include/qtcnn.h but missing from {handle._name}: the build is "
                          "stale, rebuild the library (__graft_entry__.build())") from None
        fn.restype, fn.argtypes = restype, argtypes
    if signatures is SIGNATURES:
        handle._qt_abi_bound = True
    return handle
