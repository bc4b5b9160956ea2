"""ctypes binding of libdsrl_hip.so (include/dsrl_hip.h).

The library is the product's only arithmetic path: if it cannot be loaded, or a call returns an error code,
a RuntimeError is raised - there is no CPU or stock-PyTorch fallback behind these wrappers.
"""
import ctypes as C
import os

import torch  # noqa: F401  (imported first so the HIP runtime the allocator uses is the one the library binds to)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libdsrl_hip.so')

fp = C.c_void_p          # device pointers travel as integers
i32 = C.c_int
i64 = C.c_int64
u64 = C.c_uint64
u32 = C.c_uint32
f32 = C.c_float
sz = C.c_size_t
stream_t = C.c_void_p

_conv_shape = [i32] * 10                      # N,H,W,C,K,R,S,stride,pad,dil


class WgradProblem(C.Structure):              # include/dsrl_hip.h: dsrl_wgrad_problem
    _fields_ = [('x', C.c_void_p), ('dy', C.c_void_p), ('dw', C.c_void_p)] + [(n, C.c_int32) for n in
                ('ldx', 'lddy', 'N', 'H', 'W', 'C', 'K', 'R', 'S', 'stride', 'pad', 'dil')] + [('x_amax', C.c_void_p), ('dy_amax', C.c_void_p)]


PROTOTYPES = {
    'dsrl_version': (i32, []),
    'dsrl_last_error': (C.c_char_p, []),
    'dsrl_device_check': (i32, [C.POINTER(i32)]),
    'dsrl_conv2d_fwd_workspace_bytes': (sz, _conv_shape),
    'dsrl_conv2d_fwd': (i32, [fp, i32, fp, fp, fp, i32] + _conv_shape + [fp, sz, stream_t]),
    'dsrl_conv2d_fwd_stats_parts': (i32, _conv_shape),
    'dsrl_conv2d_fwd_stats': (i32, [fp, i32, fp, fp, fp, i32] + _conv_shape + [fp, sz, fp, i32, stream_t]),
    'dsrl_conv2d_dgrad_workspace_bytes': (sz, _conv_shape),
    'dsrl_conv2d_transposed_filter_floats': (sz, [i32] * 4),
    'dsrl_conv2d_transpose_filter': (i32, [fp, fp, i32, i32, i32, i32, stream_t]),
    'dsrl_conv2d_transpose_filters_batched': (i32, [fp, i32, i64, stream_t]),
    'dsrl_conv2d_filters_amax_segment_floats': (i32, []),
    'dsrl_conv2d_filters_amax_batched': (i32, [fp, i64, stream_t]),
    'dsrl_conv2d_dgrad': (i32, [fp, i32, fp, fp, fp, i32] + _conv_shape + [fp, sz, stream_t]),
    'dsrl_conv2d_dgrad_stats_parts': (i32, _conv_shape),
    'dsrl_conv2d_dgrad_bnstats': (i32, [fp, i32, fp, fp, fp, i32] + _conv_shape + [fp, sz, fp, i32, fp, i32, fp, fp, i32, fp, i32, i32, stream_t]),
    'dsrl_conv2d_row_epilogue_supported': (i32, [i32] * 10 + [sz] + [i32] * 4),
    'dsrl_conv2d_dgrad_accumulate': (i32, [fp, i32, fp, fp, fp, i32] + _conv_shape + [fp, sz, stream_t]),
    'dsrl_conv2d_wgrad_workspace_bytes': (sz, _conv_shape),
    'dsrl_conv2d_wgrad': (i32, [fp, i32, fp, i32, fp] + _conv_shape + [fp, sz, stream_t]),
    'dsrl_conv2d_wgrad_group_table_bytes': (sz, [i32]),
    'dsrl_conv2d_wgrad_group_workspace_bytes': (sz, [fp, i32]),
    'dsrl_conv2d_wgrad_group_plan': (i32, [fp, i32, fp, sz, fp, fp, sz]),
    'dsrl_conv2d_wgrad_group_launch': (i32, [fp, fp, stream_t]),
    'dsrl_amax': (i32, [fp, i32, i64, i32, fp, stream_t]),
    'dsrl_conv2d_fwd_amax': (i32, [fp, i32, fp, fp, fp, fp, fp, fp, i32] + _conv_shape + [fp, sz, fp, i32, stream_t]),
    'dsrl_conv2d_dgrad_amax': (i32, [fp, i32, fp, fp, fp, fp, fp, fp, i32] + _conv_shape + [fp, sz, fp, i32, fp, i32, fp, fp, i32, fp, i32, i32, stream_t]),
    'dsrl_conv2d_split_filters_batched': (i32, [fp, i32, i64, stream_t]),
    'dsrl_planes_lo_offset': (sz, [i64]),
    'dsrl_planes_bytes': (sz, [i64, i32]),
    'dsrl_split_planes': (i32, [fp, i32, i64, i32, fp, fp, i32, stream_t]),
    'dsrl_conv2d_filter_planes_batched': (i32, [fp, i32, i64, stream_t]),
    'dsrl_conv2d_fwd_planes': (i32, [fp, i32, fp, fp, fp, fp, fp, fp, fp, fp, i32] + _conv_shape + [fp, sz, fp, i32, stream_t]),
    'dsrl_conv2d_dgrad_planes': (i32, [fp, i32, fp, fp, fp, fp, fp, fp, fp, fp, i32] + _conv_shape + [fp, sz, fp, i32, fp, i32, fp, fp, i32, fp, i32, i32, stream_t]),
    'dsrl_conv2d_dgrad_planes_drop': (i32, [fp, i32, fp, fp, fp, fp, fp, fp, fp, fp, i32] + _conv_shape + [fp, sz, fp, i32, fp, i32, fp, fp, i32, f32, fp, i32, i32, stream_t]),
    'dsrl_conv2d_wgrad_amax': (i32, [fp, i32, fp, fp, i32, fp, fp] + _conv_shape + [fp, sz, stream_t]),
    'dsrl_conv_precision': (i32, [i32]),
    'dsrl_conv2d_inbounds_macs': (i64, _conv_shape),
    'dsrl_conv2d_rowfold_fwd_workspace_bytes': (sz, [i32] * 9),
    'dsrl_conv2d_rowfold_fwd': (i32, [fp, i32, fp, fp, fp, i32] + [i32] * 9 + [i64, fp, sz, stream_t]),
    'dsrl_conv2d_rowfold_wgrad_workspace_bytes': (sz, [i32] * 9),
    'dsrl_conv2d_rowfold_wgrad': (i32, [fp, i32, fp, i32, fp] + [i32] * 9 + [i64, fp, sz, stream_t]),
    'dsrl_pad_image_nhwc': (i32, [fp, i64, i64, i64, i64, fp] + [i32] * 9 + [stream_t]),
    'dsrl_colsum_workspace_bytes': (sz, [i64, i32]),
    'dsrl_colsum': (i32, [fp, i32, i64, i32, fp, fp, sz, stream_t]),
    'dsrl_bn_workspace_bytes': (sz, [i64, i32]),
    'dsrl_bn_stats_floats': (sz, [i32, i32, i32]),
    'dsrl_bn_stats': (i32, [fp, i32, i64, i32, f32, f32, fp, fp, fp, fp, fp, sz, stream_t]),
    'dsrl_bn_invstd_from_var': (i32, [fp, i32, f32, fp, stream_t]),
    'dsrl_bn_apply': (i32, [fp, i32, fp, i32, i64, i32, fp, fp, fp, fp, fp, i32, i32, f32, u64, u32, fp, stream_t]),
    'dsrl_bn_fused_max_blocks': (i32, [i32]),
    'dsrl_bn_fused_barrier_timeouts': (i32, [C.POINTER(i64)]),
    'dsrl_bn_train_fwd_from_stats': (i32, [fp, i32, fp, i32, i64, i32, f32, f32, fp, fp, fp, fp, fp, fp, fp, i32, i32, f32, u64, u32, fp, i32, fp, stream_t]),
    'dsrl_bn_mask_words': (sz, [i64, i32]),
    'dsrl_bn_train_fwd_from_stats_mask': (i32, [fp, i32, fp, i32, i64, i32, f32, f32, fp, fp, fp, fp, fp, fp, fp, i32, i32, f32, u64, u32, fp, i32, fp, fp, stream_t]),
    'dsrl_bn_train_fwd': (i32, [fp, i32, fp, i32, i64, i32, f32, f32, fp, fp, fp, fp, fp, fp, fp, i32, i32, f32, u64, u32, fp, sz, fp, stream_t]),
    'dsrl_bn_bwd': (i32, [fp, i32, fp, i32, fp, i32, fp, i32, fp, i32, i64, i32, fp, fp, fp, fp, fp, i32, f32, i32, fp, sz, fp, stream_t]),
    'dsrl_bn_bwd_from_stats': (i32, [fp, i32, fp, i32, fp, i32, fp, i32, fp, i32, i64, i32, fp, fp, fp, fp, fp, i32, i32, fp, i32, fp, stream_t]),
    'dsrl_bn_bwd_from_stats_drop': (i32, [fp, i32, fp, i32, fp, i32, fp, i32, fp, i32, i64, i32, fp, fp, fp, fp, fp, i32, f32, i32, fp, i32, fp, stream_t]),
    'dsrl_bn_bwd_from_stats_res_parts': (i32, [i64, i32, i32]),
    'dsrl_bn_bwd_from_stats_res': (i32, [fp, i32, fp, i32, fp, i32, fp, i32, fp, i32, i64, i32, fp, fp, fp, fp, fp, i32, f32, i32, fp, i32, fp, fp, i32, fp, fp, fp, i32, stream_t]),
    'dsrl_dropout_fwd': (i32, [fp, i32, fp, i32, i64, i32, f32, u64, u32, stream_t]),
    'dsrl_dropout_bwd': (i32, [fp, i32, fp, i32, i64, i32, f32, u64, u32, stream_t]),
    'dsrl_bilinear_ac_fwd': (i32, [fp, i32, fp, i32, i32, i32, i32, i32, i32, i32, stream_t]),
    'dsrl_bilinear_ac_bwd_workspace_bytes': (sz, [i32] * 6),
    'dsrl_bilinear_ac_bwd': (i32, [fp, i32, fp, i32, i32, i32, i32, i32, i32, i32, fp, sz, stream_t]),
    'dsrl_global_avgpool_fwd': (i32, [fp, i32, fp, i32, i32, i32, stream_t]),
    'dsrl_global_avgpool_bwd': (i32, [fp, fp, i32, i32, i32, i32, stream_t]),
    'dsrl_maxpool3x3s2_fwd': (i32, [fp, fp, fp, i32, i32, i32, i32, stream_t]),
    'dsrl_maxpool3x3s2_bwd': (i32, [fp, fp, fp, i32, i32, i32, i32, stream_t]),
    'dsrl_convt2x2_fwd': (i32, [fp, fp, fp, fp, i32, i32, i32, i32, i32, stream_t]),
    'dsrl_convt2x2_bwd_workspace_bytes': (sz, [i32] * 5),
    'dsrl_convt2x2_bwd': (i32, [fp, fp, fp, fp, fp, fp, i32, i32, i32, i32, i32, fp, sz, stream_t]),
    'dsrl_convt2x2_fwd_ce_supported': (i32, [fp, fp, i32, i32, i32, i32, i32]),
    'dsrl_convt2x2_fwd_ce_workspace_bytes': (sz, [i32, i32, i32]),
    'dsrl_convt2x2_fwd_ce': (i32, [fp, fp, fp, fp, i32, i32, i32, i32, i32, fp, i32, fp, fp, fp, sz, stream_t]),
    'dsrl_convt2x2_bwd_ce_supported': (i32, [fp, fp, fp, i32, i32, i32, i32, i32]),
    'dsrl_convt2x2_bwd_ce': (i32, [fp, fp, fp, fp, i32, fp, fp, fp, i32, fp, fp, fp, i32, i32, i32, i32, i32, fp, sz, stream_t]),
    'dsrl_pixel_shuffle_fwd': (i32, [fp, fp, i32, i32, i32, i32, i32, stream_t]),
    'dsrl_pixel_shuffle_bwd': (i32, [fp, fp, i32, i32, i32, i32, i32, stream_t]),
    'dsrl_pointwise_strided_fwd': (i32, [fp, fp, fp, i32, i32, i32, i32, i32, stream_t]),
    'dsrl_pointwise_strided_bwd_workspace_bytes': (sz, [i32] * 5),
    'dsrl_pointwise_strided_bwd': (i32, [fp, fp, fp, fp, fp, i32, i32, i32, i32, i32, i32, fp, sz, stream_t]),
    'dsrl_copy2d': (i32, [fp, i32, fp, i32, i64, i32, stream_t]),
    'dsrl_cat_channels_supported': (i32, [fp, fp, fp, i32, fp, i32, i64]),          # srcs / lds / cs: host arrays (ctypes)
    'dsrl_cat_channels': (i32, [fp, fp, fp, i32, fp, i32, i64, fp, stream_t]),
    'dsrl_nchw_to_nhwc': (i32, [fp, fp, i32, i32, i32, i32, i32, stream_t]),
    'dsrl_ce_workspace_bytes': (sz, [i64]),
    'dsrl_ce_fwd': (i32, [fp, i32, fp, i64, i32, i32, fp, fp, sz, stream_t]),
    'dsrl_ce_bwd': (i32, [fp, i32, fp, i64, i32, i32, fp, fp, fp, i32, stream_t]),
    'dsrl_mse_workspace_bytes': (sz, [i64]),
    'dsrl_mse_fwd': (i32, [fp, fp, i64, fp, fp, sz, stream_t]),
    'dsrl_mse_bwd': (i32, [fp, fp, i64, fp, fp, stream_t]),
    'dsrl_ce_fused_workspace_bytes': (sz, [i64]),
    'dsrl_ce_fused': (i32, [fp, i32, fp, i64, i32, i32, fp, i32, fp, fp, fp, sz, stream_t]),
    'dsrl_mse_fused': (i32, [fp, fp, i64, f32, fp, fp, fp, fp, sz, stream_t]),
    'dsrl_ce_weight_sum_workspace_bytes': (sz, []),
    'dsrl_ce_weight_sum': (i32, [fp, i64, i32, i32, fp, fp, fp, sz, stream_t]),
    'dsrl_ce_w_workspace_bytes': (sz, [i64]),
    'dsrl_ce_fwd_w': (i32, [fp, i32, fp, i64, i32, i32, fp, fp, fp, sz, stream_t]),
    'dsrl_ce_bwd_w': (i32, [fp, i32, fp, i64, i32, i32, fp, fp, fp, fp, i32, stream_t]),
    'dsrl_ce_fused_w_workspace_bytes': (sz, [i64]),
    'dsrl_ce_fused_w': (i32, [fp, i32, fp, i64, i32, i32, fp, fp, i32, fp, fp, fp, sz, stream_t]),
    'dsrl_convt2x2_fwd_ce_w_workspace_bytes': (sz, [i32, i32, i32]),
    'dsrl_convt2x2_fwd_ce_w': (i32, [fp, fp, fp, fp, i32, i32, i32, i32, i32, fp, i32, fp, fp, fp, fp, sz, stream_t]),
    'dsrl_convt2x2_bwd_ce_w': (i32, [fp, fp, fp, fp, i32, fp, fp, fp, fp, i32, fp, fp, fp, i32, i32, i32, i32, i32, fp, sz, stream_t]),
    'dsrl_class_histogram': (i32, [fp, i64, fp, fp, stream_t]),
    'dsrl_ce_f_workspace_bytes': (sz, [i64]),
    'dsrl_ce_fwd_f': (i32, [fp, i32, fp, i64, i32, i32, fp, f32, fp, fp, sz, stream_t]),
    'dsrl_ce_bwd_f': (i32, [fp, i32, fp, i64, i32, i32, fp, f32, fp, fp, fp, i32, stream_t]),
    'dsrl_ce_fused_f_workspace_bytes': (sz, [i64]),
    'dsrl_ce_fused_f': (i32, [fp, i32, fp, i64, i32, i32, fp, f32, fp, i32, fp, fp, fp, sz, stream_t]),
    'dsrl_convt2x2_fwd_ce_f_workspace_bytes': (sz, [i32, i32, i32]),
    'dsrl_convt2x2_fwd_ce_f': (i32, [fp, fp, fp, fp, i32, i32, i32, i32, i32, fp, i32, fp, f32, fp, fp, fp, sz, stream_t]),
    'dsrl_convt2x2_bwd_ce_f': (i32, [fp, fp, fp, fp, i32, fp, f32, fp, fp, fp, i32, fp, fp, fp, i32, i32, i32, i32, i32, fp, sz, stream_t]),
    'dsrl_ce_s_workspace_bytes': (sz, [i64]),
    'dsrl_ce_fwd_s': (i32, [fp, i32, fp, i64, i32, i32, fp, f32, fp, fp, sz, stream_t]),
    'dsrl_ce_bwd_s': (i32, [fp, i32, fp, i64, i32, i32, fp, f32, fp, fp, fp, i32, stream_t]),
    'dsrl_ce_fused_s_workspace_bytes': (sz, [i64]),
    'dsrl_ce_fused_s': (i32, [fp, i32, fp, i64, i32, i32, fp, f32, fp, i32, fp, fp, fp, sz, stream_t]),
    'dsrl_convt2x2_fwd_ce_s_workspace_bytes': (sz, [i32, i32, i32]),
    'dsrl_convt2x2_fwd_ce_s': (i32, [fp, fp, fp, fp, i32, i32, i32, i32, i32, fp, i32, fp, f32, fp, fp, fp, sz, stream_t]),
    'dsrl_convt2x2_bwd_ce_s': (i32, [fp, fp, fp, fp, i32, fp, f32, fp, fp, fp, i32, fp, fp, fp, i32, i32, i32, i32, i32, fp, sz, stream_t]),
    'dsrl_ohem_workspace_bytes': (sz, [i64]),
    'dsrl_ohem_prob': (i32, [fp, i32, fp, i64, i32, i32, fp, fp, stream_t]),
    'dsrl_ohem_select': (i32, [fp, i64, f32, i64, fp, fp, sz, stream_t]),
    'dsrl_ohem_apply': (i32, [fp, fp, i64, i32, fp, fp, stream_t]),
    'dsrl_ohem_target': (i32, [fp, i32, fp, i64, i32, i32, f32, i64, fp, fp, fp, fp, sz, stream_t]),
    'dsrl_dice_workspace_bytes': (sz, [i64]),
    'dsrl_dice_fwd': (i32, [fp, i32, fp, i64, i32, i32, f32, f32, fp, fp, fp, sz, stream_t]),
    'dsrl_dice_bwd': (i32, [fp, i32, fp, i64, i32, i32, fp, i32, fp, i32, stream_t]),
    'dsrl_convt2x2_bwd_ce_d': (i32, [fp, fp, fp, fp, i32, fp, fp, fp, fp, fp, i32, fp, fp, fp, i32, i32, i32, i32, i32, fp, sz, stream_t]),
    'dsrl_lovasz_workspace_bytes': (sz, [i64, i32, i32]),
    'dsrl_lovasz_record_floats': (sz, [i32, i32]),
    'dsrl_lovasz_fwd': (i32, [fp, i32, fp, i64, i32, i32, f32, i32, fp, fp, fp, sz, stream_t]),
    'dsrl_lovasz_bwd': (i32, [fp, i32, fp, i64, i32, i32, fp, i32, i32, fp, i32, stream_t]),
    'dsrl_convt2x2_bwd_ce_l': (i32, [fp, fp, fp, fp, i32, fp, fp, i32, fp, fp, fp, i32, fp, fp, fp, i32, i32, i32, i32, i32, fp, sz, stream_t]),
    'dsrl_relax_mask': (i32, [fp, i32, i32, i32, i32, i32, i32, fp, fp, stream_t]),
    'dsrl_ce_r_workspace_bytes': (sz, [i64]),
    'dsrl_ce_fwd_r': (i32, [fp, i32, fp, i64, i32, i32, fp, fp, fp, fp, sz, stream_t]),
    'dsrl_ce_bwd_r': (i32, [fp, i32, fp, i64, i32, i32, fp, fp, fp, fp, fp, i32, stream_t]),
    'dsrl_ce_fused_r_workspace_bytes': (sz, [i64]),
    'dsrl_ce_fused_r': (i32, [fp, i32, fp, i64, i32, i32, fp, fp, fp, i32, fp, fp, fp, sz, stream_t]),
    'dsrl_convt2x2_fwd_ce_r_workspace_bytes': (sz, [i32, i32, i32]),
    'dsrl_convt2x2_fwd_ce_r': (i32, [fp, fp, fp, fp, i32, i32, i32, i32, i32, fp, i32, fp, fp, fp, fp, fp, sz, stream_t]),
    'dsrl_convt2x2_bwd_ce_r': (i32, [fp, fp, fp, fp, i32, fp, fp, fp, fp, fp, i32, fp, fp, fp, i32, i32, i32, i32, i32, fp, sz, stream_t]),
    'dsrl_loss_mix': (i32, [fp, fp, fp, f32, f32, fp, fp, stream_t]),
    'dsrl_fa_saved_floats': (sz, [i32] * 5),
    'dsrl_fa_workspace_bytes': (sz, [i32] * 5),
    'dsrl_fa_fwd': (i32, [fp, fp, i32, i32, i32, i32, i64, i64, i64, i64, i32, i32, fp, fp, fp, sz, stream_t]),
    'dsrl_fa_bwd': (i32, [fp, fp, i32, i32, i32, i32, i64, i64, i64, i64, i32, i32, fp, fp, fp, fp, fp, sz, stream_t]),
    'dsrl_seg_metrics': (i32, [fp, i32, fp, i64, i32, i32, fp, stream_t]),
    'dsrl_seg_metrics_cm_max_classes': (i32, []),
    'dsrl_seg_metrics_cm': (i32, [fp, i32, fp, i64, i32, i32, fp, fp, stream_t]),
    'dsrl_confusion_matrix_max_classes': (i32, []),
    'dsrl_confusion_matrix': (i32, [fp, fp, i64, i32, i32, fp, fp, stream_t]),
    'dsrl_sssr_tail_predict_supported': (i32, [i32] * 6),
    'dsrl_sssr_tail_predict_workspace_bytes': (sz, [i32] * 3),
    'dsrl_sssr_tail_predict': (i32, [fp, i32] + [i32] * 6 + [fp] * 9 + [i32, fp, fp, fp, fp, sz, stream_t]),
    'dsrl_sssr_tail_predict_flip': (i32, [fp, i32] + [i32] * 6 + [fp] * 9 + [i32, fp, fp, fp, fp, sz, stream_t]),
    'dsrl_sssr_tail_predict_cm': (i32, [fp, i32] + [i32] * 6 + [fp] * 9 + [i32, fp, fp, fp, fp, sz, fp, stream_t]),
    'dsrl_sssr_tail_predict_flip_cm': (i32, [fp, i32] + [i32] * 6 + [fp] * 9 + [i32, fp, fp, fp, fp, sz, fp, stream_t]),
    'dsrl_prob_merge_supported': (i32, [i32] * 6),
    'dsrl_prob_merge_acc_bytes': (sz, [i32] * 4),
    'dsrl_prob_merge_workspace_bytes': (sz, [i32] * 3),
    'dsrl_prob_merge': (i32, [fp, i32] + [i32] * 5 + [fp, i32, i32, i32, stream_t]),
    'dsrl_prob_merge_finish': (i32, [fp, i32] + [i32] * 5 + [fp, i32, i32, i32, fp, fp, i32, fp, fp, fp, fp, sz, fp, stream_t]),
    'dsrl_window_merge_supported': (i32, [i32] * 6),
    'dsrl_window_merge_workspace_bytes': (sz, [i32] * 3),
    'dsrl_window_merge': (i32, [fp, i32] + [i32] * 5 + [fp] + [i32] * 6 + [stream_t]),
    'dsrl_window_merge_finish': (i32, [fp] + [i32] * 4 + [C.POINTER(i32), i32, C.POINTER(i32), i32, i32, i32, i32, fp, fp, i32, fp, fp, fp, fp, sz, fp,
                                       stream_t]),          # ys / xs: host arrays (ctypes)
    'dsrl_window_merge_finish_ex': (i32, [fp] + [i32] * 4 + [C.POINTER(i32), i32, C.POINTER(i32), i32, i32, i32, i32, fp, fp, i32, fp, fp, fp, fp, sz, fp,
                                          fp, i32, fp, stream_t]),
    'dsrl_fingerprint_segment_words': (i32, []),
    'dsrl_fingerprint_segments': (i32, [fp, i64, fp, fp, fp, i32, stream_t]),
    'dsrl_class_map_visualize': (i32, [fp, fp, fp, fp, fp, i32, i32, i32, i32, C.c_double, stream_t]),
    'dsrl_prepare_batch': (i32, [fp, fp, fp, C.POINTER(f32), C.POINTER(f32), fp, fp, fp, i32, i32, i32, i32, i32, stream_t]),
    'dsrl_augment_geometry': (i32, [fp, fp, fp, fp, fp, fp, i32, i32, i32, stream_t]),
    'dsrl_prepare_batch_augmented': (i32, [fp, fp, fp, C.POINTER(f32), C.POINTER(f32), fp, fp, fp, i32, i32, i32, i32, i32, fp, stream_t]),
    'dsrl_colour_jitter_workspace_bytes': (sz, [i32, i32, i32]),
    'dsrl_colour_jitter_means': (i32, [fp, fp, fp, fp, sz, i32, i32, i32, stream_t]),
    'dsrl_prepare_batch_jittered': (i32, [fp, fp, fp, C.POINTER(f32), C.POINTER(f32), fp, fp, fp, i32, i32, i32, i32, i32, fp, fp, fp, stream_t]),
    'dsrl_sgd_step': (i32, [fp, fp, fp, i64, f32, f32, f32, f32, stream_t]),
    'dsrl_sgd_step_dev': (i32, [fp, fp, fp, i64, fp, stream_t]),
    'dsrl_sgd_step_dev_segments': (i32, [fp, fp, fp, fp, i64, fp, stream_t]),
    'dsrl_sgd_step_ema': (i32, [fp, fp, fp, i64, f32, f32, f32, f32, fp, fp, stream_t]),
    'dsrl_sgd_step_dev_ema': (i32, [fp, fp, fp, i64, fp, fp, fp, stream_t]),
    'dsrl_sgd_step_dev_segments_ema': (i32, [fp, fp, fp, fp, i64, fp, fp, fp, stream_t]),
    'dsrl_ema_update': (i32, [fp, fp, i64, fp, stream_t]),
    'dsrl_ema_advance': (i32, [fp, stream_t]),
    'dsrl_arena_swap': (i32, [fp, fp, i64, stream_t]),
    'dsrl_grad_sumsq': (i32, [fp, i64, i64, fp, stream_t]),
    'dsrl_grad_clip_workspace_bytes': (sz, [i64]),
    'dsrl_grad_clip_finish': (i32, [fp, i64, fp, f32, f32, f32, f32, fp, fp, stream_t]),
    'dsrl_adamw_step': (i32, [fp, fp, fp, fp, i64, f32, f32, f32, fp, stream_t]),
    'dsrl_adamw_step_dev': (i32, [fp, fp, fp, fp, i64, fp, fp, stream_t]),
    'dsrl_adamw_step_dev_segments': (i32, [fp, fp, fp, fp, fp, i64, fp, fp, stream_t]),
    'dsrl_adamw_step_ema': (i32, [fp, fp, fp, fp, i64, f32, f32, f32, fp, fp, fp, stream_t]),
    'dsrl_adamw_step_dev_ema': (i32, [fp, fp, fp, fp, i64, fp, fp, fp, fp, stream_t]),
    'dsrl_adamw_step_dev_segments_ema': (i32, [fp, fp, fp, fp, fp, i64, fp, fp, fp, fp, stream_t]),
    'dsrl_adamw_advance': (i32, [fp, stream_t]),
    'dsrl_adamw_set_step': (i32, [fp, i64, stream_t]),
    'dsrl_nan_check': (i32, [fp, i64, fp, stream_t]),
    'dsrl_sssr_tail_predict_ex': (i32, [fp, i32] + [i32] * 6 + [fp] * 9 + [i32, fp, fp, fp, fp, sz, fp, fp, i32, fp, stream_t]),
    'dsrl_sssr_tail_predict_flip_ex': (i32, [fp, i32] + [i32] * 6 + [fp] * 9 + [i32, fp, fp, fp, fp, sz, fp, fp, i32, fp, stream_t]),
    'dsrl_prob_merge_finish_ex': (i32, [fp, i32] + [i32] * 5 + [fp, i32, i32, i32, fp, fp, i32, fp, fp, fp, fp, sz, fp, fp, i32, fp, stream_t]),
    'dsrl_calibration_max_bins': (i32, []),
    'dsrl_calibration_from_logits': (i32, [fp, i32, fp, i64, i32, i32, i32, fp, fp, fp, stream_t]),
    'dsrl_temperature_max_points': (i32, []),
    'dsrl_temperature_workspace_bytes': (sz, [i64, i32]),
    'dsrl_temperature_stats': (i32, [fp, i32, fp, i64, i32, i32, fp, i32, fp, fp, fp, sz, stream_t]),
    'dsrl_sssr_tail_predict_t': (i32, [fp, i32] + [i32] * 6 + [fp] * 9 + [i32, fp, fp, fp, fp, sz, fp, fp, i32, fp, f32, stream_t]),
    'dsrl_sssr_tail_predict_flip_t': (i32, [fp, i32] + [i32] * 6 + [fp] * 9 + [i32, fp, fp, fp, fp, sz, fp, fp, i32, fp, f32, stream_t]),
    'dsrl_calibration_from_logits_t': (i32, [fp, i32, fp, i64, i32, i32, i32, fp, fp, fp, f32, stream_t]),
    'dsrl_sr_quality_workspace_bytes': (sz, [i32] * 4),
    'dsrl_sr_quality': (i32, [fp, i32, fp, i32, i32, i32, i32, i32, C.POINTER(f32), C.POINTER(f32), fp, fp, fp, sz, stream_t]),
    'dsrl_boundary_counts_max_classes': (i32, []),
    'dsrl_boundary_counts_max_distance': (i32, []),
    'dsrl_boundary_counts_workspace_bytes': (sz, [i32] * 4),
    'dsrl_boundary_counts': (i32, [fp, fp, i32, i32, i32, i32, i32, i32, fp, fp, fp, fp, sz, stream_t]),
    'dsrl_rng_bind_device_key': (i32, [fp]),
    'dsrl_rng_advance_key': (i32, [fp, stream_t]),
    'dsrl_prof_enable': (i32, [i32]),
    'dsrl_prof_read': (i32, [i32, C.POINTER(i64), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    'dsrl_prof_read_bytes': (i32, [i32, C.POINTER(C.c_double)]),
    'dsrl_prof_kernel_name': (C.c_char_p, [i32]),
}

_lib = None


class DsrlHipError(RuntimeError):
    pass


def load():
    """Loads libdsrl_hip.so (once). Raises DsrlHipError with the build hint when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise DsrlHipError(f'{LIB_PATH} not found: build it with `python -c "import __graft_entry__ as g; g.build()"` '
                           f'or `make -C {os.path.join(_HERE, "csrc")}` - there is no fallback path')
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)          # AttributeError here means header and library disagree
        fn.restype = res
        fn.argtypes = args
    if lib.dsrl_version() != 1:
        raise DsrlHipError(f'libdsrl_hip.so ABI version {lib.dsrl_version()} != 1')
    _lib = lib
    return lib


def knob(name, default):
    """The one way the package reads a DSRL_* environment switch (table: DESIGN.md, "Environment switches"); the library's twin is knob() in
    csrc/common.h.  The value comes back in the type of `default`: bool ('0' = off, anything else on), int, or the string itself (default a
    string or None)."""
    v = os.environ.get(name)
    if v is None:
        return default
    if isinstance(default, bool):
        return v != '0'
    if isinstance(default, int):
        return int(v)
    return v


def check(code, what):
    if code != 0:
        msg = _lib.dsrl_last_error().decode('utf-8', 'replace') if _lib is not None else ''
        raise DsrlHipError(f'{what} failed with code {code}: {msg}')


def call(name, *args):
    lib = load()
    check(getattr(lib, name)(*args), name)


def query(name, *args):
    return getattr(load(), name)(*args)
