"""The ctypes signature of every entry point of libstts2.so: name -> ([argument types], return type).

One entry per prototype of include/stts2.h and include/stts2_train.h, in the headers' own order, so the two can be
read side by side.  engine.lib() applies the whole table when it loads the library; tests/test_native_abi.py holds
it to the headers (names both ways, argument count, the class of every argument and of the return value).  A new
entry point gets its line here and nowhere else.

Every pointer is a c_void_p (engine.call passes a tensor there as its data_ptr()) except the host int / double arrays and out-pointers
that callers pass as ctypes arrays or byref(), and the two string returns.
"""
import ctypes

i, ll, ull, f, d, vp = (ctypes.c_int, ctypes.c_longlong, ctypes.c_ulonglong, ctypes.c_float, ctypes.c_double,
                        ctypes.c_void_p)
pi, pll, pd, pvp = ctypes.POINTER(i), ctypes.POINTER(ll), ctypes.POINTER(d), ctypes.POINTER(vp)
string = ctypes.c_char_p

SIGNATURES = {
    # ================================================================== include/stts2.h
    "stts_model_create": ([i, pi, i, pvp], i),
    "stts_model_destroy": ([vp], None),
    "stts_param_count": ([vp], i),
    "stts_param_name": ([vp, i], string),
    "stts_param_numel": ([vp, i], ll),
    "stts_set_param": ([vp, i, vp], i),
    "stts_packed_bytes": ([vp, i], ll),
    "stts_pack": ([vp, i, vp, ll, vp], i),
    "stts_workspace_bytes": ([vp, i, i, i], ll),
    "stts_decoder_fwd": ([vp, i, vp, vp, vp, vp, vp, ull, ll, i, i, vp, vp, ll, vp], i),
    "stts_f0n_fwd": ([vp, i, vp, vp, i, i, vp, vp, vp, ll, vp], i),
    "stts_style_fwd": ([vp, i, vp, i, i, vp, vp, ll, vp], i),
    "stts_pitch_fwd": ([vp, i, vp, i, i, vp, vp, vp, vp, ll, vp], i),
    "stts_pitch_error_offset": ([vp, i, i, i], ll),
    "stts_log_norm": ([vp, i, i, i, f, f, vp, vp], i),
    # text aligner, monotonic alignment search (the search's lengths are host arrays)
    "stts_aligner_fwd": ([vp, i, vp, vp, vp, vp, i, i, i, vp, vp, vp, vp, vp, ll, vp], i),
    "stts_aligner_workspace_bytes": ([vp, i, i, i, i], ll),
    "stts_maximum_path_workspace_bytes": ([i, i, i], ll),
    "stts_maximum_path": ([vp, pi, pi, i, i, i, vp, vp, ll, vp], i),
    # MultiPeriodDiscriminator
    "stts_mpd_out_elems": ([vp, i, i], ll),
    "stts_mpd_fwd": ([vp, i, vp, i, i, vp, ll, vp, ll, vp], i),
    "stts_mpd_losses": ([vp, i, i, vp, vp, ll, vp, vp], i),
    "stts_gan_losses_scratch_bytes": ([vp], ll),
    # multi-resolution mel loss
    "stts_mrstft_workspace_bytes": ([i, ll, pi, i, i], ll),
    "stts_mrstft_loss": ([vp, vp, i, ll, ll, pi, pi, pi, i, i, i, vp, vp, ll, vp], i),
    # conv1d forward / backward on caller frames
    "stts_conv1d_fwd_workspace_bytes": ([i] * 10, ll),
    "stts_conv1d_fwd": ([i, vp, vp, vp] + [i] * 9 + [vp, vp, ll, vp], i),
    "stts_conv1d_fwd_res": ([i, vp, vp, vp, vp, f] + [i] * 9 + [vp, vp, ll, vp], i),
    "stts_conv1d_fwd_act": ([i, vp, vp, vp] + [i] * 9 + [f, vp, vp, ll, vp], i),
    "stts_conv1d_fwd_tx_workspace_bytes": ([i] * 10, ll),
    "stts_conv1d_fwd_tx": ([i, vp, vp, vp] + [i] * 10 + [f, vp, vp, ll, vp], i),
    "stts_conv1d_bwd_tx_workspace_bytes": ([i] * 10, ll),
    "stts_conv1d_bwd_tx": ([i, vp, vp] + [i] * 9 + [vp, vp, ll, vp], i),
    "stts_conv1d_wgrad_tx": ([i, vp, vp] + [i] * 9 + [vp, vp, vp, ll, vp], i),
    "stts_conv1d_bwd_workspace_bytes": ([i] * 10, ll),
    "stts_conv1d_bwd": ([i, vp, vp, vp] + [i] * 9 + [vp, vp, vp, vp, ll, vp], i),
    # ConvTranspose1d
    "stts_conv_transpose1d_workspace_bytes": ([i] * 9, ll),
    "stts_conv_transpose1d_fwd": ([i, vp, vp, vp] + [i] * 8 + [vp, vp, ll, vp], i),
    "stts_conv_transpose1d_bwd": ([i, vp, vp, vp] + [i] * 8 + [vp, vp, vp, vp, ll, vp], i),
    # AdaIN1d + activation, Linear, pool / upsample, LeakyReLU, weight-norm backward
    "stts_adain_act_workspace_bytes": ([i, i, i], ll),
    "stts_adain_act_fwd": ([vp, vp, vp, i, i, i, i, vp, vp, vp, ll, vp], i),
    "stts_adain_act_bwd": ([vp, vp, vp, i, vp, vp, i, i, i, vp, vp, vp, vp, ll, vp], i),
    "stts_linear_fwd": ([vp, vp, vp, i, i, i, vp, vp], i),
    "stts_linear_bwd": ([vp, vp, vp, i, i, i, vp, vp, vp, vp], i),
    "stts_pool_workspace_bytes": ([i, i, i], ll),
    "stts_pool_fwd": ([vp, vp, vp, i, i, i, vp, vp], i),
    "stts_pool_bwd": ([vp, vp, vp, i, i, i, vp, vp, vp, vp, ll, vp], i),
    "stts_upsample2": ([vp, i, i, i, vp, vp], i),
    "stts_upsample2_bwd": ([vp, i, i, i, vp, vp], i),
    "stts_leaky_relu": ([vp, ll, f, vp, vp], i),
    "stts_leaky_relu_bwd": ([vp, vp, ll, f, vp, vp], i),
    "stts_weight_norm_bwd": ([vp, vp, vp, i, i, vp, vp, vp], i),
    # MultiResSpecDiscriminator
    "stts_msd_out_elems": ([vp, i, i], ll),
    "stts_msd_fwd": ([vp, i, vp, i, i, vp, ll, vp, ll, vp], i),
    "stts_msd_losses": ([vp, i, i, vp, vp, ll, vp, vp], i),
    # style front-end (log-mel)
    "stts_mel_frames": ([ll], ll),
    "stts_mel_workspace_bytes": ([], ll),
    "stts_wave_preprocess": ([vp, i, ll, ll, vp, vp, ll, vp], i),
    # duration / text path
    "stts_frames_gemm": ([vp, ll, ll, ll, i, i, i, vp, ll, ll, ll, ll, i, i, i, vp, vp, vp, ll, ll, ll, i, vp], i),
    "stts_frames_gemm_ws": ([vp, ll, ll, ll, i, i, i, vp, ll, ll, ll, ll, i, i, i, vp, vp, vp, ll, ll, ll, i, vp, ll,
                             vp], i),
    "stts_bilstm_workspace_bytes": ([i, i, i], ll),
    "stts_set_lstm_group": ([i], i),
    "stts_bilstm_fwd": ([vp, ll, ll, ll, i, i, i, vp, pvp, i, vp, vp, vp, vp, ll, vp], i),
    "stts_bilstm_error_offset": ([i, i, i], ll),
    "stts_set_bilstm_debug": ([i, i], i),
    "stts_row_norm": ([vp, ll, ll, ll, i, i, i, i, vp, vp, ll, f, i, f, vp, vp, i, vp, ll, ll, vp], i),
    "stts_embedding": ([vp, i, i, vp, i, i, vp, vp, vp, vp], i),
    "stts_durations": ([vp, ll, ll, i, i, i, vp, vp, f, f, f, vp, vp, vp, vp, vp], i),
    "stts_expand_frames": ([vp, ll, ll, ll, i, i, i, vp, i, vp, vp, vp], i),
    "stts_weight_norm": ([vp, vp, i, i, vp, vp], i),
    # errors, ABI revision, options, profiling
    "stts_error_string": ([i], string),
    "stts_abi_version": ([], i),
    "stts_set_option": ([i, i], i),
    "stts_get_option": ([i], i),
    "stts_set_debug_buffer": ([vp], i),
    "stts_profile_enable": ([i], i),
    "stts_profile_read": ([pd, pll, pd, pd], i),
    "stts_profile_launch": ([ll, pi, pd], i),
    # diagnostics and testing hooks (not product paths)
    "stts_calib_traffic": ([i, vp, ll, i, i, i, i, vp, vp], i),
    "stts_test_fxsum": ([i, vp, ll, vp, vp, vp], i),
    "stts_test_conv1d": ([i, vp, i, i, i, vp, vp, i, i, i, i, i, i, i, i, vp, vp, f, vp, f, vp, i, vp], i),

    # ================================================================== include/stts2_train.h
    "stts_snake_workspace_bytes": ([i, i, i], ll),
    "stts_snake_fwd": ([vp, vp, i, i, i, vp, vp], i),
    "stts_snake_bwd": ([vp, vp, vp, i, i, i, vp, vp, vp, ll, vp], i),
    "stts_tanh_fwd": ([vp, ll, vp, vp], i),
    "stts_tanh_bwd": ([vp, vp, ll, vp, vp], i),
    "stts_sum_div": ([vp, i, ll, f, vp, vp], i),
    "stts_div": ([vp, ll, f, vp, vp], i),
    "stts_source_workspace_bytes": ([i, i], ll),
    "stts_source_fwd": ([vp, vp, vp, vp, ull, ll, i, i, i, vp, vp, vp, ll, vp], i),
    "stts_source_fwd_seed_dev": ([vp, vp, vp, vp, vp, ll, i, i, i, vp, vp, vp, ll, vp], i),
    "stts_source_bwd": ([vp, vp, vp, i, ll, vp, vp, vp, ll, vp], i),
    "stts_box_smooth_fwd": ([vp, i, i, i, vp, vp], i),
    "stts_box_smooth_bwd": ([vp, i, i, i, vp, vp], i),
    "stts_time_expand3": ([vp, i, i, i, i, vp, vp], i),
    "stts_time_expand3_bwd": ([vp, i, i, i, i, vp, vp], i),
    "stts_stft_mag_workspace_bytes": ([i, ll, i, i, i], ll),
    "stts_stft_mag_fwd": ([vp, i, ll, ll, i, i, i, vp, vp, vp], i),
    "stts_stft_mag_bwd": ([vp, vp, i, ll, i, i, i, vp, vp, ll, vp], i),
    "stts_mrstft_bwd_workspace_bytes": ([i, ll, vp, vp, vp, i, i], ll),
    "stts_mrstft_loss_bwd": ([vp, vp, i, ll, ll, vp, vp, vp, i, i, i, vp, vp, vp, ll, vp], i),
    # GAN loss terms, AdamW
    "stts_gan_workspace_bytes": ([i], ll),
    "stts_gan_loss": ([vp, i, vp, vp, ll, vp], i),
    "stts_gan_loss_bwd": ([vp, vp, vp, i, vp, vp, ll, vp], i),
    "stts_adamw_step": ([vp, i, d, d, d, d, d, ll, vp], i),
    "stts_adamw_step_dev": ([vp, i, d, d, d, d, d, vp, vp], i),
    # ProsodyPredictor.F0Ntrain: the training BiLSTM
    "stts_bilstm_fwd_train": ([vp, ll, ll, ll, i, i, i, vp, vp, i, vp, vp, vp, ll, vp], i),
    "stts_bilstm_bwd_workspace_bytes": ([i, i, i, i], ll),
    "stts_bilstm_bwd": ([vp, i, i, i, vp, vp, i, vp, vp, vp, vp, vp, vp, ll, vp], i),
    # text / duration path
    "stts_row_norm_bwd_workspace_bytes": ([i, i, i], ll),
    "stts_row_norm_bwd": ([vp, ll, ll, ll, i, i, i, i, vp, vp, ll, f, i, f, vp, vp, ll, ll, i, vp, vp, vp, vp, vp, vp,
                           ll, vp], i),
    "stts_embedding_bwd": ([vp, i, i, vp, vp, ll, ll, i, i, vp, vp], i),
    "stts_dur_losses_workspace_bytes": ([i], ll),
    "stts_dur_losses": ([vp, ll, ll, i, i, i, vp, vp, ll, vp, vp, vp, vp, vp, ll, vp], i),
    "stts_dropout": ([vp, ll, f, ull, vp, vp], i),
    "stts_dropout_mask": ([vp, vp, ll, f, vp, vp], i),
    # StyleEncoder
    "stts_rowexp_fwd": ([vp, i, i, i, i, i, i, vp, vp], i),
    "stts_rowexp_bwd": ([vp, i, i, i, i, i, i, vp, vp], i),
    "stts_dwconv2d_s2_fwd": ([vp, vp, vp, i, i, i, i, vp, vp], i),
    "stts_dwconv2d_s2_workspace_bytes": ([i], ll),
    "stts_dwconv2d_s2_bwd": ([vp, vp, vp, i, i, i, i, vp, vp, vp, vp, ll, vp], i),
    "stts_avgpool2_fwd": ([vp, i, i, i, i, vp, vp], i),
    "stts_avgpool2_bwd": ([vp, i, i, i, i, vp, vp], i),
    "stts_spatial_mean_fwd": ([vp, i, i, i, vp, vp], i),
    "stts_spatial_mean_bwd": ([vp, i, i, i, vp, vp], i),
    "stts_smooth_l1_loss": ([vp, vp, ll, vp, vp], i),
    "stts_smooth_l1_loss_bwd": ([vp, vp, ll, vp, vp, vp, vp], i),
    # Vocos decoder
    "stts_dwconv1d_fwd": ([vp, vp, vp, i, i, i, i, vp, vp], i),
    "stts_dwconv1d_bwd_workspace_bytes": ([i, i, i, i], ll),
    "stts_dwconv1d_bwd": ([vp, vp, vp, i, i, i, i, vp, vp, vp, vp, ll, vp], i),
    "stts_gelu_fwd": ([vp, ll, vp, vp], i),
    "stts_gelu_bwd": ([vp, vp, ll, vp, vp], i),
    "stts_layer_scale_res_fwd": ([vp, vp, vp, i, i, i, vp, vp], i),
    "stts_layer_scale_res_bwd_workspace_bytes": ([i, i, i], ll),
    "stts_layer_scale_res_bwd": ([vp, vp, vp, i, i, i, vp, vp, vp, ll, vp], i),
    "stts_istft_head_workspace_bytes": ([i, i, i, i], ll),
    "stts_istft_head_fwd": ([vp, vp, i, i, i, i, vp, vp, ll, vp], i),
    "stts_istft_head_bwd": ([vp, vp, vp, i, i, i, i, vp, vp, ll, vp], i),
    # iSTFTNet decoder
    "stts_cstft_fwd": ([vp, vp, vp, i, i, i, i, vp, vp], i),
    "stts_padl_add_fwd": ([vp, vp, i, i, i, vp, vp], i),
    "stts_padl_add_bwd": ([vp, i, i, i, vp, vp], i),
    "stts_cistft_head_fwd": ([vp, vp, vp, i, i, i, i, vp, vp], i),
    "stts_cistft_head_bwd": ([vp, vp, vp, vp, i, i, i, i, vp, vp], i),
    # the aligner's S2S decoder under training, loss_s2s, loss_mono (params / grads: host arrays of 14 pointers)
    "stts_s2s_save_bytes": ([i, i, i], ll),
    "stts_s2s_fwd_train_workspace_bytes": ([i, i, i, i, i], ll),
    "stts_s2s_fwd_train": ([vp, vp, vp, vp, vp, i, i, i, i, i, vp, vp, vp, vp, vp, vp, ll, vp], i),
    "stts_s2s_bwd_workspace_bytes": ([i, i, i, i, i], ll),
    "stts_s2s_bwd": ([vp, vp, vp, vp, vp, i, i, i, i, i, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ll, vp], i),
    "stts_s2s_loss_workspace_bytes": ([i], ll),
    "stts_s2s_loss": ([vp, ll, ll, i, i, i, vp, ll, vp, vp, vp, vp, vp, ll, vp], i),
    "stts_mono_loss": ([vp, vp, ll, vp, vp, vp, vp], i),
    # the aligner's conv stack under training: GroupNorm with kept statistics, dropout + residual, MFCC frames
    "stts_groupnorm_fwd_train_workspace_bytes": ([i, i, i, i], ll),
    "stts_groupnorm_fwd_train": ([vp, vp, vp, i, i, i, i, i, f, ull, vp, vp, vp, vp, ll, vp], i),
    "stts_groupnorm_bwd_workspace_bytes": ([i, i, i, i], ll),
    "stts_groupnorm_bwd": ([vp, vp, vp, vp, i, i, i, i, i, f, ull, vp, vp, vp, vp, vp, ll, vp], i),
    "stts_dropout_add_fwd": ([vp, vp, ll, f, ull, vp, vp, vp], i),
    "stts_mfcc_frames": ([vp, vp, i, i, i, i, vp, vp], i),
}
