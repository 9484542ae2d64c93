"""ctypes binding of libidiaptts_amd.so (the C ABI declared in include/idiaptts_amd.h).

The product path has NO CPU fallback: if the HIP library is missing or a call fails this module
raises.  (cffi is not available in the target image, hence ctypes.)
"""
import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int64, c_uint8, c_uint32, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_lib", "libidiaptts_amd.so")

_lib = None


class IttsError(RuntimeError):
    pass


_P = c_void_p  # device / host pointers travel as integers

_SIGNATURES = {
    "itts_abi_version": (c_int, []),
    "itts_last_error": (c_char_p, []),
    "itts_device_count": (c_int, []),
    "itts_release_scratch": (c_int, []),
    "itts_defer_reductions": (c_int, [c_int]),
    "itts_reduce_deferred": (c_int, [_P]),
    "itts_scratch_pool_stats": (c_int, [POINTER(c_int64), POINTER(c_int64), POINTER(c_int64)]),
    "itts_comm_version": (c_int, []),
    "itts_comm_unique_id": (c_int, [_P]),
    "itts_comm_init_rank": (c_int, [_P, c_int, c_int, POINTER(c_void_p)]),
    "itts_comm_destroy": (c_int, [c_void_p]),
    "itts_allreduce_flat": (c_int, [_P, c_int64, c_int, c_int, c_void_p, _P]),
    "itts_cheaptrick_fft_size": (c_int, [c_int, c_double]),
    "itts_num_aperiodicities": (c_int, [c_int]),
    "itts_mcep_alpha": (c_double, [c_int]),
    "itts_world_num_frames": (c_int64, [c_int64, c_int, c_double]),
    "itts_world_synth_length": (c_int64, [c_int64, c_int, c_double]),
    "itts_wav_info": (c_int, [c_char_p, POINTER(c_int), POINTER(c_int64)]),
    "itts_wav_read_batch": (c_int, [POINTER(c_char_p), c_int, POINTER(c_int64), c_double, _P,
                                    c_int]),
    "itts_write_feature_archives": (c_int, [_P, c_int64, POINTER(c_int64), c_int,
                                            POINTER(c_char_p), c_int, POINTER(c_int),
                                            POINTER(c_int), POINTER(c_int), POINTER(c_char_p),
                                            c_int, _P]),
    "itts_questions_load": (c_int, [c_char_p, POINTER(c_void_p), POINTER(c_int), POINTER(c_int)]),
    "itts_questions_free": (None, [c_void_p]),
    "itts_questions_vector": (c_int, [c_void_p, c_char_p, _P]),
    "itts_labels_count_frames": (c_int, [POINTER(c_char_p), c_int, POINTER(c_int64), c_int]),
    "itts_labels_generate": (c_int, [c_void_p, POINTER(c_char_p), c_int, POINTER(c_int64), _P,
                                     c_int64, c_int]),
    "itts_normalise_rows_f32": (c_int, [_P, c_int64, c_int, _P, _P, _P]),
    "itts_mlpg_scratch_bytes": (c_int64, [c_int64, c_int]),
    "itts_mlpg_generation": (c_int, [_P, c_int64, c_int, c_int, _P, POINTER(c_int64), c_int, _P,
                                     c_int64, c_int, _P, _P]),
    "itts_mlpg_scratch_bytes_f32": (c_int64, [c_int64, c_int]),
    "itts_mlpg_generation_f32": (c_int, [_P, c_int64, c_int, c_int, _P, POINTER(c_int64), c_int, _P,
                                         c_int64, c_int, _P, _P]),
    "itts_lf0_vuv": (c_int, [_P, POINTER(c_int64), c_int, c_double, c_float, _P, _P, _P]),
    "itts_interpolate_lin_f32": (c_int, [_P, POINTER(c_int64), c_int, _P, _P, _P]),
    "itts_assemble_cmp_f32": (c_int, [_P, c_int64, c_int, _P, _P, _P, c_int64, c_int,
                                      POINTER(c_int64), c_int, c_int, _P, c_int64, _P]),
    "itts_feature_stats_workspace_bytes": (c_int64, [c_int, c_int]),
    "itts_feature_stats": (c_int, [_P, c_int64, c_int64, c_int, c_int, c_int, c_int, _P, _P, _P,
                                   _P]),
    "itts_linear_fwd": (c_int, [_P, c_int64, _P, _P, _P, c_int64, c_int64, c_int, c_int, c_int,
                                _P]),
    "itts_rows_gather_f32": (c_int, [_P, c_int64, c_int64, _P, c_int64, c_int, _P, _P, c_int64, c_int, _P]),
    "itts_mlpg_plan_create": (c_int, [_P, c_int, POINTER(c_void_p)]),
    "itts_mlpg_plan_destroy": (None, [_P]),
    "itts_mlpg_plan_frames": (c_int64, [_P]),
    "itts_mlpg_generation_planned": (c_int, [_P, _P, c_int, c_int64, c_int, c_int, _P, _P, c_int64, c_int, _P, _P]),
    "itts_mlpg_choose_form": (c_int, [c_int, c_int, c_int64, c_int64, c_int]),
    "itts_mlpg_set_override": (c_int, [c_int, c_int, c_int]),
    "itts_mlpg_get_override": (c_int, [POINTER(c_int), POINTER(c_int), POINTER(c_int)]),
    "itts_mlpg_last_form": (c_int, []),
    "itts_mlpg_adjoint_scratch_bytes": (c_int64, [c_int64, c_int]),
    "itts_mlpg_adjoint": (c_int, [_P, c_int, c_int64, c_int, c_int, _P, POINTER(c_int64), c_int, _P, c_int, c_int64,
                                  c_int, _P, _P]),
    "itts_mlpg_adjoint_planned": (c_int, [_P, _P, c_int, c_int64, c_int, c_int, _P, _P, c_int, c_int64, c_int, _P, _P]),
    "itts_mlpg_adjoint_choose_form": (c_int, [c_int, c_int, c_int64, c_int64]),
    "itts_mlpg_adjoint_set_override": (c_int, [c_int]),
    "itts_mlpg_adjoint_get_override": (c_int, []),
    "itts_mlpg_adjoint_last_form": (c_int, []),
    "itts_sqrt_inplace_f64": (c_int, [_P, c_int64, _P]),
    "itts_square_inplace_f64": (c_int, [_P, c_int64, _P]),
    "itts_stft": (c_int, [_P, POINTER(c_int64), POINTER(c_int64), POINTER(c_int64), c_int, c_int, c_int, c_int, _P,
                          c_int, _P, c_int64, _P]),
    "itts_stft_mel": (c_int, [_P, POINTER(c_int64), POINTER(c_int64), POINTER(c_int64), c_int, c_int, c_int, c_int,
                              _P, _P, _P, c_int, _P, c_int64, _P]),
    "itts_mel_project": (c_int, [_P, c_int64, c_int, c_int64, _P, _P, c_int, _P, c_int64, _P]),
    "itts_griffinlim": (c_int, [_P, _P, _P, _P, POINTER(c_int64), c_int, c_int, c_int, c_int, _P, c_int, c_double,
                                c_int, _P, _P]),
    "itts_griffinlim_tile_frames": (c_int, [c_int, c_int]),
    "itts_mel_inverse": (c_int, [_P, c_int64, c_int, c_int64, c_int, c_int, _P, _P, _P, _P, c_double, c_double, c_int,
                                 c_int, _P, c_int64, c_int, _P, _P]),
    "itts_batch_pad_gather_f32": (c_int, [_P, c_int64, c_int64, _P, _P, c_int, c_int64, c_int, c_int, _P, c_int64, _P,
                                          _P, c_int64, _P, _P]),
    "itts_batch_pack_rows_f32": (c_int, [_P, c_int64, _P, _P, c_int, c_int64, c_int, c_int, _P, c_int64, c_int,
                                         c_int64, c_int64, _P]),
    "itts_batch_concat_rows_f32": (c_int, [_P, c_int64, c_int64, _P, _P, _P, c_int, c_int64, c_int, _P, c_int64, c_int,
                                           _P]),
    "itts_batch_pad_colsum_workspace_bytes": (c_int64, [c_int64, c_int]),
    "itts_batch_pad_colsum_f32": (c_int, [_P, c_int64, _P, c_int, c_int64, c_int, c_int, _P, c_int, _P, _P]),
    "itts_linear_fwd_mse_workspace_bytes": (c_int64, [c_int64, c_int]),
    "itts_linear_fwd_mse": (c_int, [_P, c_int64, _P, _P, _P, c_int64, _P, c_double, c_float, c_int64,
                                    c_int, c_int, _P, _P, c_int64, _P, _P]),
    "itts_sparse_rows_layout": (c_int, [c_int64, c_int, POINTER(c_int64)]),
    "itts_sparse_rows_build": (c_int, [_P, c_int64, c_int64, c_int, _P, c_int, _P]),
    "itts_linear_fwd_sparse": (c_int, [_P, _P, c_int64, _P, _P, _P, c_int64, c_int64, c_int, c_int, c_int, _P]),
    "itts_sparse_path_counts": (c_int, [POINTER(c_int64)]),
    "itts_sparse_cols_plan_ints": (c_int, []),
    "itts_sparse_cols_layout": (c_int, [c_int64, c_int, POINTER(c_int64)]),
    "itts_sparse_cols_build": (c_int, [_P, c_int64, c_int64, c_int, _P, _P, _P]),
    "itts_sparse_cols_build_from_rows": (c_int, [_P, c_int64, c_int, c_int, _P, _P, _P]),
    "itts_linear_bwd_weight_sparse_workspace_bytes": (c_int64, [c_int64, c_int, c_int, c_int64]),
    "itts_linear_bwd_weight_sparse": (c_int, [_P, c_int64, _P, _P, _P, c_int64, _P, c_int64, _P, c_int64, c_int,
                                              c_int, _P, c_int, _P]),
    "itts_sparse_wgrad_counts": (c_int, [POINTER(c_int64)]),
    "itts_act_bwd": (c_int, [_P, _P, _P, c_int64, c_int, _P]),
    "itts_linear_bwd_input": (c_int, [_P, c_int64, _P, _P, c_int64, _P, c_int64, c_int, c_int64,
                                      c_int, c_int, _P]),
    "itts_linear_bwd_weight_workspace_bytes": (c_int64, [c_int64, c_int, c_int]),
    "itts_linear_bwd_weight": (c_int, [_P, c_int64, _P, c_int64, _P, _P, c_int64, c_int, c_int,
                                       _P, c_int, _P]),
    "itts_linear_bwd": (c_int, [_P, c_int64, _P, c_int64, _P, _P, _P, _P, c_int64, _P, c_int64, c_int,
                                c_int64, c_int, c_int, _P, c_int, _P]),
    "itts_dropout_apply": (c_int, [_P, c_int64, _P, c_int64, c_int64, c_int, c_int, c_double, c_uint64, c_uint32,
                                   c_int64, _P]),
    "itts_dropout_act_bwd": (c_int, [_P, c_int64, _P, c_int64, _P, c_int64, c_int64, c_int, c_int, c_double, c_uint64,
                                     c_uint32, c_int64, _P]),
    "itts_linear_fwd_dropout": (c_int, [_P, c_int64, _P, _P, _P, c_int64, c_int64, c_int, c_int, c_int, c_double,
                                        c_uint64, c_uint32, c_int64, _P]),
    "itts_linear_bwd_input_dropout": (c_int, [_P, c_int64, _P, _P, c_int64, _P, c_int64, c_int, c_int64, c_int, c_int,
                                              c_double, c_uint64, c_uint32, c_int64, _P]),
    "itts_linear_bwd_dropout": (c_int, [_P, c_int64, _P, c_int64, _P, _P, _P, _P, c_int64, _P, c_int64, c_int,
                                        c_int64, c_int, c_int, _P, c_int, c_double, c_uint64, c_uint32, c_int64, _P]),
    "itts_linear_fwd_sparse_dropout": (c_int, [_P, _P, c_int64, _P, _P, _P, c_int64, c_int64, c_int, c_int, c_int,
                                               c_double, c_uint64, c_uint32, c_int64, _P]),
    "itts_conv1d_fwd": (c_int, [_P, c_int64, _P, _P, _P, c_int64, c_int, c_int, c_int, c_int, c_int,
                                c_int, c_int, c_int, c_int, _P]),
    "itts_conv1d_bwd_input": (c_int, [_P, c_int64, _P, _P, c_int64, _P, c_int64, c_int, c_int, c_int,
                                      c_int, c_int, c_int, c_int, c_int, c_int, _P]),
    "itts_conv1d_bwd_weight_workspace_bytes": (c_int64, [c_int, c_int, c_int, c_int, c_int, c_int,
                                                         c_int]),
    "itts_conv1d_bwd_weight": (c_int, [_P, c_int64, _P, c_int64, _P, _P, c_int, c_int, c_int, c_int,
                                       c_int, c_int, c_int, c_int, _P, c_int, _P]),
    "itts_conv1d_plan": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, POINTER(c_int),
                                 POINTER(c_int), POINTER(c_int64)]),
    "itts_layernorm_fwd": (c_int, [_P, c_int64, _P, _P, _P, c_int64, _P, _P, c_int64, c_int, c_double, c_int, _P]),
    "itts_layernorm_workspace_bytes": (c_int64, [c_int64, c_int]),
    "itts_layernorm_bwd": (c_int, [_P, c_int64, _P, c_int64, _P, c_int64, _P, _P, _P, _P, c_int64, _P, _P, c_int64,
                                   c_int, c_int, _P, _P]),
    "itts_attention_workspace_bytes": (c_int64, [c_int, c_int, c_int]),
    "itts_attention_fwd": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int64, c_int64, c_double, c_uint64,
                                   c_uint32, _P]),
    "itts_attention_bwd": (c_int, [_P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int64, c_int64, c_double,
                                   c_uint64, c_uint32, _P]),
    "itts_allpass_warp_fwd": (c_int, [_P, c_int64, _P, _P, _P, _P, c_int64, c_int64, c_int, c_int, _P]),
    "itts_allpass_warp_bwd": (c_int, [_P, c_int64, _P, c_int64, _P, _P, _P, _P, c_int64, _P, c_int64, c_int, c_int,
                                      _P]),
    "itts_time_pool_plan": (c_int, [c_int, c_int64, c_int, POINTER(c_int), POINTER(c_int), POINTER(c_int64)]),
    "itts_time_pool_fwd": (c_int, [_P, c_int64, _P, c_int, c_int64, c_int, c_int, c_int, _P, c_int64, _P, _P]),
    "itts_time_pool_bwd": (c_int, [_P, c_int64, _P, c_int, c_int64, c_int, c_int, c_int, _P, c_int64, _P]),
    "itts_vae_reparam_fwd": (c_int, [_P, c_int64, _P, c_int64, _P, c_int64, c_int64, c_int, _P]),
    "itts_vae_reparam_bwd": (c_int, [_P, c_int64, _P, c_int64, _P, c_int64, _P, c_int64, _P, c_int64, _P, c_int64,
                                     c_int64, c_int, _P]),
    "itts_vae_kld_workspace_bytes": (c_int64, [c_int64, c_int]),
    "itts_vae_kld": (c_int, [_P, c_int64, _P, c_int64, _P, c_int64, c_int, _P, _P, c_int64, _P, c_int64, _P, _P, _P]),
    "itts_xent_plan": (c_int, [c_int64, c_int, c_int, POINTER(c_int), POINTER(c_int)]),
    "itts_softmax_xent_workspace_bytes": (c_int64, [c_int64, c_int]),
    "itts_softmax_xent": (c_int, [_P, c_int64, _P, _P, _P, c_int64, c_int, c_int64, _P, _P, _P, c_int64, _P, _P]),
    "itts_softmax_xent_strided_workspace_bytes": (c_int64, [c_int, c_int64]),
    "itts_softmax_xent_strided": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int64, c_int, c_int64, _P, _P, _P, _P, _P]),
    "itts_class_counts": (c_int, [_P, c_int64, _P, c_int64, c_int, _P, _P, _P, _P]),
    "itts_masked_mse_workspace_bytes": (c_int64, [c_int64, c_int]),
    "itts_masked_mse": (c_int, [_P, c_int64, _P, c_int64, _P, c_int64, c_int, c_double, c_float,
                                _P, _P, c_int64, _P, _P]),
    "itts_weighted_loss": (c_int, [_P, c_int64, _P, c_int64, _P, c_int64, c_int, c_int, _P, _P,
                                   c_int64, _P, c_int64, _P, _P]),
    "itts_cheaptrick_mcep": (c_int, [_P, POINTER(c_int64), _P, POINTER(c_int64), c_int, c_int,
                                     c_double, c_int, c_double, _P, c_int, c_double, c_double,
                                     c_int, c_int, c_double, _P, c_int64, _P, _P, _P]),
    "itts_mcep": (c_int, [_P, c_int64, c_int, c_int, c_double, c_double, c_int, c_int, c_double,
                          _P, c_int64, _P, _P, _P]),
    "itts_mgc2sp": (c_int, [_P, c_int64, c_int, c_double, c_int, _P, _P, _P, _P]),
    "itts_mgcep": (c_int, [_P, c_int, c_int64, c_int, c_int, c_double, c_double, c_double, c_int,
                           c_int, c_double, _P, c_int64, _P, _P, _P]),
    "itts_mgc2sp_gamma": (c_int, [_P, c_int64, c_int, c_double, c_double, c_int, _P, _P, _P, _P]),
    "itts_code_aperiodicity": (c_int, [_P, c_int64, c_int, c_int, _P, _P, _P]),
    "itts_decode_aperiodicity": (c_int, [_P, c_int64, c_int, c_int, _P, _P]),
    "itts_decode_aperiodicity_voiced": (c_int, [_P, _P, c_int64, c_int, c_int, _P, _P]),
    "itts_stonemask": (c_int, [_P, POINTER(c_int64), _P, POINTER(c_int64), c_int, c_int, c_double,
                               _P, _P]),
    "itts_d4c": (c_int, [_P, POINTER(c_int64), _P, POINTER(c_int64), c_int, c_int, c_double, c_int,
                         c_double, _P, _P, _P, c_int64, _P]),
    "itts_dio": (c_int, [_P, POINTER(c_int64), POINTER(c_int64), c_int, c_int, c_double, c_double,
                         c_double, c_double, c_double, _P, _P]),
    "itts_harvest_num_frames": (c_int64, [c_int64, c_int, c_double]),
    "itts_harvest": (c_int, [_P, POINTER(c_int64), POINTER(c_int64), c_int, c_int, c_double, c_double,
                             c_double, _P, _P, _P, _P, _P, _P]),
    "itts_wav2world": (c_int, [_P, POINTER(c_int64), POINTER(c_int64), c_int, c_int, c_double, c_int,
                               _P, _P, _P, _P]),
    "itts_world_synthesize": (c_int, [_P, _P, _P, POINTER(c_int64), POINTER(c_int64), c_int, c_int,
                                      c_double, c_int, c_double, _P, _P, _P]),
    "itts_world_synthesize_after": (c_int, [_P, _P, _P, POINTER(c_int64), POINTER(c_int64), c_int, c_int,
                                      c_double, c_int, c_double, _P, _P, _P, _P, _P]),
    "itts_lstm_state_bytes": (c_int64, [c_int, c_int, c_int]),
    "itts_lstm_layer_fwd": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, _P,
                                    _P, _P, _P, _P, _P, _P]),
    "itts_lstm_layer_bwd": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, _P,
                                    _P, _P, _P]),
    "itts_gru_state_bytes": (c_int64, [c_int, c_int, c_int]),
    "itts_gru_layer_fwd": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, _P,
                                   _P, _P, _P, _P]),
    "itts_gru_layer_bwd": (c_int, [_P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, _P,
                                   _P, _P, _P, _P]),
    "itts_rnn_layer_state_bytes": (c_int64, [c_int, c_int, c_int]),
    "itts_rnn_layer_fwd": (c_int, [_P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, _P]),
    "itts_rnn_layer_bwd": (c_int, [_P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, _P, _P, _P]),
    "itts_rnn_layer_counts": (c_int, [POINTER(c_int64)]),
    "itts_rnn_path_counts": (c_int, [POINTER(c_int64)]),
    "itts_gemm_path_counts": (c_int, [POINTER(c_int64)]),
    "itts_gemm_last_plan": (c_int, [POINTER(ctypes.c_int32), c_int]),
    "itts_adam_step": (c_int, [_P, _P, _P, _P, c_int64, c_float, c_float, c_float, c_float,
                               c_float, c_int64, c_float, _P]),
    "itts_grad_norm_accum": (c_int, [_P, c_int64, c_int, _P, c_int, _P, _P]),
    "itts_adam_step_fused": (c_int, [_P, _P, _P, _P, c_int64, c_float, c_float, c_float, c_float,
                                     c_float, c_int64, c_float, _P, c_int, c_float, c_float, _P,
                                     c_float, _P]),
    "itts_sgd_step": (c_int, [_P, _P, _P, c_int64, c_float, c_float, c_float, c_float, c_int,
                              c_int, c_float, _P]),
    "itts_ema_update": (c_int, [_P, _P, c_int64, c_float, _P]),
    "itts_fir_filtfilt_workspace_bytes": (c_int64, [c_int64, c_int, c_int]),
    "itts_fir_filtfilt_batch": (c_int, [_P, POINTER(c_int64), c_int, _P, c_int, _P, _P, _P]),
    "itts_resample_poly_batch": (c_int, [_P, POINTER(c_int64), POINTER(c_int64), c_int, c_int, c_int, _P, c_int, _P,
                                         _P]),
    "itts_loudness_normalise_batch": (c_int, [_P, POINTER(c_int64), c_int, c_double, _P, _P]),
    "itts_frame_rms_batch": (c_int, [_P, POINTER(c_int64), POINTER(c_int64), c_int, c_int, c_int, c_int, _P, _P]),
    "itts_mol_loss_workspace_bytes": (c_int64, [c_int, c_int64]),
    "itts_mol_loss": (c_int, [_P, _P, _P, c_int, c_int, c_int64, c_int, c_int, c_double, c_int, _P, _P, _P, _P, _P]),
    "itts_mulaw_encode_f64": (c_int, [_P, POINTER(c_int64), c_int, c_int, _P, _P]),
    "itts_mulaw_decode": (c_int, [_P, POINTER(c_int64), c_int, c_int, _P, _P]),
    "itts_mulaw_onehot": (c_int, [_P, POINTER(c_int64), POINTER(c_int64), c_int, c_int, _P, _P]),
    "itts_sample_linearly": (c_int, [_P, c_int, POINTER(c_int64), c_int, c_int, c_int, _P, c_int, _P]),
    "itts_glu_gate_fwd": (c_int, [_P, c_int64, _P, c_int64, _P, c_int64, c_int64, c_int, _P]),
    "itts_glu_gate_bwd": (c_int, [_P, c_int64, _P, c_int64, _P, c_int64, _P, c_int64, c_int64, c_int, _P]),
    "itts_wavenet_state_floats": (c_int64, [c_int, c_int, c_int, c_int, POINTER(c_int)]),
    "itts_wavenet_generate": (c_int, [_P] * 10 + [POINTER(c_int), c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                      c_int, c_double, _P, c_int64, _P, POINTER(c_int), c_int, c_int64, c_int, _P,
                                      c_int64, _P, _P, _P]),
    "itts_vocoder_windows": (c_int, [_P, c_int64, _P, c_int64, c_int, c_int, c_int, POINTER(c_int64), c_int, c_int64,
                                     _P, _P, _P]),
    "itts_fixed_attention_plan": (c_int, [c_int, c_int64, c_int, c_int, c_int, c_int, POINTER(c_int64)]
                                  + [POINTER(c_int)] * 6),
    "itts_fixed_attention_fwd": (c_int, [_P, c_int64, c_int64, _P, c_int64, c_int64, c_int, c_int64, c_int, c_int,
                                         c_int, c_int, _P, c_int64, c_int64, _P, c_int64, c_int64, _P]),
    "itts_fixed_attention_bwd": (c_int, [_P, c_int64, c_int64, _P, c_int64, c_int64, c_int, c_int64, c_int, c_int, _P,
                                         c_int64, c_int64, _P]),
    "itts_rnn_cell_step": (c_int, [c_int, c_int, _P, c_int64, _P, c_int64, _P, _P, c_int64, _P, c_int64, c_int, c_int,
                                   _P, c_int64, _P, c_int64, _P]),
    "itts_dtw_workspace_bytes": (c_int64, [c_int, c_int, c_int]),
    "itts_dtw_plan": (c_int, [c_int, c_int, c_int, POINTER(c_int), POINTER(c_int), POINTER(c_int)]),
    "itts_dtw_align": (c_int, [_P, c_int64, c_int64, _P, c_int64, c_int64, c_int, POINTER(ctypes.c_int32),
                               POINTER(ctypes.c_int32), c_int, c_int, c_int, c_int, c_int, _P, _P, _P, c_int64, _P,
                               c_int64, _P]),
    "itts_dtw_step_probe": (c_int, [c_int, c_int, _P, _P]),
}


def declared_symbols():
    """Every symbol include/idiaptts_amd.h declares (kept in sync by tests/test_abi.py)."""
    return sorted(_SIGNATURES)


def load():
    """Loads the shared library (building is the job of __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise IttsError(
            "HIP library {} is missing. Build it with `python -m idiaptts_amd.build` "
            "(there is no CPU fallback).".format(LIB_PATH))
    # torch first: its wheel carries a HIP runtime of its own, and the process must end up with ONE -- loaded the other
    # way round (this library pulling in /opt/rocm's copy before torch brings its own) the two runtimes do not know
    # each other's devices and allocations: "no ROCm-capable device is detected" from the first call that allocates
    # (seen with __graft_entry__.build() followed by smoke() in one process)
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(status, what=""):
    if status != 0:
        msg = load().itts_last_error()
        raise IttsError("{} failed with status {}: {}".format(
            what or "libidiaptts_amd call", status, msg.decode() if msg else ""))


def offsets_array(offsets):
    """A host int64 array for the `const int64_t*` offset parameters, from a list / tuple / numpy array (through
    numpy: a quarter of the time of converting element by element -- 10 instead of 36 us for 257 offsets, which is
    inside every timed call of the short entry points)."""
    import numpy as np
    arr = np.array(offsets, dtype=np.int64, order="C", ndmin=1)      # (a private, writable copy: from_buffer needs one)
    if arr.ndim != 1:
        raise ValueError("offsets must be one-dimensional")
    return (c_int64 * arr.shape[0]).from_buffer(arr)


def normalise_rows(sample, sub, div):
    """`((sample - sub) / div).astype(np.float32)` for the data readers' `preprocess_sample`: a float32 [rows, cols]
    sample with float64 per-column parameters goes through one pass of native code (itts_normalise_rows_f32: the same
    bits, without the float64 temporaries); anything else through numpy as written."""
    import numpy as np
    sub, div = np.asarray(sub), np.asarray(div)
    if (isinstance(sample, np.ndarray) and sample.dtype == np.float32 and sample.ndim == 2
            and sample.flags.c_contiguous and sub.dtype == np.float64 and div.dtype == np.float64
            and sub.shape == (sample.shape[1],) and div.shape == (sample.shape[1],)):
        try:
            L = load()
        except Exception:                        # library not built (documentation builds, linting): numpy
            L = None
        if L is not None:
            sub, div = np.ascontiguousarray(sub), np.ascontiguousarray(div)
            out = np.empty_like(sample)
            check(L.itts_normalise_rows_f32(sample.ctypes.data, sample.shape[0], sample.shape[1],
                                            sub.ctypes.data, div.ctypes.data, out.ctypes.data),
                  "itts_normalise_rows_f32")
            return out
    return ((sample - sub) / div).astype(np.float32, copy=False)


def current_stream():
    """Raw hipStream_t of torch's current stream (0 = default stream)."""
    import torch
    return torch.cuda.current_stream().cuda_stream


def require_gpu():
    import torch
    if not torch.cuda.is_available():
        raise IttsError("No HIP device visible: the idiaptts_amd hot path only runs on an "
                        "MI355X-class GPU (there is no CPU fallback).")
    load()
