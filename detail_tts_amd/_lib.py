"""ctypes binding of libdetail_hip.so (include/detail_hip.h).  Fails loudly when the library is missing —
there is NO CPU fallback in the product path."""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# DTTS_LIB_PATH: another build of the same library (diagnostic builds of tools/diag_token_pk.py); the default is the in-tree product library
LIB_PATH = os.environ.get("DTTS_LIB_PATH") or os.path.join(HERE, "libdetail_hip.so")

c_float_p = C.POINTER(C.c_float)
c_int_p = C.POINTER(C.c_int)
c_u64_p = C.POINTER(C.c_ulonglong)
c_i64_p = C.POINTER(C.c_longlong)

# slots of the loss entries' output (include/detail_hip.h: DTTS_DISC_LOSS_FM and the slots after it)
DISC_COUNT, DISC_MAPS = 6, 37
DISC_LOSS_FM, DISC_LOSS_DISC, DISC_LOSS_GEN, DISC_LOSSES_R, DISC_LOSSES_G, DISC_LOSSES_GEN, DISC_MAP_MEANS = 0, 1, 2, 3, 9, 15, 21
DISC_LOSS_MEL, DISC_LOSS_KL, DISC_LOSS_GEN_ALL, DISC_OUT_FLOATS = 58, 59, 60, 64


class DttsConfig(C.Structure):
    _fields_ = [
        ("diff_channels", C.c_int), ("diff_layers", C.c_int), ("diff_heads", C.c_int), ("mel_channels", C.c_int),
        ("diff_out_channels", C.c_int), ("diff_steps", C.c_int), ("diff_trained_steps", C.c_int), ("cond_free_k", C.c_float),
        ("gpt_dim", C.c_int), ("gpt_layers", C.c_int), ("gpt_heads", C.c_int), ("gpt_mel_codes", C.c_int),
        ("gpt_text_tokens", C.c_int), ("gpt_max_mel_pos", C.c_int), ("gpt_max_text_pos", C.c_int),
        ("inter_channels", C.c_int), ("hidden_channels", C.c_int), ("filter_channels", C.c_int), ("enc_heads", C.c_int),
        ("enc_layers", C.c_int), ("gin_channels", C.c_int), ("upsample_initial_channel", C.c_int), ("n_upsamples", C.c_int),
        ("upsample_rates", C.c_int * 8), ("upsample_kernels", C.c_int * 8), ("n_resblock_kernels", C.c_int),
        ("resblock_kernels", C.c_int * 4), ("resblock_dilations", C.c_int * 4),
    ]


class DttsGptRowOptions(C.Structure):
    """dtts_gpt_row_options: the sampling settings of one row of a decode session"""
    _fields_ = [("temperature", C.c_float), ("top_p", C.c_float), ("repetition_penalty", C.c_float), ("typical_mass", C.c_float),
                ("min_p", C.c_float), ("epsilon_cutoff", C.c_float), ("top_k", C.c_int), ("max_generate_length", C.c_int),
                ("no_repeat_ngram_size", C.c_int), ("min_length", C.c_int), ("min_new_tokens", C.c_int), ("exp_decay_start", C.c_int),
                ("exp_decay_factor", C.c_double), ("suppress_tokens", c_int_p), ("n_suppress_tokens", C.c_int),
                ("begin_suppress_tokens", c_int_p), ("n_begin_suppress_tokens", C.c_int)]


class DttsGptOptions(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("seed", C.c_ulonglong), ("sample_ids", c_int_p), ("max_generate_length", C.c_int), ("top_k", C.c_int),
                ("top_p", C.c_float), ("temperature", C.c_float), ("repetition_penalty", C.c_float), ("suppress_eos", C.c_int),
                ("forced_uniforms", C.c_void_p), ("forced_codes", c_int_p), ("row_seeds", c_u64_p),
                ("row_options", C.POINTER(DttsGptRowOptions)), ("typical_mass", C.c_float),
                ("no_repeat_ngram_size", C.c_int), ("min_length", C.c_int), ("min_new_tokens", C.c_int), ("exp_decay_start", C.c_int),
                ("exp_decay_factor", C.c_double), ("suppress_tokens", c_int_p), ("n_suppress_tokens", C.c_int),
                ("begin_suppress_tokens", c_int_p), ("n_begin_suppress_tokens", C.c_int), ("min_p", C.c_float), ("epsilon_cutoff", C.c_float),
                ("num_beams", C.c_int), ("length_penalty", C.c_float), ("early_stopping", C.c_int),
                ("token_wgs", C.c_int), ("prompt_codes", c_int_p), ("prompt_lens", c_int_p), ("prompt_stride", C.c_int)]


class DttsConvX3Info(C.Structure):
    _fields_ = [("epi", C.c_int), ("kw3", C.c_int), ("stages", C.c_int), ("ksplit", C.c_int), ("p1", C.c_int), ("epi_vec", C.c_int),
                ("cols", C.c_int), ("workgroups", C.c_int)]


class DttsAttnX3Info(C.Structure):
    _fields_ = [("conv", DttsConvX3Info), ("attn_ksplit", C.c_int), ("attn_p1", C.c_int), ("attn_workgroups", C.c_int)]


class DttsGemvInfo(C.Structure):
    _fields_ = [("slices", C.c_int), ("vec", C.c_int), ("rpw", C.c_int), ("nb", C.c_int)]


class DttsKernelStat(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("launches", C.c_longlong), ("total_ms", C.c_double), ("union_ms", C.c_double), ("flops", C.c_double),
                ("bytes", C.c_double)]


# name -> (restype, argtypes); every symbol include/detail_hip.h declares
SIGNATURES = {
    "dtts_version": (C.c_char_p, []),
    "dtts_default_config": (None, [C.POINTER(DttsConfig)]),
    "dtts_gpt_options_init": (None, [C.POINTER(DttsGptOptions)]),
    "dtts_create": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(DttsConfig), C.c_int]),
    "dtts_destroy": (C.c_int, [C.c_void_p]),
    "dtts_last_error": (C.c_char_p, [C.c_void_p]),
    "dtts_bind_weights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_char_p), c_u64_p, c_u64_p, C.c_int, C.c_void_p]),
    "dtts_vq_decode": (C.c_int, [C.c_void_p, c_int_p, c_int_p, C.c_int, C.c_void_p, c_int_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "dtts_vq_encode": (C.c_int, [C.c_void_p, C.c_void_p, c_int_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dtts_resample": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "dtts_mel_spectrogram": (C.c_int, [C.c_void_p, C.c_void_p, c_int_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "dtts_spectrogram": (C.c_int, [C.c_void_p, C.c_void_p, c_int_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "dtts_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "dtts_get_option": (C.c_int, [C.c_void_p, C.c_char_p, c_int_p]),
    "dtts_uncond_cache_stats": (C.c_int, [C.c_void_p, c_u64_p]),
    "dtts_profile_enable": (C.c_int, [C.c_int]),
    "dtts_profile_sampling": (C.c_int, [C.c_int]),
    "dtts_profile_report": (C.c_int, [C.POINTER(DttsKernelStat), C.c_int]),
    "dtts_gpt_generate": (C.c_int, [C.c_void_p, C.c_void_p, c_int_p, C.c_int, c_int_p, c_int_p, C.c_int, C.c_int,
                                    C.POINTER(DttsGptOptions), c_int_p, c_int_p, C.c_void_p, C.c_int, C.c_void_p]),
    "dtts_gpt_prefill": (C.c_int, [C.c_void_p, C.c_void_p, c_int_p, C.c_int, c_int_p, c_int_p, C.c_int, C.c_int,
                                   C.POINTER(DttsGptOptions), C.c_void_p, C.c_int, C.c_void_p]),
    "dtts_gpt_decode_step": (C.c_int, [C.c_void_p, C.c_void_p]),
    "dtts_gpt_decode": (C.c_int, [C.c_void_p, C.c_int, c_int_p, C.c_void_p]),
    "dtts_gpt_steps": (C.c_int, [C.c_void_p]),
    "dtts_gpt_all_finished": (C.c_int, [C.c_void_p, c_int_p, C.c_void_p]),
    "dtts_gpt_finish": (C.c_int, [C.c_void_p, c_int_p, c_int_p, C.c_void_p]),
    "dtts_op_sample_logits": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, c_int_p, C.c_int, C.c_void_p, C.c_int, C.c_float,
                                        C.c_float, C.c_float, c_int_p, C.c_void_p]),
    "dtts_op_sample_logits_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, c_int_p, C.c_int, C.c_void_p, C.c_int, C.c_float,
                                           C.c_float, C.c_float, C.c_float, C.c_int, c_int_p, C.c_void_p]),
    "dtts_op_sample_logits_opts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(DttsGptOptions), c_int_p, C.c_int, c_int_p,
                                             c_int_p, c_int_p, C.c_void_p, c_int_p, C.c_void_p]),
    "dtts_op_sample_logits_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(DttsGptOptions), C.POINTER(DttsGptRowOptions),
                                             c_int_p, C.c_int, c_int_p, c_int_p, c_int_p, C.c_void_p, c_int_p, C.c_void_p]),
    "dtts_gpt_beam_generate": (C.c_int, [C.c_void_p, C.c_void_p, c_int_p, C.c_int, c_int_p, c_int_p, C.c_int, C.c_int,
                                         C.POINTER(DttsGptOptions), C.c_int, c_int_p, c_int_p, c_float_p, C.c_void_p]),
    "dtts_gpt_beam_finish": (C.c_int, [C.c_void_p, C.c_int, c_int_p, c_int_p, c_float_p, C.c_void_p]),
    "dtts_op_beam_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(DttsGptOptions), C.c_int, c_int_p, C.c_int,
                                    c_int_p, c_float_p, c_int_p, c_float_p, c_int_p, c_int_p, c_int_p, c_int_p, c_int_p, c_int_p,
                                    c_float_p, c_int_p, c_int_p, C.c_void_p]),
    "dtts_gpt_first_stop_step": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "dtts_gpt_decay_multipliers": (None, [C.c_double, C.c_int, C.c_void_p]),
    "dtts_sampler_max_vocab": (C.c_int, []),
    "dtts_diff_p_sample": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, c_int_p, C.c_int, C.c_int, C.c_int, C.c_ulonglong, c_int_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p]),
    "dtts_gpt_latents": (C.c_int, [C.c_void_p, C.c_void_p, c_int_p, C.c_int, c_int_p, c_int_p, C.c_int, c_int_p, c_int_p, C.c_int,
                                   C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "dtts_gpt_score": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, c_int_p, c_int_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dtts_gpt_forward_losses": (C.c_int, [C.c_void_p, C.c_void_p, c_int_p, C.c_int, c_int_p, C.c_int, c_int_p, C.c_int, C.c_int, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dtts_voice_pool": (C.c_int, [C.c_void_p, C.c_void_p, c_float_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "dtts_wav_edges": (C.c_int, [C.c_void_p, C.c_void_p, c_int_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p]),
    "dtts_wav_join": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, c_int_p, c_int_p, c_int_p, C.c_longlong, C.c_int, C.c_void_p,
                                C.c_void_p]),
    "dtts_gpt_generate_cond": (C.c_int, [C.c_void_p, C.c_void_p, c_int_p, c_int_p, C.c_int, C.c_int, C.POINTER(DttsGptOptions), c_int_p, c_int_p,
                                         C.c_void_p, C.c_int, C.c_void_p]),
    "dtts_gpt_prefill_cond": (C.c_int, [C.c_void_p, C.c_void_p, c_int_p, c_int_p, C.c_int, C.c_int, C.POINTER(DttsGptOptions), C.c_void_p,
                                        C.c_int, C.c_void_p]),
    "dtts_gpt_beam_generate_cond": (C.c_int, [C.c_void_p, C.c_void_p, c_int_p, c_int_p, C.c_int, C.c_int, C.POINTER(DttsGptOptions), C.c_int,
                                              c_int_p, c_int_p, c_float_p, C.c_void_p]),
    "dtts_gpt_latents_cond": (C.c_int, [C.c_void_p, C.c_void_p, c_int_p, c_int_p, C.c_int, c_int_p, c_int_p, C.c_int, C.c_int, C.c_void_p,
                                        C.c_int, C.c_void_p]),
    "dtts_gpt_forward_losses_cond": (C.c_int, [C.c_void_p, C.c_void_p, c_int_p, C.c_int, c_int_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p]),
    "dtts_vq_decode_cond": (C.c_int, [C.c_void_p, c_int_p, c_int_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "dtts_diff_conditioning": (C.c_int, [C.c_void_p, C.c_void_p, c_int_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "dtts_diff_timestep_independent": (C.c_int, [C.c_void_p, C.c_void_p, c_int_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dtts_diff_timestep_independent_ex": (C.c_int, [C.c_void_p, C.c_void_p, c_int_p, C.c_int, C.c_int, C.c_void_p, c_int_p, c_int_p, C.c_int,
                                                    C.c_void_p, C.c_void_p]),
    "dtts_op_frame_map": (C.c_int, [C.c_void_p, c_int_p, c_int_p, c_int_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "dtts_diff_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, c_int_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "dtts_diff_sample": (C.c_int, [C.c_void_p, C.c_void_p, c_int_p, C.c_int, C.c_int, C.c_ulonglong, c_int_p, C.c_int, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "dtts_diff_schedule": (C.c_int, [C.c_void_p, c_int_p, C.c_int, c_int_p, C.c_void_p]),
    "dtts_diff_schedule_coefs": (C.c_int, [C.c_void_p, C.c_int, c_int_p, c_float_p, C.c_int, c_int_p]),
    "dtts_diff_sample_ex": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, c_int_p, C.c_int, C.c_int, C.c_ulonglong,
                                      c_int_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "dtts_diff_step": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, c_int_p, C.c_int, C.c_int, C.c_int,
                                 C.c_ulonglong, c_int_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dtts_diff_invert": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, c_int_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p]),
    "dtts_diff_sample_from": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p, c_int_p, C.c_int, C.c_int,
                                        C.c_ulonglong, c_int_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "dtts_diff_inpaint": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_void_p, c_int_p, C.c_int, C.c_int,
                                    C.c_ulonglong, c_int_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p]),
    "dtts_op_inpaint_blend": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, c_int_p, C.c_int, C.c_int, C.c_int, c_float_p,
                                        C.c_int, C.c_int, C.c_ulonglong, c_int_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dtts_inpaint_table": (C.c_int, [c_int_p, C.c_int, C.c_int, c_float_p, C.c_int, c_int_p]),
    "dtts_diff_reverse_step": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, c_int_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                         C.c_void_p]),
    "dtts_diff_mean_variance": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, c_int_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dtts_ddim_reverse_table": (C.c_int, [c_int_p, C.c_int, C.c_int, C.c_float, c_float_p, C.c_int, c_int_p]),
    "dtts_diff_forward_t": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, c_int_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                      C.c_void_p]),
    "dtts_dpm_schedule_table": (C.c_int, [C.c_int, c_float_p, c_float_p, c_float_p, C.c_int, c_int_p]),
    "dtts_diff_schedule_dpm": (C.c_int, [C.c_void_p, C.c_int, c_int_p, C.c_void_p]),
    "dtts_diff_step_dpm": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, c_int_p, C.c_int, C.c_int, C.c_int,
                                     C.c_void_p, C.c_void_p]),
    "dtts_diff_forward_tf": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, c_int_p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p,
                                       C.c_void_p]),
    "dtts_diff_forward_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, c_int_p, C.c_int, C.c_int, c_int_p, C.c_void_p,
                                         C.c_void_p]),
    "dtts_diff_schedule_qtable": (C.c_int, [C.c_void_p, C.c_int, c_float_p, C.c_int, c_int_p]),
    "dtts_diff_q_sample": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, c_int_p, C.c_void_p, C.c_ulonglong, c_int_p, C.c_int, C.c_int,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dtts_diff_loss_terms": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, c_int_p, C.c_int, C.c_int,
                                       C.c_void_p, C.c_void_p, C.c_void_p]),
    "dtts_diff_training_losses": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, c_int_p, C.c_void_p, C.c_ulonglong, c_int_p, C.c_void_p, c_int_p,
                                            C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dtts_diff_bpd_terms": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, c_int_p, C.c_int, C.c_int,
                                      C.c_void_p, C.c_void_p, C.c_void_p]),
    "dtts_diff_prior_bpd": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "dtts_diff_calc_bpd": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, c_int_p, C.c_int, C.c_int, C.c_void_p, C.c_ulonglong, c_int_p,
                                     C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dtts_l1_mean": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "dtts_posterior_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, c_int_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_ulonglong, c_int_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dtts_flow_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, c_int_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "dtts_slice_segments": (C.c_int, [C.c_void_p, C.c_void_p, c_int_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "dtts_kl_loss": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, c_int_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                               C.c_void_p]),
    "dtts_flowvae_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, c_int_p, C.c_int, C.c_int, C.c_void_p, C.c_ulonglong, c_int_p,
                                       c_int_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    "dtts_bind_discriminator": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_char_p), c_u64_p, c_u64_p, C.c_int, C.c_void_p]),
    "dtts_disc_layout": (C.c_int, [C.c_int, C.c_int, c_i64_p, c_int_p]),
    "dtts_disc_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "dtts_disc_losses": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), c_i64_p, C.c_int, C.POINTER(C.c_void_p),
                                   C.POINTER(C.c_void_p), c_i64_p, C.c_void_p, C.c_void_p]),
    "dtts_spec_to_mel": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "dtts_op_conv1d_grouped": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "dtts_op_period_split": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "dtts_flowvae_stage_work": (C.c_longlong, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "dtts_flowvae_stage_losses": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, c_int_p, C.c_int, C.c_int, C.c_void_p, C.c_ulonglong,
                                            c_int_p, c_int_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dtts_vocoder": (C.c_int, [C.c_void_p, C.c_void_p, c_int_p, C.c_int, C.c_int, C.c_ulonglong, c_int_p, C.c_float, C.c_void_p,
                               C.c_void_p, C.c_void_p, C.c_void_p]),
    "dtts_vocoder_stream": (C.c_int, [C.c_void_p, C.c_void_p, c_int_p, C.c_int, C.c_int, C.c_ulonglong, c_int_p, C.c_float, C.c_void_p,
                                      C.c_int, C.c_void_p, C.c_void_p]),
    "dtts_vocoder_ticket": (C.c_longlong, [C.c_void_p]),
    "dtts_vocoder_check": (C.c_int, [C.c_void_p, C.c_longlong]),
    "dtts_vocoder_check_active": (C.c_int, [C.c_void_p]),
    "dtts_generator": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, c_int_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "dtts_op_mel_style": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, c_int_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "dtts_op_attention_block": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, c_int_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "dtts_op_resblock": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, c_int_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "dtts_op_resblock1": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, c_int_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "dtts_op_wn": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, c_int_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "dtts_op_enc_p": (C.c_int, [C.c_void_p, C.c_void_p, c_int_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dtts_op_conv1d": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, c_int_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                 C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "dtts_op_conv1d_x3": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, c_int_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                    C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(DttsConvX3Info),
                                    C.c_void_p]),
    "dtts_attn_x3_image_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "dtts_op_attention_x3": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, c_int_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                       C.c_int, C.c_void_p, C.c_void_p, C.POINTER(DttsAttnX3Info), C.c_void_p]),
    "dtts_op_attention": (C.c_int, [C.c_void_p, C.c_void_p, c_int_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                    C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dtts_op_attention_rel": (C.c_int, [C.c_void_p, C.c_void_p, c_int_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                        C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dtts_gpt_attentions": (C.c_int, [C.c_void_p, C.c_void_p, c_int_p, C.c_int, c_int_p, c_int_p, C.c_int, c_int_p, c_int_p, C.c_int, C.c_int,
                                      c_int_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "dtts_gpt_attentions_cond": (C.c_int, [C.c_void_p, C.c_void_p, c_int_p, c_int_p, C.c_int, c_int_p, c_int_p, C.c_int, C.c_int, c_int_p,
                                           C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "dtts_gpt_text_alignment": (C.c_int, [C.c_void_p, C.c_void_p, c_int_p, C.c_int, c_int_p, c_int_p, C.c_int, c_int_p, c_int_p, C.c_int,
                                          C.c_int, c_int_p, C.c_int, c_float_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dtts_gpt_text_alignment_cond": (C.c_int, [C.c_void_p, C.c_void_p, c_int_p, c_int_p, C.c_int, c_int_p, c_int_p, C.c_int, C.c_int,
                                               c_int_p, C.c_int, c_float_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dtts_op_attn_probs": (C.c_int, [C.c_void_p, C.c_void_p, c_int_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_int, C.c_float, c_int_p, c_int_p, c_int_p, c_int_p, C.c_int, C.c_int, C.c_int, c_float_p, C.c_int,
                                     C.c_void_p, C.c_void_p]),
    "dtts_op_monotone_path": (C.c_int, [C.c_void_p, C.c_void_p, c_int_p, c_int_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "dtts_op_philox_normal": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_ulonglong, c_int_p, C.c_int, C.c_int, C.c_void_p]),
    "dtts_op_gemv_block": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                     C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(DttsGemvInfo), C.c_void_p]),
    "dtts_op_decode_attention": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_longlong, C.c_int, c_int_p, c_int_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                           C.c_void_p, C.c_void_p]),
    "dtts_op_gpt_final_ln": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, c_int_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "dtts_op_ln_fold_vectors": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    "dtts_op_kv_to_cache": (C.c_int, [C.c_void_p, C.c_void_p, c_int_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p]),
}

_lib = None


class LibraryMissing(RuntimeError):
    pass


def load():
    """dlopen libdetail_hip.so.  `import torch` first so our NEEDED libamdhip64.so binds to the HIP runtime torch
    already loaded (SURVEY.md §7 toolchain facts) and torch's streams are valid inside the library."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LibraryMissing(
            f"{LIB_PATH} not found — build it with `python -m detail_tts_amd.build` (hipcc, gfx950). "
            "There is no CPU fallback for the product path.")
    try:
        import torch  # noqa: F401
    except Exception:  # pragma: no cover
        pass
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib
