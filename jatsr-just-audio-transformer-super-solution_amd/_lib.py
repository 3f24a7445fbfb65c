"""ctypes binding of libjat_hip.so (C ABI: include/jat_hip.h).

There is deliberately no fallback: if the library is not built, or a compute entry point is called
without a GPU, this raises — the product path never routes through the CPU oracle.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# The trainer queues its weight-gradient GEMMs on a second stream beside the backward's dX chain, and exchanges gradients on a
# third.  ROCm maps a process's streams onto a limited number of hardware queues, and streams that share a queue run one
# after the other.  How many queues a process may open is left to the environment it runs in.
# JAT_OPERAND_DTYPE=fp16 selects the fp16-operand build of the same kernels for the whole process (the v3mod2 trainer's
# autocast dtype, train_ddp_v3mod2.py:854); JAT_LIB_PATH overrides everything (A/B of two builds)
OPERAND_DTYPE = os.environ.get("JAT_OPERAND_DTYPE", "bf16").lower()
if OPERAND_DTYPE not in ("bf16", "fp16", "float16", "bfloat16"):
    raise ValueError(f"JAT_OPERAND_DTYPE must be bf16 or fp16, got {OPERAND_DTYPE!r}")
OPERAND_DTYPE = "fp16" if OPERAND_DTYPE in ("fp16", "float16") else "bf16"
LIB_PATH = os.environ.get("JAT_LIB_PATH") or os.path.join(
    _HERE, "csrc", "libjat_hip_fp16.so" if OPERAND_DTYPE == "fp16" else "libjat_hip.so")

JAT_OK, JAT_E_INVALID, JAT_E_HIP, JAT_E_STATE, JAT_E_SEQLEN = 0, -1, -2, -3, -4
NORM_RMS_W, NORM_LN_NOAFFINE = 0, 1
FB_ACCUMULATE, FB_NO_HOOK = 1, 2   # JAT_FB_* flags of jat_trainer_fwd_bwd_ex


class JatConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "input_channels", "cond_channels", "patch_len", "hidden_size", "depth", "num_q_heads",
        "num_kv_heads", "bottleneck_dim", "mlp_hidden", "norm_mode")]


class JatDacConfig(C.Structure):
    _fields_ = [("latent_channels", C.c_int32), ("channels", C.c_int32), ("n_blocks", C.c_int32),
                ("strides", C.c_int32 * 4)]


class JatDacEncoderConfig(C.Structure):
    _fields_ = [("channels", C.c_int32), ("hidden_size", C.c_int32), ("n_blocks", C.c_int32), ("strides", C.c_int32 * 4),
                ("n_codebooks", C.c_int32), ("codebook_size", C.c_int32), ("codebook_dim", C.c_int32)]


class JatYinParams(C.Structure):
    _fields_ = [("fmin", C.c_double), ("fmax", C.c_double), ("sr", C.c_int32), ("frame_length", C.c_int32),
                ("hop_length", C.c_int32), ("trough_threshold", C.c_float)]


class JatPyinParams(C.Structure):
    _fields_ = [("fmin", C.c_double), ("fmax", C.c_double), ("sr", C.c_int32), ("frame_length", C.c_int32),
                ("hop_length", C.c_int32), ("n_thresholds", C.c_int32), ("beta_a", C.c_double), ("beta_b", C.c_double),
                ("boltzmann_parameter", C.c_double), ("resolution", C.c_double), ("max_transition_rate", C.c_double),
                ("switch_prob", C.c_double), ("no_trough_prob", C.c_double)]


class JatTensorRef(C.Structure):
    _fields_ = [("name", C.c_char_p), ("data", C.c_void_p), ("numel", C.c_int64)]


# name -> (restype, argtypes); every symbol include/jat_hip.h declares
_VP, _I32, _I64, _F32, _SZ = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_size_t
SIGNATURES = {
    "jat_last_error": (C.c_char_p, []),
    "jat_version": (C.c_int, []),
    "jat_operand_dtype": (C.c_int, []),
    "jat_model_create": (C.c_int, [C.POINTER(JatConfig), C.POINTER(_VP)]),
    "jat_model_destroy": (None, [_VP]),
    "jat_model_load_weights": (C.c_int, [_VP, C.POINTER(JatTensorRef), _I32, _VP]),
    "jat_model_set_switch": (C.c_int, [_VP, C.c_char_p, _I32]),
    "jat_model_workspace_bytes": (C.c_int, [_VP, _I32, _I32, C.POINTER(_SZ)]),
    "jat_forward": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _I32, _I32, _VP, _SZ, _VP]),
    "jat_block_forward": (C.c_int, [_VP, _I32, _VP, _VP, _VP, _I32, _I32, _VP, _SZ, _VP]),
    "jat_attn_forward": (C.c_int, [_VP, _I32, _VP, _VP, _I32, _I32, _VP, _SZ, _VP]),
    "jat_time_embed": (C.c_int, [_VP, _VP, _VP, _I32, _VP, _SZ, _VP]),
    "jat_sampler_create": (C.c_int, [_VP, _I32, _I32, _I32, _F32, C.POINTER(_VP)]),
    "jat_solver_plan": (C.c_int, [_VP, _I32, _I32, _VP, _I32, _VP, _VP, _VP]),
    "jat_sampler_create_ex": (C.c_int, [_VP, _I32, _I32, _VP, _I32, _I32, _F32, C.POINTER(_VP)]),
    "jat_sampler_destroy": (None, [_VP]),
    "jat_sampler_run": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _VP]),
    "jat_sampler_info": (C.c_int, [_VP, _VP, _VP, _VP]),
    "jat_sampler_tail_fused": (C.c_int, [_VP]),
    "jat_sampler_set_lengths": (C.c_int, [_VP, C.POINTER(_I32), _I32, _VP]),
    "jat_cfg_euler_step": (C.c_int, [_VP, _VP, _F32, _F32, _F32, _I32, _I32, _I32, _VP]),
    "jat_cfg_stage_step": (C.c_int, [_VP, _VP, _VP, _F32, _F32, _F32, _F32, _F32, _I32, _I32, _I32, _I32, _VP]),
    "jat_channel_affine": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _VP]),
    "jat_crossfade_pair": (C.c_int, [_VP, _I32, _VP, _I32, _I32, _VP, _I32, _VP]),
    "jat_k_norm_modulate": (C.c_int, [_VP, _VP, _VP, _VP, _I64, _VP, _I32, _I32, _I32, _I32, _VP]),
    "jat_k_gemm": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _VP, _I64, _I32, _I32, _VP]),
    "jat_k_gemm_fold": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _VP, _I64, _I32, _VP, _VP, _VP, _VP, _I32, _I32, _VP]),
    "jat_k_gemm_cfg_euler": (C.c_int, [_VP, _VP, _VP, _I32, _I32, _I32, _I32, _VP, _I32, _VP, _VP, _VP, _VP, _F32, _F32, _F32, _I32, _I32, _VP]),
    "jat_k_gemm_cfg_stage": (C.c_int, [_VP, _VP, _VP, _I32, _I32, _I32, _I32, _VP, _I32, _VP, _VP, _VP, _VP, _VP, _F32, _F32, _F32, _F32,
                                       _F32, _I32, _I32, _I32, _VP]),
    "jat_k_gemm_splitk": (C.c_int, [_VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _VP]),
    "jat_k_gemm_wave_n": (C.c_int, [_I32]),
    "jat_k_gemm_plan": (C.c_int, [_VP, _I32, _I32, _I32, _I32, _I32, _VP, _VP]),
    "jat_k_qkv_attn": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _VP, _VP, _I32, _VP]),
    "jat_k_weight_grad": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _VP, _SZ, _VP]),
    "jat_k_weight_grad_ex": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _VP, _SZ, _I32, _VP]),
    "jat_k_weight_grad_plan": (C.c_int, [_I32, _I32, _I32, _VP, _VP]),
    "jat_k_attention": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _VP]),
    "jat_k_attention_lens": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _VP]),
    "jat_k_attention_route": (C.c_int, [_I32, _I32, _I32, _I32, _VP, _VP, _VP]),
    "jat_k_recon_loss": (C.c_int, [_VP, _VP, _VP, _VP, _I64, C.c_double, _F32, _VP, _SZ, _VP]),
    "jat_k_cast_bf16": (C.c_int, [_VP, _VP, _I64, _VP]),
    "jat_k_attention_train": (C.c_int, [_VP] * 5 + [_I32] * 5 + [C.c_uint64, _I32, _F32, _VP]),
    "jat_k_attention_bwd": (C.c_int, [_VP] * 9 + [_I32] * 5 + [C.c_uint64, _I32, _F32, _I32, _VP, _SZ, _VP]),
    "jat_k_norm_bwd": (C.c_int, [_VP, _VP, _VP, _VP, _I64, _VP, _I32, _VP, _VP, _I64, _VP] + [_I32] * 4 + [_VP, _SZ, _VP]),
    "jat_k_gate_bwd": (C.c_int, [_VP, _VP, _VP, _I64, _VP, _VP, _I64] + [_I32] * 3 + [C.c_uint64, _I32, _F32, _I32, _F32] +
                       [_VP, _SZ, _VP]),
    "jat_k_resid_gate": (C.c_int, [_VP, _VP, _VP, _I64, _VP] + [_I32] * 3 + [C.c_uint64, _I32, _F32, _I32, _F32, _VP]),
    "jat_k_gelu": (C.c_int, [_VP, _VP, _I64, C.c_uint64, _I32, _F32, _VP]),
    "jat_k_gelu_bwd": (C.c_int, [_VP, _VP, _I64, C.c_uint64, _I32, _F32, _VP]),
    "jat_k_adamw": (C.c_int, [_VP, _VP, _VP, _VP, _I64] + [_F32] * 7 + [_I32, _VP, _VP, _SZ, _VP]),
    "jat_k_adamw_ema": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _I64] + [_F32] * 8 + [_I32, _VP, _VP, _SZ, _VP]),
    "jat_k_small_dw": (C.c_int, [_VP, _I64, _VP, _I64, _VP, _VP] + [_I32] * 4 + [_VP]),
    "jat_k_small_dx": (C.c_int, [_VP, _I64, _VP, _I32, _VP] + [_I32] * 4 + [_VP, _VP, _SZ, _VP]),
    "jat_k_latent_loss": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _I32, _I32] + [C.c_double] * 7 + [_F32, _VP, _SZ, _VP]),
    "jat_k_latent_loss_ex": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _I32, _I32] + [C.c_double] * 9 + [_F32, _VP, _SZ, _VP]),
    "jat_k_latent_loss_plan": (C.c_int, [_I32, _VP, _VP, _VP, _VP]),
    "jat_trainer_create": (C.c_int, [_VP, C.POINTER(JatTensorRef), _I32, _VP, _VP, _VP, _VP, _I64, _I32, _I32, _VP,
                                     C.POINTER(_VP)]),
    "jat_trainer_destroy": (None, [_VP]),
    "jat_trainer_workspace_bytes": (C.c_int, [_VP, C.POINTER(_SZ)]),
    "jat_trainer_repack": (C.c_int, [_VP, _VP]),
    "jat_trainer_prepare": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _F32, _I32, _VP, _VP, _VP, _VP]),
    "jat_trainer_set_grad_hook": (C.c_int, [_VP, _VP, _VP]),
    "jat_trainer_set_regularisers": (C.c_int, [_VP, C.POINTER(_F32), C.POINTER(_F32)]),
    "jat_trainer_set_latent_loss": (C.c_int, [_VP] + [C.c_double] * 7),
    "jat_trainer_set_charbonnier": (C.c_int, [_VP, C.c_double]),
    "jat_trainer_set_loss_ex": (C.c_int, [_VP] + [C.c_double] * 9),
    "jat_trainer_loss_terms": (C.c_int, [_VP, _VP, _VP]),
    "jat_trainer_fwd_bwd": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _F32, C.c_uint64, _VP, _VP, _VP]),
    "jat_trainer_fwd_bwd_ex": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _F32, C.c_uint64, _VP, _VP, _I32, _VP]),
    "jat_trainer_optim": (C.c_int, [_VP, _F32, _F32, _F32, _F32, _F32, _F32, _F32, _I32, _VP, _VP]),
    "jat_trainer_set_ema": (C.c_int, [_VP, _VP, _F32]),
    "jat_trainer_swap_ema": (C.c_int, [_VP, _VP]),
    "jat_prof_gemm_site": (C.c_int, [_VP, _I32, _I32]),
    "jat_prof_collect": (C.c_int, [_VP, C.POINTER(C.c_double), C.POINTER(_I32), C.POINTER(C.c_double), C.POINTER(_I32)]),
    "jat_dac_decoder_create": (C.c_int, [C.c_void_p, C.POINTER(JatTensorRef), _I32, _I32, _I32, _VP, C.POINTER(_VP)]),
    "jat_dac_decoder_destroy": (None, [_VP]),
    "jat_dac_workspace_bytes": (C.c_int, [_VP, C.POINTER(_SZ)]),
    "jat_dac_decode": (C.c_int, [_VP, _VP, _VP, _I32, _I32, _I32, _VP]),
    "jat_dac_pack_weight": (C.c_int, [_I32, _VP, _I32, _I32, _I32, _VP]),
    "jat_k_dac_split": (C.c_int, [_VP, _VP, _VP, _I64, _VP]),
    "jat_k_dac_conv": (C.c_int, [_VP] * 10 + [_I32] * 8 + [_VP]),
    "jat_k_dac_tail": (C.c_int, [_VP] * 5 + [_I32] * 3 + [_VP]),
    "jat_dac_encoder_create": (C.c_int, [C.c_void_p, C.POINTER(JatTensorRef), _I32, _I32, _I32, _VP, C.POINTER(_VP)]),
    "jat_dac_encoder_destroy": (None, [_VP]),
    "jat_dac_encoder_workspace_bytes": (C.c_int, [_VP, C.POINTER(_SZ)]),
    "jat_dac_encode": (C.c_int, [_VP] * 6 + [_I32] * 4 + [_VP]),
    "jat_k_dac_head": (C.c_int, [_VP] * 7 + [_I32] * 3 + [_VP]),
    "jat_k_dac_rvq": (C.c_int, [_VP] * 10 + [_I32] * 4 + [_VP]),
    "jat_resample_table": (C.c_int, [_I32, _I32, _I32, C.c_double, _VP] + [C.POINTER(_I32)] * 4),
    "jat_resampler_create": (C.c_int, [_I32, _I32, _I32, C.c_double, _VP, C.POINTER(_VP)]),
    "jat_resampler_destroy": (None, [_VP]),
    "jat_resample_out_length": (C.c_int, [_VP, _I64, C.POINTER(_I64)]),
    "jat_resample": (C.c_int, [_VP, _VP, _VP, _I32, _I64, _VP]),
    "jat_k_resample_geometry": (C.c_int, [_I32, _I32, _I32, C.c_double, _I64] + [C.POINTER(_I32)] * 10),
    "jat_channel_stats": (C.c_int, [_VP, _I32, _I32, _I32, _VP, _VP, _VP, _SZ, _VP]),
    "jat_mel_filterbank": (C.c_int, [_I32, _I32, _I32, _VP]),
    "jat_stft_frames": (C.c_int, [_I64, _I32, C.POINTER(_I64)]),
    "jat_audio_metrics_create": (C.c_int, [_I32, _I32, _I32, _I32, _VP, C.POINTER(_VP)]),
    "jat_audio_metrics_destroy": (None, [_VP]),
    "jat_audio_metrics_workspace_bytes": (C.c_int, [_VP, _I32, _I64, C.POINTER(_SZ)]),
    "jat_audio_metrics_run": (C.c_int, [_VP, _VP, _VP, _I32, _I64, _I32, _VP, _VP, _VP, _VP, _VP, _SZ, _VP]),
    "jat_stft": (C.c_int, [_VP, _VP, _VP, _I32, _I64, _VP, _VP, _VP]),
    "jat_istft_workspace_bytes": (C.c_int, [_I32, _I32, _I32, _I64, C.POINTER(_SZ)]),
    "jat_istft": (C.c_int, [_VP, _VP, _I32, _I64, _VP, _VP, _SZ, _VP]),
    "jat_ltas": (C.c_int, [_VP, _VP, _I32, _I64, _VP, _VP, _SZ, _VP]),
    "jat_band_gain": (C.c_int, [_I32, _I32, C.c_double, C.c_double, _VP]),
    "jat_band_splice_workspace_bytes": (C.c_int, [_I32, _I32, _I32, _I64, _I64, C.POINTER(_SZ)]),
    "jat_band_splice": (C.c_int, [_VP, _VP, _VP, _I32, _I64, _I64, _VP, _VP, _VP, _SZ, _VP]),
    "jat_latent_gather": (C.c_int, [_VP] * 10 + [_I32] * 3 + [_VP]),
    "jat_train_monitor": (C.c_int, [_VP, _VP, _VP, _I64, _VP, _VP, _SZ, _VP]),
    "jat_bank_create": (C.c_int, [_I32, _I32, _I32, C.POINTER(_VP)]),
    "jat_bank_destroy": (None, [_VP]),
    "jat_bank_size": (C.c_int, [_VP, C.POINTER(_I32)]),
    "jat_bank_clear": (C.c_int, [_VP]),
    "jat_bank_add": (C.c_int, [_VP, _VP, _VP, _I32, _I64, _I64, _I64, _I32, _VP, _VP, _VP, _VP, _VP]),
    "jat_bank_rows": (C.c_int, [_VP, _I32, C.POINTER(_VP), C.POINTER(_VP)]),
    "jat_bank_load_rows": (C.c_int, [_VP, _VP, _VP, _I32, _VP]),
    "jat_bank_search_workspace_bytes": (C.c_int, [_VP, _I64, C.POINTER(_SZ)]),
    "jat_bank_search": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _VP, _VP, _VP, _SZ, _VP]),
    "jat_bank_blend": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _F32, _VP, _I32, _I32, _VP]),
    "jat_bank_topk_workspace_bytes": (C.c_int, [_VP, _I64, _I32, C.POINTER(_SZ)]),
    "jat_bank_search_topk": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _VP, _VP, _VP, _SZ, _VP]),
    "jat_bank_blend_topk": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _VP, _VP, _F32, _F32, _VP, _I32, _I32, _VP]),
    "jat_yin_periods": (C.c_int, [_I32, C.c_double, C.c_double, _I32, C.POINTER(_I32), C.POINTER(_I32)]),
    "jat_yin": (C.c_int, [C.POINTER(JatYinParams), _VP, _I32, _I64] + [_VP] * 7),
    "jat_f0_compare": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, C.c_double, _VP, _VP]),
    "jat_pyin_beta_probs": (C.c_int, [C.c_double, C.c_double, _I32, _VP]),
    "jat_pyin_create": (C.c_int, [C.POINTER(JatPyinParams), C.POINTER(_VP)]),
    "jat_pyin_destroy": (None, [_VP]),
    "jat_pyin_shape": (C.c_int, [_VP] + [C.POINTER(_I32)] * 4),
    "jat_pyin_tables": (C.c_int, [_VP] * 6),
    "jat_pyin_workspace_bytes": (C.c_int, [_VP, _I32, _I64, C.POINTER(_SZ)]),
    "jat_pyin_track": (C.c_int, [_VP, _VP, _I32, _I64] + [_VP] * 10 + [_SZ, _VP]),
    "jat_pyin_decode": (C.c_int, [_VP, _VP, _I32, _I32, _VP, _VP, _VP, _VP, _SZ, _VP]),
    "jat_pyin_set_profile": (C.c_int, [_VP, _I32]),
    "jat_pyin_profile": (C.c_int, [_VP, _VP]),
}
# name -> (restype, argtypes); every symbol include/jat_hip_ms.h declares (multi-scale retrieval), bound after SIGNATURES
MS_SIGNATURES = {
    "jat_bank_add_pooled": (C.c_int, [_VP, _VP, _VP, _I32, _I64, _I64, _I64, _I32, _I32, _VP, _VP, _VP, _VP, _VP]),
    "jat_bank_pool_frames": (C.c_int, [_VP, _VP, _VP, _I32, _I32, _I32, _I32, C.POINTER(_I32), C.POINTER(_VP), _VP]),
    "jat_bank_mix_scales": (C.c_int, [_VP, _I32, C.POINTER(_I32), C.POINTER(_VP), C.POINTER(_F32), _F32, _VP, _I32, _I32, _I32,
                                      _VP]),
}
# name -> (restype, argtypes); every symbol include/jat_hip_harm.h declares (harmonic analysis, template, comparison)
HARM_SIGNATURES = {
    "jat_harmonic_analyze": (C.c_int, [_VP, _I32, _I64, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _VP, _VP, _VP]),
    "jat_harmonic_synth_workspace_bytes": (C.c_int, [_I32, _I64, _I32, C.POINTER(_SZ)]),
    "jat_harmonic_synth": (C.c_int, [_VP, _VP, _VP, _I32, _I32, _I32, _I64, _I32, _I32, _VP, _VP, _VP, _SZ, _VP]),
    "jat_harmonic_compare": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, C.c_double, C.c_double, _VP, _VP]),
}
# name -> (restype, argtypes); every symbol include/jat_hip_km.h declares (k-means compaction of a retrieval bank)
KM_SIGNATURES = {
    "jat_bank_assign_workspace_bytes": (C.c_int, [_VP, _VP, _I64, C.POINTER(_SZ)]),
    "jat_bank_assign": (C.c_int, [_VP, _I64, _I64, _VP, _VP, _VP, _VP, _VP, _SZ, _VP]),
    "jat_bank_cluster_update_workspace_bytes": (C.c_int, [_VP, _I32, C.POINTER(_SZ)]),
    "jat_bank_cluster_update": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _SZ, _VP]),
    "jat_bank_sum_dist2": (C.c_int, [_VP, _I64, _VP, _VP]),
}
# name -> (restype, argtypes); every symbol include/jat_hip_ivf.h declares (IVF index over a retrieval bank)
IVF_SIGNATURES = {
    "jat_bank_group_workspace_bytes": (C.c_int, [_VP, _I32, C.POINTER(_SZ)]),
    "jat_bank_group": (C.c_int, [_VP, _VP, _I32, _VP, _VP, _VP, _VP, _SZ, _VP]),
    "jat_ivf_search_workspace_bytes": (C.c_int, [_VP, _VP, _I64, _I32, _I32, C.POINTER(_SZ)]),
    "jat_ivf_search": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _VP, _VP, _VP, _VP, _SZ, _VP]),
}
# name -> (restype, argtypes); every symbol include/jat_hip_rate.h declares (voicing-aware index rates)
RATE_SIGNATURES = {
    "jat_f0_classes": (C.c_int, [_VP, _VP, _I32, _I32, _I32, _F32, _I32, _VP, _VP, _VP, _VP]),
    "jat_rate_track": (C.c_int, [_VP, _I32, _I32, _I32, C.POINTER(_F32), _I32, _VP, _VP]),
    "jat_rate_mix": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _VP]),
}
# name -> (restype, argtypes); every symbol include/jat_hip_iir.h declares (IIR low-pass cascades: sosfilt, sosfiltfilt)
IIR_SIGNATURES = {
    "jat_iir_create": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), _I32, _VP, C.POINTER(_VP)]),
    "jat_iir_destroy": (None, [_VP]),
    "jat_iir_geometry": (C.c_int, [C.POINTER(_I32), C.POINTER(_I32)]),
    "jat_iir_padlen": (C.c_int, [_VP, C.POINTER(_I32)]),
    "jat_iir_workspace_bytes": (C.c_int, [_I32, _I64, C.POINTER(_SZ)]),
    "jat_iir_sosfilt": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I64, _VP, _SZ, _VP]),
    "jat_iir_sosfiltfilt": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I64, _VP, _SZ, _VP]),
}
RATE_MAX_HALF_WINDOW = 32    # JAT_RATE_MAX_HALF_WINDOW
RATE_MAX_SMOOTH = 16         # JAT_RATE_MAX_SMOOTH
IVF_MAX_NPROBE = 8           # JAT_IVF_MAX_NPROBE
IVF_MAX_ROWS = 1 << 22       # JAT_IVF_MAX_ROWS
KM_MAX_POOL = 1 << 22        # JAT_KM_MAX_POOL
HARM_MAX = 128               # JAT_HARM_MAX
BANK_MAX_SCALES = 4          # JAT_BANK_MAX_SCALES
BANK_SCALES = (1, 2, 4, 8)   # what a scale may be
MONITOR_WORK_BYTES = 49152   # JAT_MONITOR_WORK_BYTES
LTAS_SLICES = 64             # JAT_LTAS_SLICES
BANK_SLAB = 4096             # JAT_BANK_SLAB
BANK_KEYS, BANK_VALUES = 0, 1
BANK_MAX_K = 8               # JAT_BANK_MAX_K

GRAD_HOOK = C.CFUNCTYPE(None, C.c_int64, C.c_int64, C.c_void_p)   # jat_trainer_set_grad_hook callback

_lib = None


class JatError(RuntimeError):
    pass


def lib():
    """Load libjat_hip.so (once).  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise JatError(f"{LIB_PATH} not found: build it first (`python -c 'import __graft_entry__ as g; "
                           f"g.build()'` or `make -C {os.path.dirname(LIB_PATH)}`); there is no CPU fallback")
        # torch first: it brings its own copy of the HIP runtime, and a process that loaded the system's copy through this library
        # before it finds no device at the first kernel launch ("no ROCm-capable device is detected")
        import torch  # noqa: F401
        h = C.CDLL(LIB_PATH)
        for name, (res, args) in list(SIGNATURES.items()) + list(MS_SIGNATURES.items()) + list(HARM_SIGNATURES.items()) + \
                list(KM_SIGNATURES.items()) + list(IVF_SIGNATURES.items()) + list(RATE_SIGNATURES.items()) + \
                list(IIR_SIGNATURES.items()):
            if not hasattr(h, name) and os.environ.get("JAT_LIB_ALLOW_MISSING"):
                continue      # A/B against an OLDER build through JAT_LIB_PATH (tools/sampler_ab.py): it lacks the newest entry points
            fn = getattr(h, name)
            fn.restype = res
            fn.argtypes = args
        _lib = h
    return _lib


def operand_dtype() -> str:
    """'bf16' or 'fp16': what the loaded library rounds GEMM / attention operands to."""
    return "fp16" if lib().jat_operand_dtype() == 1 else "bf16"


def check(rc: int):
    """Translate a C-ABI return code into the exception the reference would raise at that point."""
    if rc == JAT_OK:
        return
    msg = lib().jat_last_error().decode("utf-8", "replace")
    if rc == JAT_E_SEQLEN:
        raise ValueError(msg)              # jat_audiosr_v3.py:451-452
    if rc == JAT_E_INVALID:
        raise ValueError(msg)
    raise JatError(f"libjat_hip error {rc}: {msg}")


def require_gpu():
    import torch
    if not torch.cuda.is_available():
        raise JatError("jatsr_amd needs an AMD GPU (gfx950): torch.cuda.is_available() is False and there is "
                       "no CPU fallback on the product path")


def stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
