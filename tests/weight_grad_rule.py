"""The weight-gradient launch rule of csrc/gemm_tn.hip (`gemm_tn_tile`, `gemm_tn_ksplit`; reported by `jat_k_weight_grad_plan`)
and the weight shapes a model hands to it (csrc/jat_train.cpp `dw_shapes`), restated in Python.  Shared by
tests/test_weight_grad_plan_cpu.py and tests/test_gpu_grad_accum.py."""


def tn_path(out, inn, tokens):
    """(tile, K slices) a weight gradient [out, in] over `tokens` rows takes."""
    nkt = (tokens + 63) // 64
    big = out % 256 == 0 and inn % 256 == 0 and out * inn >= 1024 * 1024
    tiles = (out // 256) * (inn // 256) if big else (out // 128) * (inn // 128)
    s = min((256 if big else 512) // tiles, nkt // 8)
    return (256 if big else 128), max(1, min(s, 16))


def dw_shapes(hidden_size, num_kv_heads, bottleneck_dim, mlp_hidden, input_channels, cond_channels, patch_len=4, head_dim=64):
    """[out, in] of the seven weights whose gradient is a GEMM over all tokens: final Linear, MLP fc2 / fc1, out_proj, fused QKV,
    patch-embed proj.2 / proj.0."""
    D = hidden_size
    return [(patch_len * input_channels, D), (D, mlp_hidden), (mlp_hidden, D), (D, D), (D + 2 * num_kv_heads * head_dim, D),
            (D, bottleneck_dim), (bottleneck_dim, patch_len * (input_channels + cond_channels))]
