"""Model configurations at the hidden sizes `jat_model_create` accepts but no `recipe.CONFIGS` entry has — test infrastructure,
shared by tests/test_forward_ref_cpu.py (the fp64 twin against the oracle) and tests/test_gpu_widths.py (the kernels against the
twin and the numpy training oracle).  They stay out of `recipe.CONFIGS`, which fixtures and the benchmark key on.

All are depth 2, patch_len 4, 32 channels (a CPU oracle evaluates them in under a second); together they cover
    D / 256 = 3, 4, 6, 8           norm_modulate_kernel, linear_f32_kernel<3, 4, 6, 8>, splitk_resid_norm_block_kernel at
                                   192 / 256 / 384 / 512 threads
    Q / KV = 3, 8, 1, 4            the head-pair loop of attn_group_kernel at an odd and three even group sizes, hk = h / G
    mlp_ratio 4, 3, 2.5, 2         MLP widths 3072, 3072, 3840, 4096
    bottleneck 128, 256
"""

WIDTH_CONFIGS = {
    "w768": dict(input_channels=32, cond_channels=32, patch_len=4, hidden_size=768, depth=2, num_q_heads=12, num_kv_heads=4,
                 bottleneck_dim=128, mlp_ratio=4.0),
    "w1024": dict(input_channels=32, cond_channels=32, patch_len=4, hidden_size=1024, depth=2, num_q_heads=16, num_kv_heads=2,
                  bottleneck_dim=256, mlp_ratio=3.0),
    "w1536": dict(input_channels=32, cond_channels=32, patch_len=4, hidden_size=1536, depth=2, num_q_heads=24, num_kv_heads=24,
                  bottleneck_dim=128, mlp_ratio=2.5),
    "w2048": dict(input_channels=32, cond_channels=32, patch_len=4, hidden_size=2048, depth=2, num_q_heads=32, num_kv_heads=8,
                  bottleneck_dim=128, mlp_ratio=2.0),
}
WIDTHS = list(WIDTH_CONFIGS)

# forward only: the sampler and the trainer condition on a latent of the sampled shape and reject cond_channels != input_channels
W1536_CIN64 = dict(WIDTH_CONFIGS["w1536"], input_channels=64, cond_channels=32)
FORWARD_CONFIGS = dict(WIDTH_CONFIGS, w1536_cin64=W1536_CIN64)
