"""tests/forward_ref.py against the oracle, and its own rounding floor (CPU only).

With rnd = identity every function of the twin must BE the fp64 oracle (`oracle.jat_oracle.OracleModel`, itself pinned to the
reference's goldens by tests/test_oracle_golden.py): 1e-12, measured 4e-16 ... 1.4e-15.  With the operand rounding, the block
update's error against the exact twin — the floor E0 the GPU tests gate the kernels on — must be reproducible and sit where
the number format puts it, so that the twin cannot silently lose (or gain) a rounding point.
"""
import math

import numpy as np
import pytest
import torch

import jatsr_amd.recipe as recipe
from oracle import jat_oracle as O

import forward_ref as R
from width_cases import FORWARD_CONFIGS

EXACT = 1e-12
CFGS = {"micro": recipe.CONFIGS["micro"], "v3mod2_depth1": dict(recipe.CONFIGS["v3mod2"], depth=1)}
_cache = {}


def setup(name):
    if name not in _cache:
        cfg = CFGS[name]
        sd = recipe.make_state_dict(cfg)
        _cache[name] = (cfg, sd, O.OracleModel(cfg, sd, "rms", np.float64))
    return _cache[name]


@pytest.mark.parametrize("name", list(CFGS))
@pytest.mark.parametrize("fold", [False, True])
def test_exact_twin_is_the_oracle(name, fold):
    """patch embed, time MLP, adaLN, every block, attention, final norm + linear + unpatchify, the whole forward (T % 4 != 0
    included): rnd = identity against the fp64 oracle, un-folded and in the folded sampler's arrangement of the same maths
    (one t for the batch, as in a sampler step)."""
    cfg, sd, orc = setup(name)
    tw = R.Twin(cfg, sd, fold=fold)
    C, D = cfg["input_channels"], cfg["hidden_size"]
    for T in (24, 22):
        x_t, x_c = recipe.make_latents(2, C, T, salt=3)
        t = np.array([0.3, 0.3] if fold else [0.2, 0.7], np.float32)
        ref = orc.forward(x_t, t, x_c, record=True)
        st = {}
        got = tw.forward(x_t, t, x_c, stages=st)
        assert got.shape == ref.shape and R.rel_l2(got, ref) < EXACT
        for k, v in st.items():
            assert R.rel_l2(v, orc.stages[k]) < EXACT, k
        last = R.t64(orc.stages[f"block{cfg['depth'] - 1}"])
        assert R.rel_l2(tw.final(last, T), ref) < EXACT
    x = recipe.gaussian("blk_x", (1 if fold else 3, 10, D), 1).astype(np.float64)
    temb = recipe.gaussian("blk_t", (1 if fold else 3, D), 2).astype(np.float64)
    for i in range(cfg["depth"]):
        assert R.rel_l2(tw.adaln(i, R.t64(temb)), orc.adaln(i, temb)) < EXACT
        assert R.rel_l2(tw.block(i, R.t64(x), R.t64(temb)), orc.block(i, x, temb)) < EXACT


@pytest.mark.parametrize("norm", ["rms", "ln"])
@pytest.mark.parametrize("name", list(FORWARD_CONFIGS))
def test_exact_twin_is_the_oracle_at_the_other_widths(name, norm):
    """The reference the GPU gates of tests/test_gpu_widths.py rest on, at the hidden sizes, Q / KV ratios (3, 8, 1, 4), MLP ratios
    (4, 3, 2.5, 2) and channel counts (input != cond in one case) of tests/width_cases.py, for RMSNorm (V3) and LayerNorm (V2):
    every stage of the forward, the time MLP, adaLN and each block on their own, ragged T; the folded arrangement (RMSNorm
    only) and two CFG sampler steps where the model can be sampled (cond_channels == input_channels)."""
    cfg = FORWARD_CONFIGS[name]
    sd = recipe.make_state_dict(cfg, norm)
    orc = O.OracleModel(cfg, sd, norm, np.float64)
    Cin, Cc, D = cfg["input_channels"], cfg["cond_channels"], cfg["hidden_size"]
    x_t, x_c = recipe.gaussian("x_t", (3, Cin, 70), 7), recipe.gaussian("x_cond", (3, Cc, 70), 7)
    for fold in ([False, True] if norm == "rms" else [False]):
        tw = R.Twin(cfg, sd, norm=norm, fold=fold)
        t = np.array([0.3, 0.3, 0.3] if fold else [0.2, 0.55, 0.9], np.float32)
        ref = orc.forward(x_t, t, x_c, record=True)
        st = {}
        got = tw.forward(x_t, t, x_c, stages=st)
        assert got.shape == ref.shape == x_t.shape and R.rel_l2(got, ref) < EXACT
        for k, v in st.items():
            assert R.rel_l2(v, orc.stages[k]) < EXACT, k
        if Cin == Cc:
            lr, z0 = recipe.gaussian("lr_latent", (2, Cin, 22), 210), recipe.gaussian("z0", (2, Cin, 22), 211)
            assert R.rel_l2(tw.sample(lr, z0, 2, 3.0), O.flow_matching_sample(orc, lr, z0, num_steps=2, cfg_scale=3.0)) < EXACT
    tw = R.Twin(cfg, sd, norm=norm)
    tt = np.array([0.0, 0.02, 0.5, 0.98, 1.0], np.float32)
    assert R.rel_l2(tw.t_embed(R.t64(tt)), orc.t_embed(tt)) < EXACT
    x = recipe.gaussian("blk_x", (3, 10, D), 1).astype(np.float64)
    temb = recipe.gaussian("blk_t", (3, D), 2).astype(np.float64)
    for i in range(cfg["depth"]):
        assert R.rel_l2(tw.adaln(i, R.t64(temb)), orc.adaln(i, temb)) < EXACT
        assert R.rel_l2(tw.block(i, R.t64(x), R.t64(temb)), orc.block(i, x, temb)) < EXACT


@pytest.mark.parametrize("name", list(CFGS))
def test_fused_attention_of_one_kv_group_is_the_oracles_attention(name):
    """`qkv_attention_group` on every KV group's rows of Wq / Wk / Wv, concatenated and sent through out_proj, is
    GroupedQueryAttention.forward; with a row scale and biases it is the same function of the scaled, shifted projections."""
    cfg, sd, orc = setup(name)
    D, Hq, Hkv = cfg["hidden_size"], cfg["num_q_heads"], cfg["num_kv_heads"]
    g = Hq // Hkv * 64
    x = R.t64(recipe.gaussian("attn_x", (2, 37, D), 3))
    wq, wk, wv, wo = (R.t64(sd[f"blocks.0.attn.{n}_proj.weight"]) for n in ("q", "k", "v", "out"))
    groups = [R.qkv_attention_group(x, wq[kv * g:(kv + 1) * g], wk[kv * 64:(kv + 1) * 64], wv[kv * 64:(kv + 1) * 64], R.identity,
                                    inv_freq=R.rope_inv_freq()) for kv in range(Hkv)]
    assert R.rel_l2(torch.cat(groups, -1) @ wo.T, orc.attention(0, x.numpy())) < EXACT
    # rstd applied after the matmul + a bias == the projection of the scaled row with a bias
    rs = 0.5 + R.t64(recipe.gaussian("attn_rs", (2, 37, 1), 4)).abs()
    bq, bk, bv = (R.t64(recipe.gaussian("attn_b" + n, (m,), 5)) * 0.1 for n, m in (("q", g), ("k", 64), ("v", 64)))
    a = R.qkv_attention_group(x, wq[:g], wk[:64], wv[:64], R.identity, bq=bq, bk=bk, bv=bv, row_scale=rs)
    b = R.attention_group((x * rs) @ wq[:g].T + bq, (x * rs) @ wk[:64].T + bk, (x * rs) @ wv[:64].T + bv, R.identity)
    assert R.rel_l2(a, b) < EXACT


def test_attention_reference_with_key_lengths_is_the_plain_reference_on_the_valid_tokens():
    """`attention_heads(lens=...)`, the reference of tests/test_gpu_kernels.py::test_attention_lens_*: for every sample the rows
    < lens[b] equal the plain reference evaluated on that sample's first lens[b] tokens alone, whatever the keys beyond hold
    (here: K scaled by 8 and V = 100, as the GPU tests poison them); all-full lens and lens above N equal the plain reference;
    the rows past lens[b] are finite and are the softmax over the valid keys of their own queries; lens[b] = 1 gives V's row 0 in
    every query row.  The plain reference itself is pinned against a direct evaluation of single heads."""
    B, N, Hq, Hkv = 4, 23, 6, 2
    lens = [23, 13, 1, 22]
    q, k, v = (R.t64(recipe.gaussian("lens_" + n, (B * N, h * 64), 9)) * s for n, h, s in (("q", Hq, 1.5), ("k", Hkv, 1.5), ("v", Hkv, 1.0)))
    plain = R.attention_heads(q, k, v, B, N, Hq, Hkv)
    # the plain reference itself, head by head
    for b, h in ((0, 0), (3, 5), (1, 2)):
        rows = slice(b * N, (b + 1) * N)
        kv = h // (Hq // Hkv)
        s = q[rows, h * 64:(h + 1) * 64] @ k[rows, kv * 64:(kv + 1) * 64].T / 8.0
        assert R.rel_l2(plain[rows, h * 64:(h + 1) * 64], torch.softmax(s, -1) @ v[rows, kv * 64:(kv + 1) * 64]) < EXACT
    kp, vp = k.clone().view(B, N, -1), v.clone().view(B, N, -1)
    for b, n in enumerate(lens):
        kp[b, n:] *= 8
        vp[b, n:] = 100.0
    kp, vp = kp.view(B * N, -1), vp.view(B * N, -1)
    got = R.attention_heads(q, kp, vp, B, N, Hq, Hkv, lens=lens)
    assert bool(torch.isfinite(got).all())
    for b, n in enumerate(lens):
        rows = slice(b * N, b * N + n)
        alone = R.attention_heads(q[rows], k[rows], v[rows], 1, n, Hq, Hkv)
        assert R.rel_l2(got[rows], alone) < EXACT, b
        # a row past lens[b]: its own query over the valid keys
        if n < N:
            h, kv, r = 4, 4 // (Hq // Hkv), b * N + N - 1
            s = q[r, h * 64:(h + 1) * 64] @ k[rows, kv * 64:(kv + 1) * 64].T / 8.0
            assert R.rel_l2(got[r, h * 64:(h + 1) * 64], torch.softmax(s, -1) @ v[rows, kv * 64:(kv + 1) * 64]) < EXACT
    assert torch.equal(got[2 * N:3 * N], v.view(B, N, Hkv, 64)[2, 0].repeat_interleave(Hq // Hkv, 0).reshape(1, -1).expand(N, -1))
    # the poison is seen without the mask
    assert R.rel_l2(R.attention_heads(q, kp, vp, B, N, Hq, Hkv), plain) > 1.0
    for full in ([N] * B, [N + 7] * B, torch.tensor([N, N + 1, N, 2 * N])):
        assert torch.equal(R.attention_heads(q, k, v, B, N, Hq, Hkv, lens=full), plain)


def test_cfg_euler_step_and_sampler_are_the_oracles():
    cfg, sd, orc = setup("micro")
    C = cfg["input_channels"]
    xp = recipe.gaussian("xp", (4, C, 22), 1).astype(np.float64)
    z = recipe.gaussian("z", (2, C, 22), 2).astype(np.float64)
    for t, dt in ((np.float32(0.3), np.float32(0.02)), (np.float32(0.9995), np.float32(0.0005))):
        assert R.rel_l2(R.cfg_euler_step(R.t64(xp), R.t64(z), 3.0, t, dt), O.cfg_euler_step(xp, z, 3.0, t, dt)) < EXACT
    assert np.array_equal(R.linspace_f32(0.0, 1.0, 51), O.linspace_f32(0.0, 1.0, 51))
    lr = recipe.gaussian("lr_latent", (2, C, 22), 200)
    z0 = recipe.gaussian("z0", (2, C, 22), 201)
    ref = O.flow_matching_sample(orc, lr, z0, num_steps=3, cfg_scale=3.0)
    for fold in (False, True):
        assert R.rel_l2(R.Twin(cfg, sd, fold=fold).sample(lr, z0, 3, 3.0), ref) < EXACT
    assert R.rel_l2(R.Twin(cfg, sd).sample(lr, z0, 2, 1.0), O.flow_matching_sample(orc, lr, z0, num_steps=2, cfg_scale=1.0)) < EXACT


# relative rms of one rounding to p significant bits is at most 2^-p / sqrt(3); bf16 keeps 8 bits, fp16 11
_ULP_RMS = {torch.bfloat16: 2.0 ** -9 / math.sqrt(3.0), torch.float16: 2.0 ** -12 / math.sqrt(3.0)}


@pytest.mark.parametrize("dtype,lo,hi", [(torch.bfloat16, 2.5e-3, 4e-3), (torch.float16, 2.5e-3 / 8, 4e-3 / 8)])
def test_block_update_floor_at_full_width(dtype, lo, hi):
    """E0 = rel_l2(twin(rnd) - x, twin(id) - x) of one block at D = 1280 (recipe weights, x scaled like a residual stream, a time
    embedding per sample from the time MLP).

      - with the modulation vectors given exactly, so that only the block's own rounding points act (weights, normalised rows,
        q / k / v, probabilities, attention output, GELU output): inside [2.5e-3, 4e-3] for bf16 — measured 3.29e-3 ... 3.33e-3 —
        and 8x lower for fp16 (three more bits; 4.11e-4 ... 4.13e-4);
      - through adaLN as the block entry point runs it (silu(t_emb) and the adaLN weight are GEMM operands: rounded): above
        that, by no more than the rounding of three modulation vectors per half (shift, scale, gate), each the sum of
        products of two rounded operands: sqrt(3) * sqrt(2) * 2^-p / sqrt(3) added in quadrature.  Measured 3.93e-3 ...
        4.00e-3 (bf16), 4.9e-4 ... 5.0e-4 (fp16);
      - reproducible: the same call gives the same bits; and the same within 5 % at another shape (one sample of 112 rows
        against two of 128: the adaLN part of a single sample is one draw of 6 x 1280 modulation errors, about 1 % of spread)."""
    cfg = dict(recipe.CONFIGS["v3mod2"], depth=1)
    sd = recipe.make_state_dict(cfg)
    exact, rounded = R.Twin(cfg, sd), R.Twin(cfg, sd, R.make_rnd(dtype))
    seen = []
    for B, N in ((2, 128), (1, 112)):
        x = R.t64(recipe.gaussian("floor_x", (B, N, 1280), N)) * 0.7
        temb = exact.t_embed(torch.linspace(0.1, 0.9, B, dtype=R.F64))
        ref = exact.block(0, x, temb)
        inner = R.rel_l2(rounded.block(0, x, mod=exact.adaln(0, temb)) - x, ref - x)
        got = rounded.block(0, x, temb)
        full = R.rel_l2(got - x, ref - x)
        print(f"{dtype} B={B} N={N}: E0 {inner:.3e} (exact modulation), {full:.3e} (through adaLN)")
        assert lo <= inner <= hi
        assert inner < full <= math.sqrt(inner ** 2 + 6 * _ULP_RMS[dtype] ** 2)
        assert torch.equal(got, rounded.block(0, x, temb))
        seen.append((inner, full))
    assert abs(seen[0][0] / seen[1][0] - 1) < 0.05 and abs(seen[0][1] / seen[1][1] - 1) < 0.05
