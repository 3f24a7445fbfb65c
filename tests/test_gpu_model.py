"""Model-level parity on the GPU: the HIP path behind the reference's module API vs the CPU oracle and the
committed reference-generated goldens.

Tolerances (measured on the reference itself): the reference's own bf16-autocast forward
deviates from its fp32 forward by rel-L2 0.9-1.3e-2 (max-abs 0.024-0.049), its 50-step CFG sampler by
1.6e-2.  The HIP path keeps the residual stream, norm statistics, softmax, RoPE and modulation in fp32 and
only rounds GEMM/attention operands to bf16, so it must stay within:
    single forward  rel-L2 <= 2e-2, max-abs <= 0.1
    50-step sampler rel-L2 <= 3e-2
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import jatsr_amd  # noqa: E402
import jatsr_amd._lib as L  # noqa: E402
import jatsr_amd.recipe as recipe  # noqa: E402
from helpers import fwd_inputs, load_golden, rel_l2, sampler_inputs, sub  # noqa: E402
from jatsr_amd.model import DiTBlock_GQA, GroupedQueryAttention, JaT_AudioSR_V2, JaT_AudioSR_V3  # noqa: E402
from oracle import jat_oracle as O  # noqa: E402

FWD_TOL, FWD_MAXABS, SAMPLER_TOL = 2e-2, 0.1, 3e-2
_models = {}


def build(cfg_name, norm="rms", salt=0):
    key = (cfg_name, norm, salt)
    if key not in _models:
        L.require_gpu()
        cfg = recipe.CONFIGS[cfg_name]
        cls = JaT_AudioSR_V3 if norm == "rms" else JaT_AudioSR_V2
        m = cls(**cfg)
        sd = {k: torch.from_numpy(v) for k, v in recipe.make_state_dict(cfg, norm, salt).items()}
        missing, unexpected = m.load_state_dict(sd, strict=False)
        assert not unexpected and all(".rope." in k for k in missing)
        _models.clear()  # keep at most one big model resident
        _models[key] = m.to("cuda").eval()
    return _models[key]


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


@pytest.mark.parametrize("name", ["fwd_micro_T24", "fwd_micro_T22_pad", "fwd_micro_ln_T24", "fwd_tiny_T128",
                                  "fwd_tiny_T516_pad", "fwd_v3mod2_T512", "fwd_v3mod2_T1378"])
def test_forward_vs_reference_golden(name):
    z, meta = load_golden(name)
    cfg, x_t, t, x_c = fwd_inputs(meta)
    m = build(meta["cfg"], meta["norm"], meta["salt"])
    out = m(cuda(x_t), cuda(t), cuda(x_c))
    assert out.shape == x_t.shape and out.dtype == torch.float32
    o = out.cpu().numpy()
    assert np.isfinite(o).all()
    o_s = o if meta["full"] else sub(o, *meta["s_out"])
    r = rel_l2(o_s, z["out64"])
    ma = float(np.abs(o_s - z["out64"]).max())
    print(f"{name}: rel-L2 {r:.3e} max-abs {ma:.3e}")
    assert r < FWD_TOL and ma < FWD_MAXABS
    assert abs(np.linalg.norm(o.astype(np.float64)) / float(z["out_l2"]) - 1) < 1e-2


def test_loader_rejects_a_missing_or_missized_tensor_and_the_handle_recovers():
    """jat_model_load_weights on a handle of its own: a missing name and a wrong element count are refused with their code and
    text, before and after a correct load, and the forward through that handle equals the forward of a model that was only ever
    loaded correctly, bit for bit."""
    from jatsr_amd.model import _Handle
    z, meta = load_golden("fwd_micro_T24")
    cfg, x_t, t, x_c = fwd_inputs(meta)
    good = build(meta["cfg"], meta["norm"], meta["salt"])
    want = good(cuda(x_t), cuda(t), cuda(x_c))
    m = type(good)(**cfg)
    m.load_state_dict({k: v.detach().cpu().clone() for k, v in good.state_dict().items()}, strict=False)
    m = m.to("cuda").eval()
    named = m._named_for_pack()
    h = _Handle(*m._handle_cfg())

    def load(tensors, numel={}):
        refs = (L.JatTensorRef * len(tensors))()
        for i, (k, v) in enumerate(tensors.items()):
            refs[i] = L.JatTensorRef(k.encode(), v.data_ptr(), numel.get(k, v.numel()))
        rc = L.lib().jat_model_load_weights(h.ptr, refs, len(tensors), L.stream_ptr())
        return rc, L.lib().jat_last_error().decode()

    def rejections():
        for name in ("final_layer.1.bias", "blocks.1.mlp.0.bias"):
            rc, msg = load({k: v for k, v in named.items() if k != name})
            assert rc == L.JAT_E_STATE and f"missing parameter '{name}'" in msg
        name = "blocks.0.mlp.3.weight"
        n = named[name].numel()
        rc, msg = load(named, {name: n // 2})
        assert rc == L.JAT_E_INVALID and f"parameter '{name}' has {n // 2} elements, expected {n}" in msg

    rejections()                               # nothing loaded yet
    m.__dict__["_jat_handle"] = h              # the model's forward loads `named` into h and runs on it
    assert torch.equal(m(cuda(x_t), cuda(t), cuda(x_c)), want)
    rejections()                               # a refused load leaves the loaded weights as they are
    assert torch.equal(m(cuda(x_t), cuda(t), cuda(x_c)), want)


def test_forward_at_the_benchmarked_batch_vs_reference_golden():
    """BASELINE configs[1] at its full size: the eval forward at B = 28, T = 512 (M = 3584 rows: other tile variants than any
    small test — un-fused QKV GEMM + attn_group_kernel, per-sample adaLN modulation, 57 norm kernels).  Rows 0-1 are the two
    samples of the `fwd_v3mod2_T512` reference golden (JaT_AudioSR_V3.forward in fp64, jat_audiosr_v3.py:422-471), rows 2-27 other
    data with their own t: rows 0-1 must meet the golden's gate, agree with the B = 2 forward to rounding, and must not change
    by a single bit when the OTHER 26 rows are permuted (batch-row independence of every kernel at this shape)."""
    z, meta = load_golden("fwd_v3mod2_T512")
    cfg, x_t, t, x_c = fwd_inputs(meta)
    assert x_t.shape[0] == 2
    m = build(meta["cfg"], meta["norm"], meta["salt"])
    B, C, T = 28, x_t.shape[1], x_t.shape[2]
    xo, co = recipe.make_latents(B - 2, C, T, salt=31)
    to = np.linspace(0.03, 0.97, B - 2).astype(np.float32)
    X, Cn, Tv = np.concatenate([x_t, xo]), np.concatenate([x_c, co]), np.concatenate([t, to])
    out = m(cuda(X), cuda(Tv), cuda(Cn))
    o = out.cpu().numpy()
    assert np.isfinite(o).all()
    r = rel_l2(sub(o[:2], *meta["s_out"]), z["out64"])
    ma = float(np.abs(sub(o[:2], *meta["s_out"]) - z["out64"]).max())
    print(f"B=28 forward, rows 0-1 vs reference golden: rel-L2 {r:.3e} max-abs {ma:.3e}")
    assert r < FWD_TOL and ma < FWD_MAXABS
    small = m(cuda(x_t), cuda(t), cuda(x_c)).cpu().numpy()
    assert rel_l2(o[:2], small) < 1e-2                     # other tiles, other bf16 rounding points; the same math
    perm = np.concatenate([[0, 1], 2 + np.random.RandomState(0).permutation(B - 2)])
    out_p = m(cuda(X[perm]), cuda(Tv[perm]), cuda(Cn[perm]))
    assert torch.equal(out_p[:2], out[:2])
    assert torch.equal(out_p[2:], out[torch.from_numpy(perm[2:]).cuda()])


def test_forward_vs_oracle_micro_batch_rows_independent():
    """Same sample at different batch positions / with different neighbours gives the same result."""
    cfg = recipe.CONFIGS["micro"]
    m = build("micro")
    x_t, x_c = recipe.make_latents(3, 32, 40, salt=11)
    t = np.array([0.1, 0.6, 0.9], np.float32)
    full = m(cuda(x_t), cuda(t), cuda(x_c)).cpu().numpy()
    one = m(cuda(x_t[1:2]), cuda(t[1:2]), cuda(x_c[1:2])).cpu().numpy()
    assert np.array_equal(full[1:2], one)
    ref = O.OracleModel(cfg, recipe.make_state_dict(cfg), "rms", np.float64).forward(x_t, t, x_c)
    assert rel_l2(full, ref) < FWD_TOL


def test_fused_qkv_attention_is_bit_identical_to_separate_kernels(monkeypatch):
    """At N = 128 tokens the q/k/v projection + RoPE + attention run as ONE kernel per (sample, KV group) with q, k, v
    kept in LDS.  The K-accumulation order and the softmax arithmetic are the same as in the separate QKV GEMM +
    attention kernels, so the two paths must agree bit for bit."""
    z, meta = load_golden("fwd_v3mod2_T512")
    cfg, x_t, t, x_c = fwd_inputs(meta)
    m = build(meta["cfg"], meta["norm"], meta["salt"])
    h = m._get_handle()                             # switches are per handle (the JAT_* variables only set its defaults at creation)
    h.set_switch("fuse_qkv_attn", 2)                # 2 = force (the default only fuses when B*Hkv fills the GPU)
    fused = m(cuda(x_t), cuda(t), cuda(x_c))
    h.set_switch("fuse_qkv_attn", 0)
    h.set_switch("qkv_split", 0)                    # the un-split QKV GEMM (a batch this small would split K: other summation order)
    separate = m(cuda(x_t), cuda(t), cuda(x_c))
    h.set_switch("qkv_split", 1)
    split = m(cuda(x_t), cuda(t), cuda(x_c))         # the small-batch default: K-slices + splitk_qkv_finish_kernel
    assert rel_l2(split.cpu().numpy(), separate.cpu().numpy()) < 2e-3
    assert rel_l2(sub(split.cpu().numpy(), *meta["s_out"]), z["out64"]) < FWD_TOL
    if L.operand_dtype() == "bf16":
        assert torch.equal(fused, separate)
    else:
        # fp16 build (tests/test_gpu_fp16.py): both paths are run-to-run deterministic and equally close to the reference
        # (5.4e-4), but a few query rows per block differ by one fp16 rounding (an fp32 intermediate that differs in its last
        # bit between the two epilogues flips 1 in 4096 roundings at 11 bits, 1 in 65536 at bf16's 8): closeness, not identity
        assert rel_l2(fused.cpu().numpy(), separate.cpu().numpy()) < 2e-3
    assert rel_l2(sub(fused.cpu().numpy(), *meta["s_out"]), z["out64"]) < FWD_TOL


def test_split_k_finish_fused_with_the_following_norm(monkeypatch):
    """Small batches run out_proj / fc2 as K-slices; the pass that sums the slices and updates the residual stream also
    normalises + modulates the row for the next consumer (norm2, the next block's norm1, the final norm) in the same launch.
    Against the two separate launches (JAT_FUSE_FINISH=0): same arithmetic up to the order of the row's sum of squares - a
    last-bit change of rstd flips isolated bf16 roundings of the normalised rows, which 28 blocks amplify to ~2e-3 (the bf16
    forward itself sits 4e-3 from the fp64 reference); both forms must meet the reference gate."""
    z, meta = load_golden("fwd_v3mod2_T512")
    cfg, x_t, t, x_c = fwd_inputs(meta)
    m = build(meta["cfg"], meta["norm"], meta["salt"])
    fused = m(cuda(x_t), cuda(t), cuda(x_c)).cpu().numpy()
    m._get_handle().set_switch("fuse_finish", 0)
    separate = m(cuda(x_t), cuda(t), cuda(x_c)).cpu().numpy()
    assert rel_l2(fused, separate) < 3e-3
    assert rel_l2(sub(fused, *meta["s_out"]), z["out64"]) < FWD_TOL
    assert rel_l2(sub(separate, *meta["s_out"]), z["out64"]) < FWD_TOL


def test_time_embed_vs_oracle():
    cfg = recipe.CONFIGS["micro"]
    m = build("micro")
    t = np.array([0.0, 0.02, 0.5, 0.98, 1.0], np.float32)
    got = m.time_embed(cuda(t)).cpu().numpy()
    ref = O.OracleModel(cfg, recipe.make_state_dict(cfg), "rms", np.float64).t_embed(t)
    assert rel_l2(got, ref) < 1e-5   # fp32 path end to end


@pytest.mark.parametrize("layer", [0, 1])
def test_block_vs_oracle(layer):
    """DiTBlock_GQA.forward(x, t_emb) through jat_block_forward, addressed as model.blocks[i]."""
    cfg = recipe.CONFIGS["micro"]
    m = build("micro")
    orc = O.OracleModel(cfg, recipe.make_state_dict(cfg), "rms", np.float64)
    x = recipe.gaussian("blk_x", (2, 10, 256), 1)
    temb = recipe.gaussian("blk_t", (2, 256), 2)
    got = m.blocks[layer](cuda(x), cuda(temb)).cpu().numpy()
    ref = orc.block(layer, x.astype(np.float64), temb.astype(np.float64))
    assert rel_l2(got, ref) < 1e-2
    assert rel_l2(got - x, ref - x) < 2e-2   # the update itself, not just the carried residual


def test_attention_module_vs_oracle():
    cfg = recipe.CONFIGS["micro"]
    m = build("micro")
    orc = O.OracleModel(cfg, recipe.make_state_dict(cfg), "rms", np.float64)
    x = recipe.gaussian("attn_x", (2, 37, 256), 3)
    got = m.blocks[1].attn(cuda(x)).cpu().numpy()
    ref = orc.attention(1, x.astype(np.float64))
    assert rel_l2(got, ref) < 1e-2


def test_attention_rope_accuracy_at_max_length():
    """RoPE angles are evaluated in registers (fract(pos*inv_freq/2pi) -> v_sin/v_cos); check the longest allowed
    sequence (N = max_len = 2048, jat_audiosr_v3.py:361), where the fp32 angle is largest, against the fp64 oracle."""
    cfg = recipe.CONFIGS["micro"]
    m = build("micro")
    orc = O.OracleModel(cfg, recipe.make_state_dict(cfg), "rms", np.float64)
    x = recipe.gaussian("attn_long", (1, 2048, 256), 9)
    got = m.blocks[0].attn(cuda(x)).cpu().numpy()
    ref = orc.attention(0, x.astype(np.float64))
    assert rel_l2(got, ref) < 1e-2
    assert rel_l2(got[:, -64:], ref[:, -64:]) < 1e-2     # the last positions carry the largest angles


def test_standalone_block_and_attention():
    """Modules constructed on their own (reference API jat_audiosr_v3.py:117,257) own a private handle."""
    cfg = recipe.CONFIGS["micro"]
    sd = recipe.make_state_dict(cfg)
    orc = O.OracleModel(cfg, sd, "rms", np.float64)
    blk = DiTBlock_GQA(256, 4, 2, 4.0)
    own = {k[len("blocks.1."):]: torch.from_numpy(v) for k, v in sd.items() if k.startswith("blocks.1.")}
    missing, unexpected = blk.load_state_dict(own, strict=False)
    assert not unexpected and all(".rope." in k for k in missing)
    blk = blk.to("cuda").eval()
    x = recipe.gaussian("blk_x", (1, 12, 256), 4)
    temb = recipe.gaussian("blk_t", (1, 256), 5)
    assert rel_l2(blk(cuda(x), cuda(temb)).cpu().numpy(), orc.block(1, x.astype(np.float64), temb.astype(np.float64))) < 1e-2
    att = GroupedQueryAttention(256, 4, 2)
    att.load_state_dict({k[len("blocks.0.attn."):]: torch.from_numpy(v) for k, v in sd.items()
                         if k.startswith("blocks.0.attn.")}, strict=False)
    att = att.to("cuda").eval()
    assert rel_l2(att(cuda(x)).cpu().numpy(), orc.attention(0, x.astype(np.float64))) < 1e-2
    with pytest.raises(AssertionError):
        GroupedQueryAttention(256, 3, 2)          # jat_audiosr_v3.py:119
    with pytest.raises(AssertionError):
        GroupedQueryAttention(256, 4, 3)          # jat_audiosr_v3.py:120


def test_zero_init_outputs_exact_zero():
    """jat_audiosr_v3.py:395-404: adaLN and final linear start at zero => output is exactly 0."""
    m = JaT_AudioSR_V3(**recipe.CONFIGS["micro"]).to("cuda").eval()
    x_t, x_c = recipe.make_latents(2, 32, 24, salt=7)
    out = m(cuda(x_t), cuda(np.array([0.3, 0.7], np.float32)), cuda(x_c))
    assert float(out.abs().max()) == 0.0


def test_sequence_too_long_raises_value_error():
    m = build("micro")
    x = torch.zeros(1, 32, 4 * 2049, device="cuda")
    with pytest.raises(ValueError):
        m(x, torch.zeros(1, device="cuda"), x)
    ok = torch.zeros(1, 32, 4 * 2048, device="cuda")   # N == max_len is allowed
    assert m(ok, torch.zeros(1, device="cuda"), ok).shape == ok.shape


def test_weights_repack_after_update():
    cfg = recipe.CONFIGS["micro"]
    m = JaT_AudioSR_V3(**cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in recipe.make_state_dict(cfg, salt=5).items()}, strict=False)
    m = m.to("cuda").eval()
    x_t, x_c = recipe.make_latents(1, 32, 16, salt=9)
    t = np.array([0.4], np.float32)
    a = m(cuda(x_t), cuda(t), cuda(x_c)).cpu().numpy()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in recipe.make_state_dict(cfg, salt=6).items()}, strict=False)
    b = m(cuda(x_t), cuda(t), cuda(x_c)).cpu().numpy()
    ref = O.OracleModel(cfg, recipe.make_state_dict(cfg, salt=6)).forward(x_t, t, x_c)
    assert rel_l2(b, ref) < FWD_TOL and rel_l2(a, ref) > 0.1


@pytest.mark.parametrize("name", ["sampler_micro_cfg3", "sampler_micro_nocfg", "sampler_tiny_cfg3"])
def test_sampler_vs_reference_golden(name):
    z, meta = load_golden(name)
    cfg, lr, z0 = sampler_inputs(meta)
    m = build(meta["cfg"], "rms", meta["salt"])
    out_g = jatsr_amd.flow_matching_sample(m, cuda(lr), num_steps=meta["steps"], cfg_scale=meta["cfg_scale"],
                                           verbose=False, z0=cuda(z0))
    out_e = jatsr_amd.flow_matching_sample(m, cuda(lr), num_steps=meta["steps"], cfg_scale=meta["cfg_scale"],
                                           verbose=False, z0=cuda(z0), use_graph=False)
    assert torch.equal(out_g, out_e)                     # hipGraph replay == eager replay, bit for bit
    o = out_g.cpu().numpy()
    o_s = o if meta["full"] else sub(o, *meta["s_out"])
    r = rel_l2(o_s, z["z"])
    print(f"{name}: rel-L2 {r:.3e}")
    assert r < SAMPLER_TOL
    # replaying the captured graph with new inputs gives new results, replaying with the old ones the old
    out2 = jatsr_amd.flow_matching_sample(m, cuda(lr) * 0.5, num_steps=meta["steps"], cfg_scale=meta["cfg_scale"],
                                          verbose=False, z0=cuda(z0))
    assert not torch.equal(out2, out_g)
    out3 = jatsr_amd.flow_matching_sample(m, cuda(lr), num_steps=meta["steps"], cfg_scale=meta["cfg_scale"],
                                          verbose=False, z0=cuda(z0))
    assert torch.equal(out3, out_g)


def test_sampler_with_norm_folding_matches_golden(monkeypatch):
    """Norm folding (the sampler's default at large M): RMSNorm weight and adaLN scale folded into per-step copies of the
    consumer weights, rstd applied after the matmul, shift @ W^T tables per step — no norm kernel in the captured graph.
    Must meet the same parity gate as the un-folded path and stay deterministic."""
    monkeypatch.setenv("JAT_FOLD_NORM", "2")    # 2 = also at small M (by default only buckets of > 2304 rows fold)
    z, meta = load_golden("sampler_tiny_cfg3")
    cfg, lr, z0 = sampler_inputs(meta)
    m = JaT_AudioSR_V3(**cfg)                      # fresh module: fresh handle and sampler cache
    m.load_state_dict({k: torch.from_numpy(v) for k, v in recipe.make_state_dict(cfg).items()}, strict=False)
    m = m.to("cuda").eval()
    a = jatsr_amd.flow_matching_sample(m, cuda(lr), num_steps=meta["steps"], cfg_scale=meta["cfg_scale"], verbose=False,
                                       z0=cuda(z0))
    b = jatsr_amd.flow_matching_sample(m, cuda(lr), num_steps=meta["steps"], cfg_scale=meta["cfg_scale"], verbose=False,
                                       z0=cuda(z0), use_graph=False)
    assert torch.equal(a, b)
    assert rel_l2(sub(a.cpu().numpy(), *meta["s_out"]), z["z"]) < SAMPLER_TOL


def test_sampler_over_the_fold_table_cap_falls_back_to_the_norm_kernels():
    """The per-step folded weights cost HBM (0.5 GB per step for v3mod2).  A handle whose "fold_cap_mb" switch is below the
    table's size must build the SAME sampler with the norm kernels instead — within the parity gate of the reference golden,
    deterministic — and leave nothing half-built behind: lifting the cap on the same handle folds again."""
    z, meta = load_golden("sampler_tiny_cfg3")
    cfg, lr, z0 = sampler_inputs(meta)
    m = JaT_AudioSR_V3(**cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in recipe.make_state_dict(cfg).items()}, strict=False)
    m = m.to("cuda").eval()
    h = m._get_handle()
    h.set_switch("fold_norm", 2)                   # fold at this small M too
    h.set_switch("fold_cap_mb", 1)                 # the tiny model's table is ~100x that
    B, T = lr.shape[0], lr.shape[2]
    capped = jatsr_amd.Sampler(m, B, T, meta["steps"], meta["cfg_scale"])
    assert capped.info() == {"folded": False, "fused_attn": capped.info()["fused_attn"], "fold_bytes": 0}
    a = capped.run(cuda(lr), cuda(z0))
    assert torch.equal(a, capped.run(cuda(lr), cuda(z0)))
    assert rel_l2(sub(a.cpu().numpy(), *meta["s_out"]), z["z"]) < SAMPLER_TOL
    h.set_switch("fold_cap_mb", 0)
    folded = jatsr_amd.Sampler(m, B, T, meta["steps"], meta["cfg_scale"])
    assert folded.info()["folded"] and folded.info()["fold_bytes"] > (1 << 20)
    b = folded.run(cuda(lr), cuda(z0))
    assert rel_l2(sub(b.cpu().numpy(), *meta["s_out"]), z["z"]) < SAMPLER_TOL
    assert rel_l2(a.cpu().numpy(), b.cpu().numpy()) < SAMPLER_TOL


def test_sampler_at_benchmarked_shape_vs_reference_golden():
    """BASELINE configs[2] dims: v3mod2 (D = 1280, depth 28, 20Q/4KV), T = 512, CFG = 3.0, against the reference's own
    `flow_matching_sample` (4 Euler steps, fixture generated by oracle/gen_golden.py on the reference classes).
      (a) the B = 2 bucket;
      (b) the B = 28 bucket bench.py times — rows 0-1 are the same two samples, rows 2-27 other data.  At M = 7168 the path
          differs from every small test: fused QKV+RoPE+attention kernel, 224 x 320 / 256 x 160 quadrant-ping-pong tiles,
          split patch embed, per-step folded weights (no norm kernels), one hipGraph.  Rows 0-1 must meet the same gate
          against the reference, agree with the B = 2 bucket to rounding, the graph must equal the eager replay bit for bit,
          and shuffling the OTHER rows must not change rows 0-1 by a single bit (batch-row independence)."""
    z, meta = load_golden("sampler_v3mod2_cfg3_4step")
    cfg, lr, z0 = sampler_inputs(meta)
    m = build(meta["cfg"], "rms", meta["salt"])
    kw = dict(num_steps=meta["steps"], cfg_scale=meta["cfg_scale"], verbose=False)
    out2 = jatsr_amd.flow_matching_sample(m, cuda(lr), z0=cuda(z0), **kw).cpu().numpy()
    r2 = rel_l2(sub(out2, *meta["s_out"]), z["z"])
    C, T = lr.shape[1], lr.shape[2]
    lr28 = np.concatenate([lr, recipe.gaussian("lr_fill", (26, C, T), 7)], 0)
    z28 = np.concatenate([z0, recipe.gaussian("z0_fill", (26, C, T), 8)], 0)
    g28 = jatsr_amd.flow_matching_sample(m, cuda(lr28), z0=cuda(z28), **kw)
    e28 = jatsr_amd.flow_matching_sample(m, cuda(lr28), z0=cuda(z28), use_graph=False, **kw)
    assert torch.equal(g28, e28)
    o28 = g28.cpu().numpy()
    assert np.isfinite(o28).all()
    r28 = rel_l2(sub(o28[:2], *meta["s_out"]), z["z"])
    rb = rel_l2(o28[:2], out2)
    print(f"sampler v3mod2 4-step CFG=3: B=2 bucket rel-L2 {r2:.3e}, B=28 bucket rows 0-1 rel-L2 {r28:.3e}, "
          f"B=28 vs B=2 {rb:.3e}")
    assert r2 < SAMPLER_TOL and r28 < SAMPLER_TOL and rb < 1e-2
    assert abs(np.linalg.norm(o28[:2].astype(np.float64)) / float(z["z_l2"]) - 1) < 1e-2
    perm = np.concatenate([[0, 1], np.arange(27, 1, -1)])
    p28 = jatsr_amd.flow_matching_sample(m, cuda(lr28[perm]), z0=cuda(z28[perm]), **kw)
    assert torch.equal(p28[:2], g28[:2])


def test_short_row_in_a_longer_bucket_equals_its_stand_alone_run():
    """`Sampler.run(lengths=...)`: a row with fewer valid frames than the bucket's T (zero-padded; its padded keys masked in
    attention, its padded frames read as zeros by the patchify kernel at every step) must reproduce the stand-alone sampling
    of that row — including T_i % 4 != 0, where the reference re-pads the state with zeros at every step
    (jat_audiosr_v3.py:435-439) — and leave the full-length rows bit-identical to a run without lengths."""
    m = build("micro")
    Cc, T = 32, 92                     # 23 tokens
    for short in (50, 37, 4):          # 50 = 12.5 tokens (ragged), 37 (ragged), 4 (a single token)
        lr = recipe.gaussian("len_lr", (3, Cc, T), short)
        z0 = recipe.gaussian("len_z0", (3, Cc, T), short + 100)
        lr[1, :, short:] = 0
        z0[1, :, short:] = 0
        kw = dict(num_steps=6, cfg_scale=2.5, verbose=False)
        both = jatsr_amd.flow_matching_sample(m, cuda(lr), z0=cuda(z0), lengths=[T, short, T], **kw)
        alone = jatsr_amd.flow_matching_sample(m, cuda(lr[1:2, :, :short]), z0=cuda(z0[1:2, :, :short]), **kw)
        full = jatsr_amd.flow_matching_sample(m, cuda(lr[[0, 2]]), z0=cuda(z0[[0, 2]]), **kw)
        assert rel_l2(both[1:2, :, :short].cpu().numpy(), alone.cpu().numpy()) < 2e-5
        assert torch.equal(both[[0, 2]], full)
    with pytest.raises(ValueError):
        jatsr_amd.flow_matching_sample(m, cuda(lr), z0=cuda(z0), lengths=[T, T + 1, T], **kw)


# (T, short): buckets beyond one 64-key block.  T = 400: 100 tokens, attn_group_kernel with lens[b] != N — 260 = 65 tokens, 257 =
# 65 tokens with a ragged last patch, 130 = 33 tokens (its stand-alone run is one block of the streaming kernel), 4 = one token.
# T = 520: 130 tokens, attn_fwd_kernel<1, 64> with three key blocks — 510 = 128 tokens (ends in the second block, leaves the third
# out; alone it is the group kernel), 260 / 257 = 65 tokens (end in the second block).
# None of these ids holds a word of the fp16 child's `-k` for this file (tests/fp16_matrix.py: forward_vs_reference,
# sampler_vs_reference, benchmarked, fused): they run on the bf16 library only, as the 23-token test above does; the fp16 library
# runs `lens` in tests/test_gpu_kernels.py::test_attention_lens_* and in the side-stream case, whose files it runs whole.
def _attn_route(ntok):
    """(group, qt, kvb) of the attention launch of a sampler bucket of ntok tokens per sample (`jat_k_attention_route`)"""
    import ctypes as C
    g, qt, kvb = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    L.check(L.lib().jat_k_attention_route(ntok, (ntok + 63) // 64 * 64, 0, 0, C.byref(g), C.byref(qt), C.byref(kvb)))
    return (g.value, qt.value, kvb.value)


LONG_BUCKET_ROWS = [(400, 260), (400, 257), (400, 130), (400, 4), (520, 510), (520, 260), (520, 257)]
_full_rows = {}


@pytest.mark.parametrize("T,short", LONG_BUCKET_ROWS)
def test_short_row_in_a_bucket_of_several_key_blocks_equals_its_stand_alone_run(T, short):
    """test_short_row_in_a_longer_bucket_equals_its_stand_alone_run where the short row changes which keys of a LATER block are
    masked (streaming kernel) or masks inside the group kernel: same pattern, same gates — the short row against its stand-alone
    run at 2e-5, the full-length rows `torch.equal` to a run without lengths."""
    m = build("micro")
    Cc = 32
    lr = recipe.gaussian("len_lr", (3, Cc, T), T)
    z0 = recipe.gaussian("len_z0", (3, Cc, T), T + 100)
    kw = dict(num_steps=6, cfg_scale=2.5, verbose=False)
    if T not in _full_rows:
        _full_rows[T] = jatsr_amd.flow_matching_sample(m, cuda(lr[[0, 2]]), z0=cuda(z0[[0, 2]]), **kw)
    lr[1, :, short:] = 0
    z0[1, :, short:] = 0
    both = jatsr_amd.flow_matching_sample(m, cuda(lr), z0=cuda(z0), lengths=[T, short, T], **kw)
    alone = jatsr_amd.flow_matching_sample(m, cuda(lr[1:2, :, :short]), z0=cuda(z0[1:2, :, :short]), **kw)
    got = both[1:2, :, :short].cpu().numpy()
    r = rel_l2(got, alone.cpu().numpy())
    here, there = _attn_route((T + 3) // 4), _attn_route((short + 3) // 4)
    print(f"T = {T} {here}, short row of {short} frames {there} against its stand-alone run: rel-L2 {r:.3e}")
    assert torch.isfinite(both).all()
    if here[0] == 0 and (T + 3) // 4 > here[2] and there[0] == 1:
        # The bucket streams its keys in blocks (attn_fwd_kernel: online softmax, the running output rescaled block by block) and the
        # row alone, at most 128 tokens, is attn_group_kernel (one softmax over all keys): two orders of the same fp32 sums, so
        # that P and the output round differently here and there and the two runs part by the operand rounding, not by 2e-5 —
        # measured 5.3e-3 for all three rows, and 0 with JAT_ATTN_GROUP=0, where the row alone streams the same blocks (DESIGN.md
        # section 2).  tests/test_gpu_kernels.py::test_attention_lens_* hold attention itself to the bit; here both runs are held
        # to the fp64 oracle's stand-alone sample under SAMPLER_TOL, and the row in the bucket to the error of the row alone times
        # 1.5, the factor tests/twin_check.py allows between two roundings of one computation.
        cfg = recipe.CONFIGS["micro"]
        ref = O.flow_matching_sample(O.OracleModel(cfg, recipe.make_state_dict(cfg), "rms", np.float64), lr[1:2, :, :short],
                                     z0[1:2, :, :short], 6, 2.5)
        e_both, e_alone = rel_l2(got, ref), rel_l2(alone.cpu().numpy(), ref)
        print(f"    against the fp64 oracle's stand-alone sample: in the bucket {e_both:.3e}, alone {e_alone:.3e}")
        assert e_both < SAMPLER_TOL and e_alone < SAMPLER_TOL
        assert e_both <= 1.5 * e_alone
    else:
        assert r < 2e-5
    assert torch.equal(both[[0, 2]], _full_rows[T])


def test_sample_long_pads_the_short_tail_into_the_main_bucket():
    """Default `sample_long`: the file's shorter last chunk rides in the same launch as the full-length chunks (one bucket);
    same result as one launch per chunk length (`pad_short_chunks=False`) and as the chunk-by-chunk loop."""
    m = build("micro")
    Cc, total, chunk, ov = 32, 100, 40, 8
    lr = cuda(recipe.gaussian("long_lr", (Cc, total), 1) * 2 + 0.3)
    mean = cuda(recipe.gaussian("mean", (Cc,), 2) * 0.1)
    std = cuda(np.abs(recipe.gaussian("std", (Cc,), 3)) + 0.5)
    plan = jatsr_amd.chunk_plan(total, chunk, ov)
    noise = [cuda(recipe.gaussian("noise", (1, Cc, b - a), i)) for i, (a, b) in enumerate(plan)]
    kw = dict(num_steps=4, cfg_scale=2.0, chunk_frames=chunk, overlap_frames=ov, noise=noise)
    merged = jatsr_amd.sample_long(m, lr, mean, std, mean, std, **kw)
    split = jatsr_amd.sample_long(m, lr, mean, std, mean, std, pad_short_chunks=False, **kw)
    assert merged.shape == split.shape == (1, Cc, total)
    assert rel_l2(merged.cpu().numpy(), split.cpu().numpy()) < 2e-5


def test_sample_long_at_v3mod2_dims_batched_equals_chunk_by_chunk():
    """BASELINE configs[4] dims: one file of T = 4096 latent frames, v3mod2 model, reference chunk plan (3 x 1378 + 478
    frames, overlap 172; infer_test_v3m2.py:340-404).  `sample_long` batches the equal-length chunks into one sampler
    launch; the reference samples them one at a time (B = 1, :370-398).  Same inputs, same noise: the two must agree to
    rounding (different GEMM tile choices at M = 2070 vs 690 rows), and the file's crossfade must equal the oracle's."""
    m = build("v3mod2")
    Cc, total = 1024, 4096
    lr = cuda(recipe.gaussian("long_lr", (Cc, total), 1) * 1.5 + 0.2)
    mean = cuda(recipe.gaussian("mean", (Cc,), 2) * 0.1)
    std = cuda(np.abs(recipe.gaussian("std", (Cc,), 3)) + 0.5)
    plan = jatsr_amd.chunk_plan(total)
    assert [b - a for a, b in plan] == [1378, 1378, 1378, 478] and plan == O.chunk_plan(total)
    noise = [cuda(recipe.gaussian("noise", (1, Cc, b - a), i)) for i, (a, b) in enumerate(plan)]
    got = jatsr_amd.sample_long(m, lr, mean, std, mean, std, num_steps=3, cfg_scale=3.0, noise=noise)
    outs = []
    for i, (a, b) in enumerate(plan):
        c = (lr[None, :, a:b] - mean.view(1, -1, 1)) / std.view(1, -1, 1)
        g = jatsr_amd.flow_matching_sample(m, c, num_steps=3, cfg_scale=3.0, verbose=False, z0=noise[i])
        outs.append((g * std.view(1, -1, 1) + mean.view(1, -1, 1)).cpu().numpy())
    ref = O.crossfade_chunks(outs, 172)
    g = got.cpu().numpy()
    assert g.shape == (1, Cc, total) and np.isfinite(g).all()
    r = rel_l2(g, ref)
    print(f"sample_long v3mod2 T=4096: batched vs chunk-by-chunk rel-L2 {r:.3e}")
    assert r < 1e-2
    # the short last chunk (478 frames) rides in the same launch as the three full chunks, zero-padded and key-masked
    # (`sample_long(pad_short_chunks=True)`): its un-faded tail must match the stand-alone B = 1 run of 478 frames
    tail = rel_l2(g[:, :, 3618 + 172:], outs[3][:, :, 172:])
    print(f"short tail chunk, padded into the 1378-frame bucket vs stand-alone: rel-L2 {tail:.3e}")
    assert tail < 1e-2
    # and with one launch per chunk length it is the very same bucket as the stand-alone run: equal up to the
    # de-normalisation's rounding (fused multiply-add in jat_channel_affine vs torch's mul + add)
    split = jatsr_amd.sample_long(m, lr, mean, std, mean, std, num_steps=3, cfg_scale=3.0, noise=noise,
                                  pad_short_chunks=False).cpu().numpy()
    assert np.allclose(split[:, :, 3618 + 172:], outs[3][:, :, 172:], rtol=0, atol=4e-6)


def test_graph_replay_is_deterministic():
    """Race screen: the captured 50-step graph replayed 25 times on the same inputs must give bit-identical
    results (a memset node inside the captured chain used to race with its neighbours on short kernels: the
    V^T padding is now cleared once at sampler creation, outside the graph)."""
    m = build("tiny")
    lr = cuda(recipe.gaussian("lr_latent", (1, 1024, 64), 200))
    z0 = cuda(recipe.gaussian("z0", (1, 1024, 64), 201))
    ref = jatsr_amd.flow_matching_sample(m, lr, num_steps=50, cfg_scale=3.0, verbose=False, z0=z0, use_graph=False)
    bad = sum(int(not torch.equal(jatsr_amd.flow_matching_sample(m, lr, num_steps=50, cfg_scale=3.0, verbose=False,
                                                                 z0=z0), ref)) for _ in range(25))
    assert bad == 0


def test_sampler_one_step_matches_forward_plus_euler():
    """One sampler step == model forward on the CFG double batch + jat_cfg_euler_step (infer_test_v3m2.py:154-179)."""
    m = build("micro")
    B, Cc, T = 2, 32, 20
    lr = cuda(recipe.gaussian("lr_latent", (B, Cc, T), 300))
    z0 = cuda(recipe.gaussian("z0", (B, Cc, T), 301))
    got = jatsr_amd.flow_matching_sample(m, lr, num_steps=1, cfg_scale=3.0, verbose=False, z0=z0)
    tb = torch.zeros(2 * B, device="cuda")
    both = m(torch.cat([z0, z0]), tb, torch.cat([lr, torch.zeros_like(lr)]))
    x = both[B:] + 3.0 * (both[:B] - both[B:])
    ref = z0 + (x - z0) / (1 - 0.0 + 1e-5) * 1.0
    # same kernels on both sides at this size (norm folding only engages for buckets of more than 2304 rows, or when forced):
    # the gate only allows for the sampler's split patch embed (cond part computed once in fp32) vs the forward's single GEMM
    assert rel_l2(got.cpu().numpy(), ref.cpu().numpy()) < 1e-2


def test_crossfade_and_chunk_plan():
    z, _ = load_golden("misc")
    chunks = [cuda(recipe.gaussian("chunk", (1, 6, n), i)) for i, n in enumerate((40, 40, 23))]
    assert np.allclose(jatsr_amd.crossfade_chunks(chunks, 8).cpu().numpy(), z["xfade_ov8"], atol=1e-6)
    assert np.array_equal(jatsr_amd.crossfade_chunks(chunks, 0).cpu().numpy(), z["xfade_ov0"])
    assert np.array_equal(jatsr_amd.crossfade_chunks(chunks[:1], 8).cpu().numpy(), z["xfade_single"])
    assert jatsr_amd.crossfade_chunks([], 8) is None
    assert jatsr_amd.chunk_plan(4096) == O.chunk_plan(4096)


def test_sample_long_batches_equal_chunks():
    """Chunked long-sequence inference (infer_test_v3m2.py:340-404) with equal-length chunks batched:
    same result as sampling the chunks one at a time and crossfading with the oracle's crossfade."""
    m = build("micro")
    Cc, total, chunk, ov = 32, 100, 40, 8
    lr = cuda(recipe.gaussian("long_lr", (Cc, total), 1) * 2 + 0.3)
    mean = cuda(recipe.gaussian("mean", (Cc,), 2) * 0.1)
    std = cuda(np.abs(recipe.gaussian("std", (Cc,), 3)) + 0.5)
    plan = jatsr_amd.chunk_plan(total, chunk, ov)
    assert plan == [(0, 40), (32, 72), (64, 100)]
    noise = [cuda(recipe.gaussian("noise", (1, Cc, b - a), i)) for i, (a, b) in enumerate(plan)]
    got = jatsr_amd.sample_long(m, lr, mean, std, mean, std, num_steps=4, cfg_scale=2.0, chunk_frames=chunk,
                                overlap_frames=ov, noise=noise)
    outs = []
    for i, (a, b) in enumerate(plan):
        c = (lr[None, :, a:b] - mean.view(1, -1, 1)) / std.view(1, -1, 1)
        g = jatsr_amd.flow_matching_sample(m, c, num_steps=4, cfg_scale=2.0, verbose=False, z0=noise[i])
        outs.append((g * std.view(1, -1, 1) + mean.view(1, -1, 1)).cpu().numpy())
    ref = O.crossfade_chunks(outs, ov)
    assert got.shape == (1, Cc, total)
    assert rel_l2(got.cpu().numpy(), ref) < 1e-5
