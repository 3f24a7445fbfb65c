"""Every launch path of the forward at full layer width (D = 1280, 20Q / 4KV, MLP 5120) against fp64, at rounding-floor tightness.

csrc/gemm_plan.cpp gives one DiT block very different launches depending on M = B * tokens: tile variants, K slices and their
finishing passes (`splitk_qkv_finish`, `splitk_resid_finish`, `splitk_resid_norm`, `splitk_gelu_finish`), the fused QKV +
attention kernel, the folded sampler's producer / consumer epilogues.  They are reached here through the entry points that
exist — `model.blocks[l](x, t_emb)` (jat_block_forward), `jat_forward` on a one- and a two-layer model, the sampler,
`jat_k_gemm_fold` — at one M per (variant, K-slices) pair the recorded plans (tests/golden/gemm_plan.json) hold.

Which finishing pass runs where.  jat_block_forward has no norm after the block, so in the block sweep a split-K out_proj
finishes through `splitk_resid_norm` (norm2 rides in it) and a split-K fc2 always through `splitk_resid_finish`.  fc2 ->
`splitk_resid_norm` only exists inside a whole forward: with the final norm (no modulation) in the one-layer forwards, with
the next block's modulated norm1 in the two-layer forwards of `test_two_layer_forward_small_m_vs_fp64` and the B = 2 sampler.

Reference and gate.  tests/forward_ref.py restates the forward in torch fp64 with the HIP path's rounding points; it is
evaluated in fp64 on the device.  `exact` = the twin with rnd = identity (the oracle, tests/test_forward_ref_cpu.py),
`rounded` = the twin rounding to the library's operand dtype.  E0 = error(rounded vs exact) on the same inputs is a property
of the reference alone (bf16: 3.9e-3 ... 4.0e-3 of a block's update, 4.1e-3 of a one-layer forward's output, 5.3e-3 of the
two-step sampled latent).  A correct kernel rounds at the twin's points and differs only in fp32 accumulation order and
isolated last-bit flips, so its error has E0's statistics:

    error(kernel vs exact) <= F * E0,  F = 1.5, one F for every shape of every section

for the whole tensor, for every sample's rows alone (a path that is wrong for the last, ragged sample must not hide in the
norm of the rest), and for the max-abs error.  Measured on MI355X, bf16 build (error / E0, worst sample, max-abs ratio):
block sweep 1.000 / 1.002 / 0.90 ... 1.09; one-layer forward 1.000 ... 1.001 / 1.003 / 0.91 ... 1.03; sampler 0.996 ... 1.000 /
1.010 / 0.98 ... 1.08.  Nothing had to be added to the twin beyond the listed points and F stayed at its start.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import jatsr_amd  # noqa: E402
import jatsr_amd._lib as L  # noqa: E402
import jatsr_amd.recipe as recipe  # noqa: E402
from jatsr_amd.model import JaT_AudioSR_V3  # noqa: E402

import forward_ref as R  # noqa: E402
from twin_check import check  # noqa: E402

OP = torch.float16 if L.OPERAND_DTYPE == "fp16" else torch.bfloat16
D = 1280
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_state = {}


def setup(depth):
    """One model of v3mod2's layer dimensions at `depth` with recipe weights, and its two twins on the device; at most one
    depth resident."""
    if _state.get("depth") != depth:
        L.require_gpu()
        _state.clear()
        cfg = dict(recipe.CONFIGS["v3mod2"], depth=depth)
        sd = recipe.make_state_dict(cfg)
        m = JaT_AudioSR_V3(**cfg)
        missing, unexpected = m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
        assert not unexpected and all(".rope." in k for k in missing)
        _state.update(depth=depth, cfg=cfg, sd=sd, model=m.to("cuda").eval(), twins={})
    return _state


def twin(depth, rounded, fold=False):
    st = setup(depth)
    key = (rounded, fold)
    if key not in st["twins"]:
        st["twins"][key] = R.Twin(st["cfg"], st["sd"], R.make_rnd(OP if rounded else None), fold=fold, device="cuda")
    return st["twins"][key]


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


# ---- 2. the block sweep ---------------------------------------------------------------------------------------------------
# (B, tokens): one M = B * tokens per distinct (variant, K slices) pair of the recorded plans, per site
BLOCK_SHAPES = [(1, 345), (4, 112), (2, 345), (1, 1000), (4, 345), (12, 128), (14, 112), (14, 128), (18, 128), (8, 345),
                (28, 112), (28, 128), (34, 112), (4, 1125), (42, 128), (56, 128), (28, 256), (28, 345), (112, 128)]
SMALL = (1, 345)          # also run with "qkv_split" 0 and with "fuse_finish" 0
SITES = {"qkv": (0, 0), "out_proj": (1, 1), "fc1": (2, 2), "fc2": (3, 3)}     # name -> (site id, index into NK of the golden)
# Pairs whose one-launch form launch_gemm redirects when the forward is not folded: variant 39 (the k-step-pair kernel) takes
# only the split-residual producer epilogues and the K slices; the plain gated-residual and the GELU epilogue go to its
# fallback, the 256 x 160 tile 32, whose row it carries.  The rule is launch_gemm's (gemm.hip): 39 runs its own kernel only if
# gemm_kpair_eligible (epilogue F32 / RESID AND the fold planes fold_out, fold_lo, fold_part are set, M % 224 == 0, no K
# slices) or gemm_kpair_part_eligible (K slices of an un-folded GEMM); everything else goes to `fallback` = 32.  An un-folded
# forward never sets the fold planes.  The sweep still runs these shapes (M = 7168: out_proj, fc2; M = 1792: fc1), i.e. tile
# 32 under both epilogues, and fc1 runs 32 by plan at M = 1568 / 3808; the producer form of 39 itself runs in the folded
# sampler test and in test_folded_producers_keep_both_planes below.
REDIRECTED = {("out_proj", (39, 1)): 32, ("fc2", (39, 1)): 32, ("fc1", (39, 1)): 32}


def _plan(handle, site, M, N, K, folding=0):
    v, k = C.c_int32(), C.c_int32()
    L.check(L.lib().jat_k_gemm_plan(handle.ptr, site, M, N, K, folding, C.byref(v), C.byref(k)))
    return (v.value, k.value)


def test_block_sweep_reaches_every_recorded_plan_pair():
    """Coverage is asserted, not assumed: the union over BLOCK_SHAPES of what `jat_k_gemm_plan` gives the model under test
    must hold every (variant, K slices) pair tests/golden/gemm_plan.json records for v3mod2 (default switches, un-folded), per
    site.  jat_block_forward carves its workspace by M exactly as jat_k_gemm_plan assumes (split-K partials up to M = 4096),
    so each pair is launched as planned; REDIRECTED names the pairs launch_gemm hands to another tile, and why."""
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "gemm_plan.json")))
    h = setup(2)["model"]._get_handle()
    counts = {}
    for name, (site, i) in SITES.items():
        N, K = gold["NK"]["v3mod2"][i]
        want = {tuple(p) for p in gold["plans"]["v3mod2"]["default"][site][0][i]}
        got = {_plan(h, site, B * n, N, K) for B, n in BLOCK_SHAPES}
        assert want <= got, (name, sorted(want - got))
        counts[name] = len(want)
        for (nm, pair), to in REDIRECTED.items():
            if nm == name:
                assert pair in want and pair[0] == 39 and pair[1] == 1 and L.lib().jat_k_gemm_wave_n(to) > 0
    assert counts == {"qkv": 6, "out_proj": 13, "fc1": 10, "fc2": 15}
    # The fused QKV + attention kernel: run_block takes it for ntok == 128 and B * Hkv >= 192 if the handle holds a fresh
    # group-major weight copy (L.wqkv_g && !group_copy_stale) — the condition jat_sampler_create evaluates for a bucket of the
    # same handle and reports through jat_sampler_info.  In the bf16 build the fused and the planned path agree bit for bit
    # (tests/test_gpu_model.py), so the outputs cannot tell which one ran: ask the library.
    fused_shapes = [s for s in BLOCK_SHAPES if s[1] == 128 and s[0] * 4 >= 192]
    assert fused_shapes == [(56, 128), (112, 128)]
    m = setup(2)["model"]
    h.set_switch("fold_norm", 0)                 # no folded-weight table for this probe
    try:
        for B, n in fused_shapes + [(42, 128)]:  # CFG doubles the batch: a bucket of B / 2 samples runs B rows of 128 tokens
            info = jatsr_amd.Sampler(m, B // 2, 4 * n, 1, 3.0).info()
            assert info["fused_attn"] == (B * 4 >= 192) and not info["folded"], (B, info)
        h.set_switch("fuse_qkv_attn", 0)
        assert not jatsr_amd.Sampler(m, 28, 512, 1, 3.0).info()["fused_attn"]
    finally:
        h.set_switch("fuse_qkv_attn", 1)
        h.set_switch("fold_norm", 1)


def _block_inputs(B, n, idx):
    x = cuda(recipe.gaussian("paths_x", (B, n, D), idx) * np.float32(0.7))          # scaled like a residual stream
    t = torch.linspace(0.03, 0.97, B, dtype=R.F64, device="cuda") if B > 1 else torch.tensor([0.4], dtype=R.F64, device="cuda")
    t_emb = twin(2, False).t_embed(t).float()                                       # every sample its own time embedding
    return x, t_emb


@pytest.mark.parametrize("B,n", BLOCK_SHAPES)
def test_block_paths_vs_fp64(B, n):
    """`model.blocks[l](x, t_emb)` of the depth-2 model against the twin at one shape of the sweep, under the default switches;
    the 128-token shapes with B >= 48 also with "fuse_qkv_attn" 0 (the planned QKV GEMM instead of the fused kernel), the small
    shape also with "qkv_split" 0 and with "fuse_finish" 0.  Per run: finite, update error <= 1.5 E0 (whole, per sample,
    max-abs), and a second run bit-identical.
    Measured (MI355X, bf16): error / E0 1.000 at every shape and switch setting (3.91e-3 ... 4.00e-3 against 3.91e-3 ...
    4.00e-3), worst single sample 1.002, max-abs 0.90 ... 1.09."""
    idx = BLOCK_SHAPES.index((B, n))
    layer = idx % 2
    st = setup(2)
    m, h = st["model"], st["model"]._get_handle()
    x, t_emb = _block_inputs(B, n, idx)
    x64, te64 = x.double(), t_emb.double()
    ref64 = twin(2, False).block(layer, x64, te64)
    ref_r = twin(2, True).block(layer, x64, te64)
    runs = [("default", {})]
    if n == 128 and B >= 48:
        runs.append(("fuse_qkv_attn=0", {"fuse_qkv_attn": 0}))
    if (B, n) == SMALL:
        runs += [("qkv_split=0", {"qkv_split": 0}), ("fuse_finish=0", {"fuse_finish": 0})]
        assert _plan(h, 0, B * n, 1792, D)[1] > 1 and _plan(h, 1, B * n, D, D)[1] > 1 and _plan(h, 3, B * n, D, 5120)[1] > 1
    try:
        for name, sw in runs:
            for k, v in sw.items():
                h.set_switch(k, v)
            got = m.blocks[layer](x, t_emb)
            again = m.blocks[layer](x, t_emb)
            for k in sw:
                h.set_switch(k, 1)
            check(f"block {B}x{n} layer {layer} [{name}]", got, x64, ref64, ref_r)
            assert torch.equal(got, again), name
    finally:
        for k in ("fuse_qkv_attn", "qkv_split", "fuse_finish"):
            h.set_switch(k, 1)


# ---- 4. head and tail -------------------------------------------------------------------------------------------------------
# (B, T): M = B * ceil(T / 4) covers plan_patch's 4 / 2 / 1 slices + splitk_gelu_finish, the second patch Linear's and the
# final linear's variants with the unpatchify epilogue, the time path at D = 1280; the last one has T % 4 != 0 (1378 = 4 * 344 + 2)
FORWARD_SHAPES = [(1, 1380), (16, 512), (18, 512), (28, 512), (32, 512), (56, 512), (28, 1380), (3, 1378)]


def test_forward_shapes_reach_the_head_and_tail_plans():
    """plan_patch's 4, 2 and 1 slices and all five recorded variants of the final linear are what FORWARD_SHAPES launch."""
    h = setup(1)["model"]._get_handle()
    Ms = [B * ((T + 3) // 4) for B, T in FORWARD_SHAPES]
    assert {_plan(h, 4, M, 512, 8192)[1] for M in Ms} == {4, 2, 1}
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "gemm_plan.json")))
    i = [tuple(nk) for nk in gold["NK"]["v3mod2"]].index((4096, 1280))
    recorded = {tuple(p) for p in gold["plans"]["v3mod2"]["default"][4][0][i]}
    final = {_plan(h, 4, M, 4096, D) for M in Ms}
    assert len(recorded) == 5 and final == recorded, (sorted(final), sorted(recorded))


@pytest.mark.parametrize("B,T", FORWARD_SHAPES)
def test_one_layer_forward_vs_fp64(B, T):
    """`jat_forward` of the depth-1 model against the twin's forward (patchify, both patch Linears, time MLP, adaLN, the block,
    final norm + linear + unpatchify): the output's error against the exact twin <= 1.5 E0, whole / per sample / max-abs, and a
    second run bit-identical.  No entry point exposes the patch-embed output, so head and tail are gated through the final
    output of a twin that uses the same block.  Measured (MI355X, bf16): error / E0 1.000 ... 1.001 (4.12e-3), worst sample
    1.003, max-abs 0.91 ... 1.03."""
    st = setup(1)
    m = st["model"]
    idx = FORWARD_SHAPES.index((B, T))
    x_t, x_c = (cuda(a) for a in recipe.make_latents(B, 1024, T, salt=40 + idx))
    t = torch.linspace(0.05, 0.95, B, device="cuda") if B > 1 else torch.tensor([0.35], device="cuda")
    ref64 = twin(1, False).forward(x_t, t, x_c)
    ref_r = twin(1, True).forward(x_t, t, x_c)
    got = m(x_t, t, x_c)
    assert got.shape == x_t.shape
    check(f"forward {B}x{T}", got, torch.zeros_like(ref64), ref64, ref_r)
    assert torch.equal(got, m(x_t, t, x_c))


@pytest.mark.parametrize("B,T", [(2, 1378), (4, 512)])
def test_two_layer_forward_small_m_vs_fp64(B, T):
    """Un-folded `jat_forward` of the depth-2 model at small M (690, 512): fc2 of block 0 is cut into K slices and finished by
    `splitk_resid_norm` WITH the modulation of block 1's norm1 (in jat_block_forward fc2 never has a norm to carry; in the
    one-layer forward it carries the un-modulated final norm).  Same gate on the output as the one-layer forwards."""
    st = setup(2)
    m, h = st["model"], st["model"]._get_handle()
    M = B * ((T + 3) // 4)
    assert _plan(h, 3, M, D, 5120)[1] > 1 and _plan(h, 1, M, D, D)[1] > 1
    x_t, x_c = (cuda(a) for a in recipe.make_latents(B, 1024, T, salt=60 + B))
    t = torch.linspace(0.15, 0.85, B, device="cuda")
    ref64 = twin(2, False).forward(x_t, t, x_c)
    ref_r = twin(2, True).forward(x_t, t, x_c)
    got = m(x_t, t, x_c)
    check(f"two-layer forward {B}x{T}", got, torch.zeros_like(ref64), ref64, ref_r)
    assert torch.equal(got, m(x_t, t, x_c))


# ---- 5. the sampler's step ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,folded,fused", [(28, True, True), (14, True, False), (2, False, False)])
def test_two_sampler_steps_vs_fp64(B, folded, fused):
    """`flow_matching_sample` (2 steps, CFG 3, T = 512) on the depth-2 model against the twin's two Euler steps:
      B = 28 (M = 7168): folded norms, the fused QKV + attention kernel, the k-step-pair producer and the persistent tiles;
      B = 14 (M = 3584): folded, planned QKV GEMM + attention kernel;  B = 2 (M = 512): the un-folded small bucket.
    `jat_sampler_info` must report just that.  The twin models the fold's rounding points (fold=True: the rounded residual
    row as A operand, rnd(W diag(w (1 + scale))), rstd after the matmul, rnd(shift) @ rnd(W)^T, hi + lo planes), so the gate
    is the same 1.5 E0 on the sampled latent.  Measured (MI355X, bf16): error / E0 1.000 / 1.000 / 0.996 (5.3e-3), worst sample
    1.010 / 1.004 / 0.999, max-abs 0.98 / 1.03 / 1.08."""
    st = setup(2)
    m = st["model"]
    T = 512
    lr = cuda(recipe.gaussian("paths_lr", (B, 1024, T), 300 + B))
    z0 = cuda(recipe.gaussian("paths_z0", (B, 1024, T), 400 + B))
    got = jatsr_amd.flow_matching_sample(m, lr, num_steps=2, cfg_scale=3.0, verbose=False, z0=z0)
    info = m._jat_samplers[(B, T, 2, 3.0)].info()
    assert (info["folded"], info["fused_attn"]) == (folded, fused), info
    ref64 = twin(2, False, fold=folded).sample(lr, z0, 2, 3.0)
    ref_r = twin(2, True, fold=folded).sample(lr, z0, 2, 3.0)
    check(f"sampler B={B}", got, torch.zeros_like(ref64), ref64, ref_r)
    assert torch.equal(got, jatsr_amd.flow_matching_sample(m, lr, num_steps=2, cfg_scale=3.0, verbose=False, z0=z0))
    m.__dict__.pop("_jat_samplers", None)      # release the bucket's buffers and folded weights


@pytest.mark.parametrize("M", [7168, 3584])
@pytest.mark.parametrize("site,key,bias_key,epi", [(1, "blocks.0.attn.out_proj.weight", None, 3),
                                                   (3, "blocks.1.mlp.3.weight", "blocks.1.mlp.3.bias", 3),
                                                   (4, "patch_embed.proj.2.weight", "patch_embed.proj.2.bias", 0)])
def test_folded_producers_keep_both_planes(M, site, key, bias_key, epi):
    """One stage of the folded sampler step on its own: the three producers of the split residual stream (second patch Linear:
    x = acc + bias; out_proj, fc2: x = (hi + lo) + gate (acc + bias)) through `jat_k_gemm_fold` on the tile `jat_k_gemm_plan`
    gives a folding bucket of M rows (7168: the k-step-pair kernel 39), with the model's own weights at full width.  The final
    latent dilutes what the stream loses; here hi + lo must BE the fp64 result to the 16 significant bits two planes hold
    (|hi + lo - x| <= 2^-15 max|x|: 2^-17 of rounding lo plus the fp32 accumulation), hi alone its rounding to the operand
    dtype — what `Twin(fold=True)._planes` states — and the row partial sums of x^2 the consumer's rstd is built from must be
    those of x.  (With `lo` forced to zero the two-step sampler test measures error / E0 = 1.41, under its 1.5 gate; this test
    then fails in all six cases with |hi + lo - x| = 3.9e-3 ... 7.8e-3 at max|x| = 1.5 ... 4.1.)"""
    st = setup(2)
    h = st["model"]._get_handle()
    W = cuda(st["sd"][key]).to(OP)
    N, K = W.shape
    assert N == D
    variant = _plan(h, site, M, N, K, folding=1)[0]
    wn = L.lib().jat_k_gemm_wave_n(variant)
    assert wn > 0 and N % wn == 0
    if M == 7168:
        assert variant == 39
    ntok = 128
    A = cuda(recipe.gaussian("prod_a", (M, K), site) * np.float32(0.5)).to(OP)
    bias = cuda(st["sd"][bias_key]) if bias_key else None
    gate = cuda(recipe.gaussian("prod_g", (M // ntok, N), site) * np.float32(0.3))
    x0 = cuda(recipe.gaussian("prod_x", (M, N), site) * np.float32(0.7))
    hi0 = x0.to(OP)
    lo0 = (x0 - hi0.float()).to(OP)
    y = A.double() @ W.double().T + (bias.double() if bias is not None else 0.0)
    ref = y if epi == 0 else (hi0.double() + lo0.double()) + gate.double().repeat_interleave(ntok, 0) * y
    outs = []
    for _ in range(2):
        hi, lo = hi0.clone(), lo0.clone()
        part = torch.full((M, N // wn), float("nan"), device="cuda")
        L.check(L.lib().jat_k_gemm_fold(L.ptr(A), L.ptr(W), L.ptr(bias), None, M, N, K, epi, L.ptr(gate), N, ntok, L.ptr(hi),
                                        L.ptr(lo), L.ptr(part), None, 0, variant, L.stream_ptr()))
        torch.cuda.synchronize()
        outs.append((hi, lo, part))
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    hi, lo, part = outs[0]
    scale = float(ref.abs().max())
    two, one = float(((hi.double() + lo.double()) - ref).abs().max()), float((hi.double() - ref).abs().max())
    print(f"producer site {site} M={M} variant {variant}: |hi + lo - x| {two:.3e}, |hi - x| {one:.3e}, max|x| {scale:.3e}")
    assert two <= 2 ** -15 * scale + 1e-5
    ulp = 2 ** -8 if OP == torch.bfloat16 else 2 ** -11
    assert bool(((hi.double() - ref).abs() <= ulp * ref.abs() + 1e-5).all())
    assert float(((part.double().sum(1) - (ref * ref).sum(1)).abs() / (ref * ref).sum(1)).max()) < 1e-5
