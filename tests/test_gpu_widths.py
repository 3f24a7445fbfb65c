"""The hidden sizes, head ratios and kernel instantiations `jat_model_create` accepts but no `recipe.CONFIGS` model runs.

Every model of the rest of the suite is D = 256 / 512 / 1280 with a Q / KV ratio of 2 or 5, MLP = 4 D and equal channel counts.
tests/width_cases.py holds four depth-2 models at D = 768 / 1024 / 1536 / 2048 (Q / KV 3 / 8 / 1 / 4, MLP ratio 4 / 3 / 2.5 / 2) and a
forward-only variant with input_channels != cond_channels; here they run what no other test starts:

    norm_modulate_kernel (every D but 256 / 512 / 1280), linear_f32_kernel<3, 4, 6, 8>, splitk_resid_norm_block_kernel at 192 ...
    512 threads, the head loops of attn_group_kernel / attn_fwd_kernel at G = 3 / 8 / 1 / 4, a folded sampler at D = 1024, and the
    trainer (small_dw / small_dx on other [6 D, D] weights, unpack_qkv_grad at other D / kvD, both weight-gradient tiles, MLP
    ratios other than 4) — sections 1-5;
    the instantiations behind switches that are read once per process (JAT_ATTN_KVB / QT / GROUP, JAT_NORM_RPW,
    JAT_ADAMW_BLOCKS), in child processes that re-run the per-kernel tests under them — section 6.

References and gates are the ones the suite already has, none wider: the fp64 twin (tests/forward_ref.py, pinned to the oracle at
these widths by tests/test_forward_ref_cpu.py) with error <= 1.5 E0 whole / per sample / max-abs (tests/twin_check.py) for the
forward and the sampler; the numpy training oracle with LOSS_TOL / GRAD_TOL / GRAD_TOL_SMALL of tests/test_gpu_train.py; the
element-wise one-ulp bound of tests/test_gpu_kernels.py `norm_modulate_case` for the norm kernel; 1e-5 for the fp32 time MLP.

Measured on MI355X ("Other widths"), error / E0 whole tensor; worst single sample; max-abs ratio:
    forward, 30 cases, bf16   0.995 ... 1.004 (E0 3.88e-3 ... 4.23e-3); <= 1.013; 0.82 ... 1.15
    forward, fp16 build       0.998 ... 1.015 (E0 4.87e-4 ... 5.21e-4); <= 1.042; 0.80 ... 1.16
    sampler, B = 2, default   0.989 ... 0.998 (E0 5.09e-3 ... 5.32e-3); 0.997 ... 1.003; 0.90 ... 1.02
    w1024 B = 10 (folded)     1.001; 1.012; 1.16        w1024 B = 2, folding forced   0.993; 0.995; 1.02
    norm kernel               worst element at 0.998 of its one-ulp bound (bf16), 0.967 (fp16); rel-L2 1.65e-3 ... 1.69e-3 (gate 3e-3)
    time_embed                1.3e-7 ... 1.4e-7 (gate 1e-5)
    training step             worst gradient at 0.31 ... 0.40 of its tolerance, always a q or k projection
F stayed 1.5 and the training gates the constants of tests/test_gpu_train.py.  Wall time: 26 s without the children, the children
7.4 / 8.4 / 9.2 s (181 per-kernel tests each, 21 of them test_attention_lens_*); tests/test_gpu_forward_paths.py takes 17 s for scale.
"""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import jatsr_amd  # noqa: E402
import jatsr_amd._lib as L  # noqa: E402
import jatsr_amd.recipe as recipe  # noqa: E402
from helpers import rel_l2  # noqa: E402
from jatsr_amd.model import JaT_AudioSR_V2, JaT_AudioSR_V3  # noqa: E402
from jatsr_amd.train import Trainer  # noqa: E402
from oracle import jat_oracle as O  # noqa: E402

import forward_ref as R  # noqa: E402
from test_gpu_kernels import norm_modulate_case  # noqa: E402
from test_gpu_train import GRAD_TOL, GRAD_TOL_SMALL, LOSS_TOL, make_trainer  # noqa: E402
from twin_check import check  # noqa: E402
from weight_grad_rule import dw_shapes  # noqa: E402
from width_cases import FORWARD_CONFIGS, W1536_CIN64, WIDTH_CONFIGS, WIDTHS  # noqa: E402

OP = torch.float16 if L.OPERAND_DTYPE == "fp16" else torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_state = {}


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def setup(name, norm="rms"):
    """The model `name` of FORWARD_CONFIGS with recipe weights on the device, and its twins on demand; one model resident."""
    if _state.get("key") != (name, norm):
        L.require_gpu()
        _state.clear()
        cfg = FORWARD_CONFIGS[name]
        sd = recipe.make_state_dict(cfg, norm)
        m = (JaT_AudioSR_V3 if norm == "rms" else JaT_AudioSR_V2)(**cfg)
        missing, unexpected = m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
        assert not unexpected and all(".rope." in k for k in missing)
        _state.update(key=(name, norm), cfg=cfg, sd=sd, norm=norm, model=m.to("cuda").eval(), twins={})
    return _state


def twin(st, rounded, fold=False):
    key = (rounded, fold)
    if key not in st["twins"]:
        st["twins"][key] = R.Twin(st["cfg"], st["sd"], R.make_rnd(OP if rounded else None), norm=st["norm"], fold=fold, device="cuda")
    return st["twins"][key]


def _plan(handle, site, M, N, K, folding=0):
    v, k = C.c_int32(), C.c_int32()
    L.check(L.lib().jat_k_gemm_plan(handle.ptr, site, M, N, K, folding, C.byref(v), C.byref(k)))
    return (v.value, k.value)


def _route(N, has_lse=0, has_dropout=0):
    """(group kernel, QT, KVB) of `launch_attention` for N tokens per sample, V padded to whole 64-key blocks"""
    g, qt, kvb = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    L.check(L.lib().jat_k_attention_route(N, (N + 63) // 64 * 64, has_lse, has_dropout, C.byref(g), C.byref(qt), C.byref(kvb)))
    return (g.value, qt.value, kvb.value)


# ---- 1. the norm kernel and the time MLP on their own ---------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", WIDTHS)
def test_norm_kernel_on_a_model_row_block(name, mode):
    """`jat_k_norm_modulate` as a block's norm1 launches it at this width: the model's own norm weight, one (shift, scale) row
    per sample out of the [B, 6 D] adaLN output (row stride 6 D), B = 3 samples of 18 tokens (M = 54: the last block of four
    waves has two rows), RMSNorm and LayerNorm.  Bound: tests/test_gpu_kernels.py `norm_modulate_case`."""
    st = setup(name)
    D = st["cfg"]["hidden_size"]
    ex = twin(st, False)
    t = torch.tensor([0.05, 0.5, 0.95], dtype=R.F64, device="cuda")
    mod = ex.adaln(0, ex.t_embed(t)).float().contiguous()
    x = cuda(recipe.gaussian("width_norm_x", (54, D), D + mode) * np.float32(0.7))
    w = cuda(st["sd"]["blocks.0.norm1.weight"])
    norm_modulate_case(x, w, mod[:, :D], mod[:, D:2 * D], 6 * D, 18, mode, f"{name} norm1 mode {mode}")


@pytest.mark.parametrize("name", WIDTHS)
def test_time_embed_at_width_vs_oracle(name):
    """`model.time_embed(t)` (sinusoid + linear_f32_kernel<D / 256> twice, fp32 end to end) against the oracle's fp64 embedding;
    the gate of tests/test_gpu_model.py::test_time_embed_vs_oracle.  B = 5: one full group of four batch rows and a ragged one."""
    st = setup(name)
    t = np.array([0.0, 0.02, 0.5, 0.98, 1.0], np.float32)
    got = st["model"].time_embed(cuda(t)).cpu().numpy()
    ref = O.OracleModel(st["cfg"], st["sd"], "rms", np.float64).t_embed(t)
    r = rel_l2(got, ref)
    print(f"{name} time_embed rel-L2 {r:.3e}")
    assert got.shape == ref.shape and rel_l2(got, ref) < 1e-5   # fp32 path end to end


# ---- 2. the forward ---------------------------------------------------------------------------------------------------------
# (B, T): 18 tokens with a ragged last patch; 128 tokens (attn_group_kernel: its head-pair loop at G = 3 / 8 / 1 / 4); 345 tokens
# (attn_fwd_kernel with a masked last key block, the small bucket with its split-K finishers)
FORWARD_SHAPES = [(3, 70), (2, 512), (1, 1378)]


def test_forward_shapes_reach_the_kernels_they_are_there_for():
    """Reached, not assumed: 128 tokens take the group attention kernel and 345 the streaming one (`jat_k_attention_route`);
    at (1, 1378) out_proj or fc2 is cut into K slices at two widths or more (`jat_k_gemm_plan`), so that
    splitk_resid_norm_block_kernel runs at D / 4 threads other than 64 / 128 / 320."""
    if not any(os.environ.get(k) for k in ("JAT_ATTN_GROUP", "JAT_ATTN_QT", "JAT_ATTN_KVB")):
        assert _route(128) == (1, 1, 64) and _route(345) == (0, 1, 64) and _route(18) == (0, 1, 64)
    threads = set()
    for name in WIDTHS:
        st = setup(name)
        h, D, mlp = st["model"]._get_handle(), st["cfg"]["hidden_size"], int(st["cfg"]["hidden_size"] * st["cfg"]["mlp_ratio"])
        if _plan(h, 1, 345, D, D)[1] > 1 or _plan(h, 3, 345, D, mlp)[1] > 1:
            threads.add(D // 4)
    assert len(threads - {64, 128, 320}) >= 2, threads


@pytest.mark.parametrize("B,T", FORWARD_SHAPES)
@pytest.mark.parametrize("norm", ["rms", "ln"])
@pytest.mark.parametrize("name", list(FORWARD_CONFIGS))
def test_forward_at_width_vs_fp64(name, norm, B, T):
    """`jat_forward` of the V3 (RMSNorm) and the V2 (LayerNorm) model against the twin: the output's error against the exact
    twin <= 1.5 E0 whole / per sample / max-abs, and a second run bit-identical."""
    st = setup(name, norm)
    m, cfg = st["model"], st["cfg"]
    salt = 500 + 10 * FORWARD_SHAPES.index((B, T)) + list(FORWARD_CONFIGS).index(name)
    x_t = cuda(recipe.gaussian("x_t", (B, cfg["input_channels"], T), salt))
    x_c = cuda(recipe.gaussian("x_cond", (B, cfg["cond_channels"], T), salt))
    t = torch.linspace(0.05, 0.95, B, device="cuda") if B > 1 else torch.tensor([0.35], device="cuda")
    ref64 = twin(st, False).forward(x_t, t, x_c)
    ref_r = twin(st, True).forward(x_t, t, x_c)
    got = m(x_t, t, x_c)
    assert got.shape == x_t.shape
    check(f"{name} {norm} forward {B}x{T}", got, torch.zeros_like(ref64), ref64, ref_r)
    assert torch.equal(got, m(x_t, t, x_c))


# ---- 3. the sampler ---------------------------------------------------------------------------------------------------------
def _two_steps(name, B, fold_switch, folded):
    st = setup(name)
    m, h, C_, T = st["model"], st["model"]._get_handle(), st["cfg"]["input_channels"], 512
    lr = cuda(recipe.gaussian("width_lr", (B, C_, T), 300 + B))
    z0 = cuda(recipe.gaussian("width_z0", (B, C_, T), 400 + B))
    m.__dict__.pop("_jat_samplers", None)         # a bucket built under another "fold_norm" must not be reused
    h.set_switch("fold_norm", fold_switch)
    try:
        got = jatsr_amd.flow_matching_sample(m, lr, num_steps=2, cfg_scale=3.0, verbose=False, z0=z0)
        info = m._jat_samplers[(B, T, 2, 3.0)].info()
        assert info["folded"] is folded and info["fused_attn"] is False, info
        again = jatsr_amd.flow_matching_sample(m, lr, num_steps=2, cfg_scale=3.0, verbose=False, z0=z0)
    finally:
        h.set_switch("fold_norm", 1)
        m.__dict__.pop("_jat_samplers", None)     # release the bucket's buffers and folded weights
    ref64 = twin(st, False, fold=folded).sample(lr, z0, 2, 3.0)
    ref_r = twin(st, True, fold=folded).sample(lr, z0, 2, 3.0)
    check(f"{name} sampler B={B} fold switch {fold_switch}", got, torch.zeros_like(ref64), ref64, ref_r)
    assert torch.equal(got, again)


@pytest.mark.parametrize("name", WIDTHS)
def test_two_sampler_steps_at_width_vs_fp64(name):
    """Two CFG Euler steps (scale 3) at B = 2, T = 512 under the default switches (M = 512: the un-folded small bucket, the group
    attention kernel) against the twin's sampler."""
    _two_steps(name, 2, 1, False)


def test_two_sampler_steps_folded_by_default_at_d1024():
    """w1024 at B = 10 (2560 rows per forward, above the split-K buckets): D / 64 = 16 row partials, the bucket folds its norms
    by default, on whichever 64-column tile the chooser takes.  The twin moves its rounding points with it (fold=True)."""
    _two_steps("w1024", 10, 1, True)


@pytest.mark.parametrize("name", WIDTHS)
def test_two_sampler_steps_with_folding_forced(name):
    """"fold_norm" = 2 asks every bucket to fold: at D = 1024 the B = 2 bucket does (16 partials); at 768 / 1536 / 2048 it must
    not (D / 64 = 12, 24, 32: not a slot count the consumers read) and must still be right."""
    _two_steps(name, 2, 2, name == "w1024")


def test_short_row_in_a_longer_bucket_at_d768():
    """`lengths=` on w768 (Q / KV 3): a short ragged row in a longer bucket equals its stand-alone run, the full-length rows stay
    bit-identical (the pattern and the gate of tests/test_gpu_model.py::test_short_row_in_a_longer_bucket_equals_its_stand_alone_run)."""
    m = setup("w768")["model"]
    Cc, T, short = 32, 92, 37
    lr = recipe.gaussian("len_lr", (3, Cc, T), short)
    z0 = recipe.gaussian("len_z0", (3, Cc, T), short + 100)
    lr[1, :, short:] = 0
    z0[1, :, short:] = 0
    kw = dict(num_steps=6, cfg_scale=2.5, verbose=False)
    try:
        both = jatsr_amd.flow_matching_sample(m, cuda(lr), z0=cuda(z0), lengths=[T, short, T], **kw)
        alone = jatsr_amd.flow_matching_sample(m, cuda(lr[1:2, :, :short]), z0=cuda(z0[1:2, :, :short]), **kw)
        full = jatsr_amd.flow_matching_sample(m, cuda(lr[[0, 2]]), z0=cuda(z0[[0, 2]]), **kw)
    finally:
        m.__dict__.pop("_jat_samplers", None)
    assert rel_l2(both[1:2, :, :short].cpu().numpy(), alone.cpu().numpy()) < 2e-5
    assert torch.equal(both[[0, 2]], full)


# ---- 4. what the model admits but the sampler and the trainer do not --------------------------------------------------------
def test_unequal_channel_counts_are_rejected_where_sampler_and_trainer_are_created():
    """input_channels != cond_channels is a model the forward takes (section 2).  The sampler and the trainer condition on a
    latent of the sampled / target shape: they must say so when they are created, not read the condition at the wrong stride."""
    m = setup("w1536_cin64")["model"]
    assert (m.input_channels, m.cond_channels) == (W1536_CIN64["input_channels"], W1536_CIN64["cond_channels"]) == (64, 32)
    with pytest.raises(ValueError, match="cond_channels"):
        jatsr_amd.Sampler(m, 2, 64, 2, 3.0)
    with pytest.raises(ValueError, match="cond_channels"):
        Trainer(m, batch_size=2, frames=24, use_grad_scaler=False)


# ---- 5. the training step ---------------------------------------------------------------------------------------------------
TRAIN_CASES = [(name, B, T, norm) for name in WIDTHS for B, T, norm in ((3, 70, "rms"), (1, 9, "ln"))] + [("w2048", 2, 300, "rms")]


def test_training_cases_use_both_weight_gradient_tiles():
    """Over TRAIN_CASES the seven GEMM-shaped weight gradients of a model take the 128 and the 256 tile (`jat_k_weight_grad_plan`:
    what the trainer launches; `out * in >= 2^20` -> 256 x 256)."""
    tiles = set()
    for name, B, T, _ in TRAIN_CASES:
        cfg = WIDTH_CONFIGS[name]
        D = cfg["hidden_size"]
        for out, inn in dw_shapes(D, cfg["num_kv_heads"], cfg["bottleneck_dim"], int(D * cfg["mlp_ratio"]), cfg["input_channels"],
                                  cfg["cond_channels"]):
            tile, ks = C.c_int32(-1), C.c_int32(-1)
            L.check(L.lib().jat_k_weight_grad_plan(out, inn, B * ((T + 3) // 4), C.byref(tile), C.byref(ks)))
            tiles.add(tile.value)
    assert tiles == {128, 256}, tiles


def _train_case(cfg, B, T, norm, salt, t, plan=None, mask_seed=None, rates=None):
    from oracle import jat_oracle_train as OT
    C_ = cfg["input_channels"]
    meta = dict(cfg=cfg, norm=norm, salt=salt, B=B, T=T, lr=1e-4, wd=0.1, clip=1.0)
    _state.clear()                                  # the forward sections' model leaves the device
    m, tr = make_trainer(meta, use_grad_scaler=False, condition_noise_ratio=0.0)
    if rates is not None:
        tr.set_regularisers(*rates)
    z_t = recipe.gaussian("zt", (B, C_, T), salt)
    cond = recipe.gaussian("cond", (B, C_, T), salt + 1)
    target = recipe.gaussian("target", (B, C_, T), salt + 2)
    kw = {} if mask_seed is None else dict(mask_seed=mask_seed)
    tr.forward_backward(cuda(z_t), cuda(t), cuda(cond), cuda(target), **kw)
    sd = recipe.make_state_dict(cfg, norm, salt)
    okw = {} if plan is None else dict(plan=OT.DropPlan(mask_seed, *rates))
    loss, grads, _ = OT.TrainOracle(cfg, sd, norm).loss_and_grads(z_t, t, cond, target, **okw)
    assert abs(float(tr._scal[0]) - loss) <= LOSS_TOL * loss
    gn = math.sqrt(sum(float((g * g).sum()) for g in grads.values()))
    worst, worst_k = 0.0, None
    for k, g in grads.items():
        r = rel_l2((tr.grad(k) / tr.scaler.scale).cpu().numpy(), g)
        tol = GRAD_TOL if np.linalg.norm(g) >= 1e-3 * gn else GRAD_TOL_SMALL
        if r / tol > worst:
            worst, worst_k = r / tol, k
        assert r <= tol, f"{k}: {r:.3e}"
    return loss, worst, worst_k


@pytest.mark.parametrize("name,B,T,norm", TRAIN_CASES)
def test_train_step_at_width_vs_numpy_oracle(name, B, T, norm):
    """One forward + backward of the trainer against the numpy oracle's hand-derived fp64 backward, driven as
    tests/test_gpu_train.py::test_train_step_vs_numpy_oracle with its constants: odd batch and ragged T (18 tokens), a single
    sample of 3 tokens with LayerNorm, and w2048 at 150 rows."""
    salt = 40 + TRAIN_CASES.index((name, B, T, norm))
    t = np.linspace(0.03, 0.97, B).astype(np.float32)
    loss, worst, k = _train_case(WIDTH_CONFIGS[name], B, T, norm, salt, t)
    print(f"{name} B={B} T={T} {norm}: loss {loss:.5f}, worst gradient at {worst:.2f} of tolerance ({k})")


def test_dropout_and_droppath_at_d768_vs_numpy_oracle():
    """Dropout 0.1 / DropPath 0.5 on w768 (GQA groups of 3), as tests/test_gpu_train.py::test_dropout_full_width_vs_numpy_oracle:
    the kernels regenerate the masks the numpy mirror builds from the same seed."""
    loss, worst, k = _train_case(WIDTH_CONFIGS["w768"], 2, 132, "rms", 31, np.asarray([0.2, 0.8], np.float32), plan=True,
                                 mask_seed=0xC0FFEE1234, rates=([0.1, 0.1], [0.0, 0.5]))
    print(f"w768 dropout: loss {loss:.5f}, worst gradient at {worst:.2f} of tolerance ({k})")


# ---- 6. the instantiations behind once-per-process switches ----------------------------------------------------------------
# environment, and the (group, QT, KVB) `launch_attention` must take under it for the eval call at N = 128 and N = 345 and
# for the training forward (lse) at N = 128
CHILDREN = {
    "child1": (dict(JAT_ATTN_KVB="128", JAT_ATTN_GROUP="0", JAT_NORM_RPW="0", JAT_ADAMW_BLOCKS="3"),
               [(128, 0, (0, 1, 128)), (345, 0, (0, 1, 128)), (128, 1, (0, 1, 128))]),
    "child2": (dict(JAT_ATTN_QT="2", JAT_ATTN_GROUP="0", JAT_NORM_RPW="4"),
               [(128, 0, (0, 2, 64)), (345, 0, (0, 2, 64)), (128, 1, (0, 2, 64))]),
    "child3": (dict(JAT_ATTN_KVB="128", JAT_ATTN_QT="2", JAT_NORM_RPW="2"),
               [(128, 0, (1, 2, 128)), (345, 0, (0, 2, 128)), (128, 1, (0, 2, 128))]),
}
# the attention and norm tests of test_gpu_kernels.py, the attention training forward / backward of test_gpu_train_kernels.py
# without the two 64-bit-index tests, the AdamW kernels (test_gpu_train_kernels.py, test_gpu_ema.py)
# what CHILD_TESTS selects: 160 tests, and the 21 test_attention_lens_* of tests/test_gpu_kernels.py (per-sample key counts on the
# switched instantiations); pinned so that a renamed test cannot leave the children unseen
CHILD_COUNT = 181
CHILD_TESTS = ("(test_attention or test_norm_modulate or test_norm_no_modulation or test_adamw or test_fused_adamw_ema_kernel) "
               "and not 64bit")
CHILD_CODE = """
import ctypes as C, json, sys
import pytest
import jatsr_amd._lib as L
for N, lse, want in json.loads(sys.argv[1]):
    g, qt, kvb = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    L.check(L.lib().jat_k_attention_route(N, (N + 63) // 64 * 64, lse, 0, C.byref(g), C.byref(qt), C.byref(kvb)))
    assert [g.value, qt.value, kvb.value] == want, (N, lse, [g.value, qt.value, kvb.value], want)
print("routes as intended")
sys.exit(pytest.main(sys.argv[2:]))
"""


@pytest.mark.parametrize("child", list(CHILDREN))
def test_switched_kernels_in_a_child_process(child):
    """attn_fwd_kernel<1, 128>, <2, 64>, <2, 128> (at N <= 128 too, with JAT_ATTN_GROUP=0), the multi-row loop of
    norm_modulate_rows_kernel (JAT_NORM_RPW = 4 / 2; 0 sends 256 / 512 / 1280 to norm_modulate_kernel) and the grid-stride loop of
    the AdamW kernels (JAT_ADAMW_BLOCKS=3) exist only behind switches the library reads once per process.  A fresh child first
    asserts through `jat_k_attention_route` — the function `launch_attention` itself calls — that it is on the intended
    instantiation, then runs the existing per-kernel tests unchanged, in the same process."""
    import json
    env_add, routes = CHILDREN[child]
    env = dict(os.environ, **env_add)
    env.pop("JAT_LIB_PATH", None)
    args = ["-x", "-q", "-p", "no:cacheprovider", "-m", "gpu", "tests/test_gpu_kernels.py", "tests/test_gpu_train_kernels.py",
            "tests/test_gpu_ema.py", "-k", CHILD_TESTS]
    out = subprocess.run([sys.executable, "-c", CHILD_CODE, json.dumps([[n, lse, list(w)] for n, lse, w in routes])] + args,
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    tail = (out.stdout + out.stderr)[-3000:]
    print(tail)
    assert out.returncode == 0 and "routes as intended" in out.stdout and " passed" in out.stdout, tail
    assert "skipped" not in out.stdout.splitlines()[-1] and "no tests ran" not in out.stdout, tail
    assert re.search(r"\b%d passed\b" % CHILD_COUNT, out.stdout.splitlines()[-1]), tail
