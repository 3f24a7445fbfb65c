"""Gradient accumulation on the GPU: the accumulate mode of every kernel that writes a parameter gradient
(`jat_k_weight_grad_ex`, `jat_trainer_fwd_bwd_ex` with JAT_FB_ACCUMULATE / JAT_FB_NO_HOOK), `Trainer(grad_accum_steps=k)` and
`fit --grad-accum-steps K`.

What is asserted bit for bit: an accumulating launch stores `old + g` with g the very fp32 value the overwriting launch
stores and one rounded add, so k accumulated micro-batches leave ((g0 + g1) + g2) ... in the flat buffer — compared with
torch's own fp32 add of the single runs (`torch.equal`).  What is asserted against the fp64 oracle uses the gates of
tests/test_gpu_train.py `test_train_step_vs_numpy_oracle`, unchanged: the oracle sees the concatenated batch of k * B samples,
whose mean loss is the mean of the k losses and whose gradient is the accumulated one over scale * k."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import jatsr_amd  # noqa: E402
import jatsr_amd._lib as L  # noqa: E402
import jatsr_amd.io as jio  # noqa: E402
import jatsr_amd.recipe as recipe  # noqa: E402
from helpers import rel_l2  # noqa: E402
from weight_grad_rule import tn_path  # noqa: E402
from jatsr_amd import fit as F  # noqa: E402
from jatsr_amd.data import LatentStore, epoch_batches, train_batch_plan  # noqa: E402
from jatsr_amd.model import JaT_AudioSR_V2, JaT_AudioSR_V3  # noqa: E402
from jatsr_amd.prepare import final_stats  # noqa: E402
from jatsr_amd.train import Trainer  # noqa: E402

FP16 = L.OPERAND_DTYPE == "fp16"
OP = torch.float16 if FP16 else torch.bfloat16
FP16_TEST_SCALE = 4096.0          # fixed loss scale of the fp16-operand library with the dynamic scaler off, as in test_gpu_train.py
GRAD_TOL, GRAD_TOL_SMALL, LOSS_TOL, GNORM_TOL = 3e-2, 8e-2, 2e-3, 1e-2    # the gates of test_train_step_vs_numpy_oracle


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


# ---- 1. the kernel ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_db", [True, False])
@pytest.mark.parametrize("out,inn,tokens,tile,split", [(128, 128, 100, 128, False), (256, 256, 1100, 128, True),
                                                       (1024, 1024, 200, 256, False), (1024, 1024, 1100, 256, True)])
def test_weight_grad_accumulate_is_prefill_plus_overwrite_result(out, inn, tokens, tile, split, with_db):
    got_tile, ks = tn_path(out, inn, tokens)
    assert got_tile == tile and (ks > 1) == split, (got_tile, ks)       # the four shapes take the four paths
    lib_tile, lib_ks = ctypes.c_int32(-1), ctypes.c_int32(-1)           # ... by the library's own account of its launch
    L.check(L.lib().jat_k_weight_grad_plan(out, inn, tokens, ctypes.byref(lib_tile), ctypes.byref(lib_ks)))
    assert lib_tile.value == tile and (lib_ks.value > 1) == split and (lib_tile.value, lib_ks.value) == (got_tile, ks)
    if not split:
        assert tokens % 64 != 0                                         # ragged last K-tile in the one-slice launches
    g = torch.Generator(device="cpu").manual_seed(1000 + out + tokens)
    dY = (torch.randn((tokens, out), generator=g) * 0.05).to("cuda").to(OP)
    X = (torch.randn((tokens, inn), generator=g) + 0.25).to("cuda").to(OP)
    work = torch.full((64 + 16 * out * inn + 32 * out,), float("nan"), device="cuda")

    def run(dW, db, accumulate):
        L.check(L.lib().jat_k_weight_grad_ex(L.ptr(dY), L.ptr(X), L.ptr(dW), L.ptr(db) if with_db else None, tokens, out, inn, 0,
                                             L.ptr(work), work.numel() * 4, accumulate, L.stream_ptr()))
        torch.cuda.synchronize()
    dW0 = torch.full((out, inn), float("nan"), device="cuda")
    db0 = torch.full((out,), float("nan"), device="cuda")
    run(dW0, db0, 0)
    assert bool(torch.isfinite(dW0).all()) and float(dW0.abs().sum()) > 0
    pre_w = torch.randn((out, inn), generator=g).to("cuda") * float(dW0.abs().mean()) + 0.37     # random, non-zero, of the result's size
    pre_b = torch.randn((out,), generator=g).to("cuda") + 2.5
    assert bool((pre_w != 0).all()) and bool((pre_b != 0).all())
    dW1, db1 = pre_w.clone(), pre_b.clone()
    run(dW1, db1, 1)
    assert torch.equal(dW1, pre_w + dW0)
    if with_db:
        assert torch.equal(db1, pre_b + db0)
    else:
        assert torch.equal(db1, pre_b)                                  # not touched
    # accumulate == 0 of the new entry point is the old one
    dW2 = torch.full((out, inn), float("nan"), device="cuda")
    L.check(L.lib().jat_k_weight_grad(L.ptr(dY), L.ptr(X), L.ptr(dW2), None, tokens, out, inn, 0, L.ptr(work), work.numel() * 4,
                                      L.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(dW2, dW0)


# ---- trainers -----------------------------------------------------------------------------------------------------------
def build(cfg_name, norm, salt, B, T, dropout=0.0, drop_path=0.0, **kw):
    L.require_gpu()
    cfg = recipe.CONFIGS[cfg_name]
    cls = JaT_AudioSR_V3 if norm == "rms" else JaT_AudioSR_V2
    m = cls(**cfg, dropout=dropout, drop_path_rate=drop_path)
    sd = {k: torch.from_numpy(v) for k, v in recipe.make_state_dict(cfg, norm, salt).items()}
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all(".rope." in k for k in missing)
    m = m.to("cuda")
    kw = dict(dict(use_grad_scaler=False, condition_noise_ratio=0.0, lr=1e-4, weight_decay=0.1, grad_clip=1.0), **kw)
    tr = Trainer(m, batch_size=B, frames=T, **kw)
    if FP16 and not kw["use_grad_scaler"]:
        tr.scaler.scale = FP16_TEST_SCALE
    return m, tr


def micro_inputs(cfg_name, B, T, salt, j):
    """(z_t, t, cond, target) of micro-batch j, as numpy."""
    C = recipe.CONFIGS[cfg_name]["input_channels"]
    z_t = recipe.gaussian("zt", (B, C, T), salt + 10 * j)
    cond = recipe.gaussian("cond", (B, C, T), salt + 10 * j + 1)
    target = recipe.gaussian("target", (B, C, T), salt + 10 * j + 2)
    t = np.linspace(0.03 + 0.02 * j, 0.97 - 0.03 * j, B).astype(np.float32)
    return z_t, t, cond, target


def fwd_bwd_c(tr, x, seed, flags):
    """One call straight through the C ABI (the trainer object counts nothing)."""
    z_t, t, cond, target = x
    L.check(L.lib().jat_trainer_fwd_bwd_ex(tr.ptr, L.ptr(z_t), L.ptr(t), L.ptr(cond), L.ptr(target), L.ptr(cond), float(tr.scaler.scale),
                                           ctypes.c_uint64(seed), L.ptr(tr._scal), None, flags, L.stream_ptr()))


def gap_mask(tr):
    used = torch.zeros(tr.grads.numel(), dtype=torch.bool, device="cuda")
    for _, off, n, _ in tr.layout:
        used[off:off + n] = True
    return ~used


SEEDS = (0x1234567, 0x89ABCDEF01, 0x5555AAAA5555)


@pytest.mark.parametrize("cfg_name,norm,B,T,kw,env", [
    ("micro", "rms", 2, 22, dict(dropout=0.1, drop_path=0.1), None),
    ("micro", "rms", 2, 22, dict(dropout=0.1, drop_path=0.1), ("JAT_DW_STREAM", "0")),
    ("micro", "ln", 1, 9, {}, None),
    ("micro", "rms", 2, 22, dict(latent_loss_weight=0.3), None),
    ("wide2", "rms", 3, 1378, {}, None),
], ids=["micro_rms_T22_drop", "micro_rms_T22_drop_one_stream", "micro_ln_B1_T9", "micro_latent_loss",
        "wide2_B3_T1378"])
def test_three_accumulated_micro_batches_equal_the_sum_of_the_single_runs(cfg_name, norm, B, T, kw, env, monkeypatch):
    """Every parameter, bit for bit: singles in overwrite mode through the C ABI, then the same three through
    `Trainer.forward_backward`, which overwrites on call 0 and accumulates on calls 1 and 2."""
    if env:
        monkeypatch.setenv(*env)          # read in jat_trainer_create
    salt = 31
    m, tr = build(cfg_name, norm, salt, B, T, grad_accum_steps=3, **kw)
    latent = kw.get("latent_loss_weight", 0.0) != 0.0
    xs = [tuple(cuda(a) for a in micro_inputs(cfg_name, B, T, salt, j)) for j in range(3)]
    singles, losses, terms = [], [], []
    out6 = torch.zeros(6, device="cuda")
    for x, seed in zip(xs, SEEDS):
        fwd_bwd_c(tr, x, seed, 0)
        singles.append(tr.grads.clone())
        losses.append(tr._scal[0].clone())
        if latent:
            L.check(L.lib().jat_trainer_loss_terms(tr.ptr, L.ptr(out6), L.stream_ptr()))
            terms.append(out6.clone())
    assert all(bool(torch.isfinite(g).all()) for g in singles)
    assert not torch.equal(singles[0], singles[1]) and not torch.equal(singles[1], singles[2])
    for x, seed in zip(xs, SEEDS):
        z_t, t, cond, target = x
        tr.forward_backward(z_t, t, cond, target, mask_seed=seed, cond_clean=cond)
    torch.cuda.synchronize()
    want = (singles[0] + singles[1]) + singles[2]
    assert torch.equal(tr.grads, want)
    assert not bool(tr.grads[gap_mask(tr)].any())         # alignment gaps between the tensors (if the layout has any) stay zero
    for name, off, n, _ in tr.layout:                     # every tensor took part: none is left at a single run's value
        assert float(singles[2][off:off + n].abs().sum()) > 0 and not torch.equal(tr.grads[off:off + n], singles[2][off:off + n]), name
    assert torch.equal(tr._scal[0], (losses[0] + losses[1]) + losses[2])
    if latent:
        sums = ((terms[0] + terms[1]) + terms[2]).tolist()            # fp32 sums on the device, the division on the host
        got = tr.loss_terms()
        assert [got[k] for k in ("total", "mse", "freq", "ms", "consistency", "latent")] == [v / 3 for v in sums]
        assert got["total"] == float(tr._scal[0]) / 3 and all(v > 0 for v in got.values())


# ---- 3. meaning ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm,B,k,T,salt", [("rms", 2, 3, 70, 41), ("ln", 1, 2, 9, 42)])
def test_accumulated_step_vs_numpy_oracle_on_the_concatenated_batch(norm, B, k, T, salt):
    from oracle import jat_oracle_train as OT
    cfg = recipe.CONFIGS["micro"]
    m, tr = build("micro", norm, salt, B, T, grad_accum_steps=k)
    xs = [micro_inputs("micro", B, T, salt, j) for j in range(k)]
    for z_t, t, cond, target in xs:
        tr.forward_backward(cuda(z_t), cuda(t), cuda(cond), cuda(target))
    grads_dev = tr.grads.clone()
    scale = tr.scaler.scale
    got_loss, got_norm = tr.optimizer_step()
    cat = [np.concatenate([x[i] for x in xs]) for i in range(4)]
    sd = recipe.make_state_dict(cfg, norm, salt)
    loss, grads, _ = OT.TrainOracle(cfg, sd, norm).loss_and_grads(*cat)
    print(f"{norm} B={B} k={k}: loss {got_loss} vs {loss}")
    assert abs(got_loss - loss) <= LOSS_TOL * loss
    gn = math.sqrt(sum(float((g * g).sum()) for g in grads.values()))
    print(f"grad norm {got_norm} vs {gn}")
    assert abs(got_norm - gn) <= GNORM_TOL * gn
    by_name = {name: grads_dev[off:off + n].view(shape) for name, off, n, shape in tr.layout}
    worst = 0.0
    for name, g in grads.items():
        r = rel_l2((by_name[name] / (scale * k)).cpu().numpy(), g)
        tol = GRAD_TOL if np.linalg.norm(g) >= 1e-3 * gn else GRAD_TOL_SMALL
        worst = max(worst, r / tol)
        assert r <= tol, f"{name}: {r:.3e}"
    print(f"worst gradient at {worst:.2f} of tolerance")


# ---- 4. the optimiser ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ema", [None, 0.99])
@pytest.mark.parametrize("k", [2, 4])
def test_k_equal_micro_batches_step_like_one(k, ema):
    """k times the same micro-batch sums to k * g exactly for k = 2 and 4, the un-scale factor 1 / (scale * k) is a power of
    two, and so is every quantity of the norm: the step is the plain step, bit for bit."""
    salt, B, T = 51, 2, 24
    x = tuple(cuda(a) for a in micro_inputs("micro", B, T, salt, 0))
    m0, tr0 = build("micro", "rms", salt, B, T, ema_decay=ema)
    tr0.forward_backward(*x)
    loss0, norm0 = tr0.optimizer_step(lr=1e-3)
    m1, tr1 = build("micro", "rms", salt, B, T, ema_decay=ema, grad_accum_steps=k)
    for _ in range(k):
        tr1.forward_backward(*x, mask_seed=tr1.step_seed())
    loss1, norm1 = tr1.optimizer_step(lr=1e-3)
    torch.cuda.synchronize()
    assert (loss1, norm1) == (loss0, norm0) and math.isfinite(norm0) and norm0 > 0
    assert torch.equal(tr1.params, tr0.params) and torch.equal(tr1.exp_avg, tr0.exp_avg) and torch.equal(tr1.exp_avg_sq, tr0.exp_avg_sq)
    assert (tr1.global_step, tr1.opt_step) == (tr0.global_step, tr0.opt_step) == (1, 1)
    if ema is not None:
        assert torch.equal(tr1.ema, tr0.ema) and tr1.ema_updates == 1 and not torch.equal(tr1.ema, tr1.params)


# ---- 5. a skipped step --------------------------------------------------------------------------------------------------
def test_a_non_finite_micro_batch_skips_the_whole_step():
    salt, B, T, k = 61, 2, 24, 3
    m, tr = build("micro", "rms", salt, B, T, use_grad_scaler=True, grad_accum_steps=k)
    if FP16:
        tr.scaler.scale = FP16_TEST_SCALE     # the dynamic scaler stays on; a start that fp16 gradients do not overflow at
    xs = [tuple(cuda(a) for a in micro_inputs("micro", B, T, salt, j)) for j in range(k)]
    before = (tr.params.clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone())
    s0 = tr.scaler.scale
    for j, x in enumerate(xs):
        tr.forward_backward(*x)
        if j == 1:
            tr.grads[5] = float("inf")        # as test_non_finite_gradients_skip_the_update does, in the middle micro-batch
    loss, gnorm = tr.optimizer_step(lr=1e-3)
    assert not np.isfinite(gnorm)
    assert all(torch.equal(a, b) for a, b in zip((tr.params, tr.exp_avg, tr.exp_avg_sq), before))
    assert tr.scaler.scale == s0 * 0.5 and (tr.global_step, tr.opt_step) == (1, 0)
    tr.forward_backward(*xs[0])               # the next step starts by overwriting: nothing of the skipped one is left
    torch.cuda.synchronize()
    assert bool(torch.isfinite(tr.grads).all())
    for x in xs[1:]:
        tr.forward_backward(*x)
    loss, gnorm = tr.optimizer_step(lr=1e-3)
    assert np.isfinite(gnorm) and np.isfinite(loss) and (tr.global_step, tr.opt_step) == (2, 1)
    assert not torch.equal(tr.params, before[0]) and tr.scaler.scale == s0 * 0.5


def test_real_overflow_inside_an_accumulated_step_skips_it_once(monkeypatch):
    """torch's GradScaler under accumulation, with the overflow made by the arithmetic and not planted: fp16 operands above 65504
    at a 2^30 loss scale (the fp16 library; the bf16 one overflows nowhere at 2^16 and must take every step).  One scale for the
    k micro-batches of a step; a step with an overflowed micro-batch changes no optimiser state, halves the scale once and counts
    as a batch but not as an update; the step after it starts by overwriting."""
    salt, B, T, k = 91, 2, 24, 3
    fp16 = L.operand_dtype() == "fp16"
    m, tr = build("micro", "rms", salt, B, T, use_grad_scaler=True, grad_accum_steps=k)
    tr.scaler.scale = 2.0 ** 30 if fp16 else 65536.0
    xs = [tuple(cuda(a) for a in micro_inputs("micro", B, T, salt, j)) for j in range(k)]
    passed = []                                   # the loss scale of every launch, as the C ABI receives it
    real = L.lib().jat_trainer_fwd_bwd_ex

    def spy(*args):
        passed.append(args[6])
        return real(*args)
    monkeypatch.setattr(L.lib(), "jat_trainer_fwd_bwd_ex", spy)

    def finite(x):
        return bool(torch.isfinite(x).all())
    taken, skipped, after_skip, clean_restarts = [], 0, False, 0
    for step in range(40):
        if tr.opt_step == 4:
            break
        before = (tr.params.clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone())
        s0, counts = tr.scaler.scale, (tr.global_step, tr.opt_step)
        del passed[:]
        overflowed = False
        for j, x in enumerate(xs):
            tr.forward_backward(*x)
            if j == 0 and after_skip:
                # what this call leaves is what it leaves in a zeroed buffer: nothing of the skipped step's inf survives
                got = tr.grads.clone()
                tr.grads.zero_()
                fwd_bwd_c(tr, x, tr.step_seed(micro=0), L.FB_NO_HOOK)       # overwrite mode again (no dropout: the seed is not read)
                assert torch.equal(got.view(torch.int32), tr.grads.view(torch.int32))
                clean_restarts += finite(got)
            overflowed = overflowed or not finite(tr.grads)
        assert len(passed) == k + int(after_skip) and set(passed) == {s0}, (passed, s0)
        loss, gnorm = tr.optimizer_step(lr=1e-3)
        assert overflowed == (not math.isfinite(gnorm)), (step, overflowed, gnorm)
        if overflowed:
            skipped += 1
            assert all(torch.equal(a, b) for a, b in zip((tr.params, tr.exp_avg, tr.exp_avg_sq), before)), step
            assert tr.scaler.scale == s0 * 0.5                              # once, not once per micro-batch
            assert (tr.global_step, tr.opt_step) == (counts[0] + 1, counts[1])
        else:
            taken.append((loss, gnorm))
            assert tr.scaler.scale == s0 and (tr.global_step, tr.opt_step) == (counts[0] + 1, counts[1] + 1)
            assert not torch.equal(tr.params, before[0])
        after_skip = overflowed
    print(f"{'fp16' if fp16 else 'bf16'}: {skipped} skipped, {len(taken)} taken, final scale {tr.scaler.scale}, taken {taken}")
    assert tr.opt_step == 4 == len(taken) and tr.global_step == 4 + skipped
    assert all(math.isfinite(a) and math.isfinite(b) and b > 0 for a, b in taken)
    if fp16:
        assert skipped >= 1 and clean_restarts >= 1, "a 2^30 loss scale must overflow fp16 operands at least once"
        assert tr.scaler.scale == 2.0 ** (30 - skipped)
    else:
        assert skipped == 0 and tr.scaler.scale == 65536.0


# ---- 6. the gradient-ready hook -----------------------------------------------------------------------------------------
def test_hook_fires_only_in_the_last_micro_batch_single_rank_rccl():
    import socket
    import torch.distributed as dist
    salt, B, T, k = 71, 2, 24, 3
    xs = [tuple(cuda(a) for a in micro_inputs("micro", B, T, salt, j)) for j in range(k)]
    m0, tr0 = build("micro", "rms", salt, B, T, overlap_grad_allreduce=False, grad_accum_steps=k)
    for x in xs:
        tr0.forward_backward(*x)
    tr0.optimizer_step(lr=1e-4)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    try:
        m1, tr1 = build("micro", "rms", salt, B, T, overlap_grad_allreduce="force", grad_accum_steps=k)
        calls = []
        orig = tr1._on_grads_ready

        def spy(off, n, user):
            calls.append((off, n))
            orig(off, n, user)
        tr1._hook = L.GRAD_HOOK(spy)
        L.check(L.lib().jat_trainer_set_grad_hook(tr1.ptr, ctypes.cast(tr1._hook, ctypes.c_void_p), None))
        for x in xs[:-1]:
            tr1.forward_backward(*x)
            assert calls == [] and tr1._pending == [] and tr1._covered == 0        # silent: not the last micro-batch
        tr1.forward_backward(*xs[-1])
        depth = recipe.CONFIGS["micro"]["depth"]
        assert len(calls) == depth + 2 and len(tr1._pending) == depth + 2
        spans = sorted(calls)
        assert spans[0][0] == 0 and all(spans[i][0] + spans[i][1] == spans[i + 1][0] for i in range(len(spans) - 1))
        assert spans[-1][0] + spans[-1][1] == tr1.grads.numel() == tr1._covered     # [0, total) exactly once
        tr1.optimizer_step(lr=1e-4)
        torch.cuda.synchronize()
        assert torch.equal(tr1.grads, tr0.grads) and torch.equal(tr1.params, tr0.params)
    finally:
        dist.destroy_process_group()


# ---- 7. misuse ----------------------------------------------------------------------------------------------------------
def test_miscounted_calls_and_bad_arguments_are_refused():
    salt, B, T = 81, 1, 9
    m, tr = build("micro", "rms", salt, B, T, grad_accum_steps=2)
    x = tuple(cuda(a) for a in micro_inputs("micro", B, T, salt, 0))
    tr.forward_backward(*x)
    with pytest.raises(L.JatError, match=r"after 1 forward_backward call.*grad_accum_steps is 2"):
        tr.optimizer_step()
    tr.forward_backward(*x)
    with pytest.raises(L.JatError, match=r"call 3 .*grad_accum_steps is 2"):
        tr.forward_backward(*x)
    with pytest.raises(L.JatError, match="last"):
        tr.accumulate_normalised(x[3], x[2])
    loss, gnorm = tr.optimizer_step()            # the two calls made are a complete step
    assert np.isfinite(loss) and np.isfinite(gnorm) and tr.global_step == 1
    torch.cuda.synchronize()
    allocated = torch.cuda.memory_allocated()
    for bad in (0, -1):
        with pytest.raises(ValueError, match="grad_accum_steps"):
            Trainer(m, batch_size=B, frames=T, grad_accum_steps=bad)
    assert torch.cuda.memory_allocated() == allocated and not tr._detached     # the model's trainer was not touched
    # flag bits the library does not know
    z_t, t, cond, target = x
    rc = L.lib().jat_trainer_fwd_bwd_ex(tr.ptr, L.ptr(z_t), L.ptr(t), L.ptr(cond), L.ptr(target), None, 1.0, ctypes.c_uint64(1),
                                        None, None, 4, L.stream_ptr())
    assert rc == L.JAT_E_INVALID


# ---- 8. fit ----------------------------------------------------------------------------------------------------------------
C_, FRAMES, BATCH, ACCUM = 32, 40, 2, 2
TRAIN_LENGTHS = [64, 41, 25, 90, 40, 77, 58, 120, 33, 71]      # 5 batches of 2 per epoch: 2 optimiser steps of 2, 1 batch left over
VAL_LENGTHS = [50, 44]


def write_folder(root):
    g = torch.Generator().manual_seed(4321)
    s = torch.zeros(2 * C_, dtype=torch.float64)
    q = torch.zeros(2 * C_, dtype=torch.float64)
    count = 0
    scale = torch.linspace(0.5, 2.0, C_).view(-1, 1)
    for split, lengths in (("train", TRAIN_LENGTHS), ("val", VAL_LENGTHS)):
        os.makedirs(os.path.join(root, split))
        for i, n in enumerate(lengths):
            hr = (torch.randn(C_, n, generator=g) * scale + 0.3).to(torch.float16)
            lr = (hr.float() * 0.7 + torch.randn(C_, n, generator=g) * 0.2 - 0.1).to(torch.float16)
            jio.save_latent_file(os.path.join(root, split, f"clip_{i:03d}.pt"), hr_latent=hr, lr_latent=lr, metadata={"name": str(i)})
            if split == "train":
                both = torch.cat([hr, lr]).double()
                s += both.sum(1)
                q += (both ** 2).sum(1)
                count += n
    with open(os.path.join(root, "global_stats_separated.json"), "w") as f:
        json.dump(final_stats(s, q, count, C_), f)
    return root


def fit_args(data_dir, base, *more):
    argv = ["--data-dir", data_dir, "--save-dir-base", base, "--preset", "micro", "--model", "v3", "--frames", str(FRAMES),
            "--batch-size", str(BATCH), "--epochs", "2", "--samples-per-epoch-multiplier", "1", "--save-interval-steps", "1",
            "--log-interval", "1", "--warmup-steps", "2", "--lr", "1e-3", "--seed", "7", "--grad-accum-steps", str(ACCUM)]
    return F.build_parser().parse_args(argv + list(more))


def read_log(folder):
    with open(os.path.join(folder, "train_log.jsonl")) as f:
        return [json.loads(line) for line in f]


def test_fit_with_two_micro_batches_per_step(tmp_path, capsys):
    data_dir = write_folder(str(tmp_path / "prepared"))
    args = fit_args(data_dir, str(tmp_path / "ck_full"))
    res = F.run(args)
    printed = capsys.readouterr().out
    n_batches = len(epoch_batches(len(TRAIN_LENGTHS), 1, BATCH, 0, 0, 1, True, args.seed))
    per_epoch = n_batches // ACCUM
    assert (n_batches, per_epoch) == (5, 2)
    assert printed.count("do not fill an optimiser step") == 1 and f"{per_epoch} steps per epoch" in printed
    steps = [r for r in read_log(res["save_dir"]) if "Train/Loss" in r]
    assert [(r["step"], r["epoch"]) for r in steps] == [(0, 0), (1, 0), (2, 1), (3, 1)]           # optimiser steps
    assert [r["Train/LR"] for r in steps] == [jatsr_amd.get_lr(g, 2 * per_epoch, 2, 1e-3) for g in range(4)]
    assert res["global_step"] == 4
    names = set(os.listdir(res["save_dir"]))
    assert {"last.pt", "interval_step_1.pt", "interval_step_2.pt", "interval_step_3.pt"} <= names
    ck = torch.load(os.path.join(res["save_dir"], "last.pt"), map_location="cpu", weights_only=False)
    assert ck["global_step"] == 4 and ck["fit_args"]["grad_accum_steps"] == ACCUM
    # the same run written out by hand: micro-batch calls, then the step
    store = LatentStore(data_dir, "train", FRAMES, "cuda")
    stats = jio.load_stats(os.path.join(data_dir, "global_stats_separated.json"), channels=C_, device="cuda")
    hand = F.build_trainer(args, F.build_model(args, "cuda"), per_epoch * args.epochs)
    assert hand.grad_accum_steps == ACCUM
    losses, term_means = [], []
    for epoch in range(args.epochs):
        batches = epoch_batches(len(store), 1, BATCH, epoch, 0, 1, True, args.seed)
        plans = [train_batch_plan(store.lengths, FRAMES, b, args.seed, epoch) for b in batches]
        for st in range(per_epoch):
            hand.accumulate_normalised(*store.batch(*plans[ACCUM * st], stats))
            losses.append(hand.step_normalised(*store.batch(*plans[ACCUM * st + 1], stats))["loss"])
            term_means.append(hand.loss_terms()["mse"])
    assert losses == [r["Train/Loss"] for r in steps]                   # floats compared exactly: bit for bit
    assert term_means == [r["Train/MSE_Loss"] for r in steps]
    assert torch.equal(hand.params, res["trainer"].params)
    # a resumed run continues bit for bit
    base = str(tmp_path / "ck_resume")
    first = F.run(fit_args(data_dir, base, "--max-steps", "2"))
    assert first["global_step"] == 2
    del first["trainer"]
    second = F.run(fit_args(data_dir, base, "--resume"))
    assert second["save_dir"] == first["save_dir"] and second["global_step"] == 4
    a, b = res["trainer"], second["trainer"]
    assert torch.equal(a.params, b.params) and torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq)
    assert [r for r in read_log(second["save_dir"]) if "Train/Loss" in r] == steps


def test_fit_rejects_a_count_below_one_before_any_workspace(tmp_path):
    with pytest.raises(SystemExit):
        fit_args("nowhere", str(tmp_path / "ck"), "--grad-accum-steps", "0")
    args = fit_args("nowhere", str(tmp_path / "ck"))
    args.grad_accum_steps = 0                       # a caller that builds the namespace itself
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with pytest.raises(ValueError, match="grad_accum_steps"):
        F.run(args)
    assert torch.cuda.memory_allocated() == before and not os.path.exists(str(tmp_path / "ck"))
