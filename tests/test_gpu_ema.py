"""The EMA of the weights on the GPU: the fused AdamW + EMA kernel through `jat_k_adamw_ema` (bit-identical p, m, v to
`jat_k_adamw`; the average against the fp64 twin of tests/ema_ref.py), the skipped step, argument rejections, the in-place
swap, and the layers above it: `Trainer(ema_decay=...)`, `ema_weights()`, checkpoints, `load_model(use_ema=...)`, `fit`.

Bounds.  The kernel forms e_new = fma(1 - d, p_new - e, e) in fp32; 1 - d is exact for the decays used (d = 0 or d >= 0.5).
Per element that is at most three roundings (the issue's count; the fma form makes two), each relative to a value no larger
than max(|p_new|, |e|): 3 * 2^-24 * max(|p_new|, |e0|) against the fp64 formula evaluated on the p_new the GPU produced, so
that AdamW's own rounding does not enter.  Over N updates the errors add (each later update scales an earlier error by
d <= 1): 3 * 2^-24 * S * N with S the largest |p| or |e| seen.  The decay handed to the C ABI is a float, so the fp64
recurrence uses the float value of `ema_decay_at`.

The fp16-operand library (tests/test_gpu_fp16.py runs a selection of this file on it): `make_trainer` of tests/test_gpu_train.py
gives a trainer without the dynamic scaler the fixed loss scale FP16_TEST_SCALE, and the fixture with the scaler on starts from
it too.  Nothing here compares a gradient with a reference, so the scale is nowhere divided out: the trainers whose bits
are compared run at the same one, and the fp64 recurrence is applied to the parameters the GPU produced.
"""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ema_ref as R  # noqa: E402
import jatsr_amd  # noqa: E402
import jatsr_amd._lib as L  # noqa: E402
import jatsr_amd.recipe as recipe  # noqa: E402
from helpers import load_golden  # noqa: E402
from jatsr_amd import fit as F  # noqa: E402
from test_gpu_fit import BATCH, TRAIN_LENGTHS, VAL_LENGTHS, fit_args, read_log, write_folder  # noqa: E402
from test_gpu_train import FP16, FP16_TEST_SCALE, cuda, make_trainer, step_inputs  # noqa: E402
from test_gpu_train_kernels import F32, call, dev, gen, guarded, guards_intact, work  # noqa: E402

HYPER = (1e-3, 0.9, 0.999, 1e-8, 0.01)     # lr, beta1, beta2, eps, weight decay: those of test_adamw
EMA_KEYS = ("ema_state_dict", "ema_decay", "ema_warmup", "ema_updates")


def bits(x):
    return x.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def f32(x):
    return float(np.float32(x))


# ---------------------------------------------------------------------------------------------------------------------
# 1. the fused kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decay", [0.0, 0.999, 0.9999])
@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("step", [1, 7])
@pytest.mark.parametrize("n", [4, 1028, 1_000_004])     # one thread; a partial block; many blocks with a ragged last one
def test_fused_adamw_ema_kernel(n, step, clip, decay):
    ls = 1024.0
    lr, b1, b2, eps, wd = HYPER
    p0, g0 = gen((n,), 70), gen((n,), 71, 0.01 * ls)
    m0, v0 = gen((n,), 72, 1e-3), gen((n,), 73, 1e-3).abs() * 1e-2
    e0 = gen((n,), 74, 1.5, 0.25)                       # independent of p0
    norm = float((g0.double() / ls).norm())
    max_norm = 0.5 * norm if clip else 2.0 * norm
    wk = work((1024 + 2) * 4)
    # the shipped launch on the same inputs
    p1, m1, v1 = p0.clone(), m0.clone(), v0.clone()
    n1 = torch.zeros(1, device=dev())
    call(L.lib().jat_k_adamw, L.ptr(p1), L.ptr(g0), L.ptr(m1), L.ptr(v1), n, lr, b1, b2, eps, wd, max_norm, ls, step, L.ptr(n1),
         L.ptr(wk), wk.numel() * 4, L.stream_ptr())
    assert not torch.equal(p1, p0)
    pb, p = guarded((n,), fill=p0)
    gb, g = guarded((n,), fill=g0)
    mb, m = guarded((n,), fill=m0)
    vb, v = guarded((n,), fill=v0)
    eb, e = guarded((n,), fill=e0)
    nb, nrm = guarded((1,))
    call(L.lib().jat_k_adamw_ema, L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), L.ptr(e), n, lr, b1, b2, eps, wd, max_norm, ls, decay,
         step, L.ptr(nrm), L.ptr(wk), wk.numel() * 4, L.stream_ptr())
    assert same_bits(p, p1) and same_bits(m, m1) and same_bits(v, v1) and same_bits(nrm, n1), "the EMA perturbed AdamW"
    assert same_bits(g, g0)
    pn, en, e0n = p.cpu().numpy().astype(np.float64), e.cpu().numpy().astype(np.float64), e0.cpu().numpy().astype(np.float64)
    ref = R.ema_update(e0n, pn, f32(decay))
    err = np.abs(en - ref)
    bound = 3 * F32 * np.maximum(np.abs(pn), np.abs(e0n))
    print(f"n={n} step={step} clip={clip} decay={decay}: worst ema error / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all(), f"ema off by {float((err / bound).max()):.2f} bounds"
    if decay > 0:
        assert not torch.equal(e, p) and not torch.equal(e, e0)
    # and the whole step agrees with the fp64 twin at the tolerance test_adamw gives p (1e-5 of the magnitudes involved)
    tw = R.adamw_ema_step(p0.cpu().numpy(), g0.cpu().numpy(), m0.cpu().numpy(), v0.cpu().numpy(), e0n, f32(lr), f32(b1), f32(b2),
                          f32(eps), f32(wd), f32(max_norm), ls, step, f32(decay))
    assert np.abs(en - tw["e"]).max() <= 1e-5 * (np.abs(e0n).max() + np.abs(pn).max())
    assert all(guards_intact(x) for x in (pb, gb, mb, vb, eb, nb))


# ---------------------------------------------------------------------------------------------------------------------
# 2. a skipped step leaves the average alone
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_non_finite_gradient_leaves_ema_untouched(bad):
    n = 1028
    p0, m0, v0, e0 = gen((n,), 80), gen((n,), 81, 1e-3), gen((n,), 82, 1e-3).abs(), gen((n,), 84)
    g = gen((n,), 83)
    g[517] = bad
    p, m, v, e = p0.clone(), m0.clone(), v0.clone(), e0.clone()
    nrm = torch.zeros(1, device=p.device)
    wk = work((1024 + 2) * 4)
    call(L.lib().jat_k_adamw_ema, L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), L.ptr(e), n, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1.0, 1.0, 0.999,
         3, L.ptr(nrm), L.ptr(wk), wk.numel() * 4, L.stream_ptr())
    assert same_bits(e, e0) and same_bits(p, p0) and same_bits(m, m0) and same_bits(v, v0)
    assert not math.isfinite(float(nrm[0]))


# ---------------------------------------------------------------------------------------------------------------------
# 3. rejections
# ---------------------------------------------------------------------------------------------------------------------
def micro(**kw):
    _, meta = load_golden("train_micro_T24")
    return (meta,) + make_trainer(meta, condition_noise_ratio=0.0, **kw)


def test_rejections_launch_nothing():
    lib, s = L.lib(), L.stream_ptr()
    f = torch.zeros(1 << 12, device=dev())
    wk = work(1 << 13)
    P, WB = L.ptr(f), wk.numel() * 4
    args = (1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 1.0)

    def rejected(rc):
        assert rc == L.JAT_E_INVALID
        with pytest.raises(ValueError):
            L.check(rc)
    q = [ctypes.c_void_p(f.data_ptr() + 64 * i) for i in range(5)]      # five buffers of their own: p, g, m, v, ema
    assert lib.jat_k_adamw_ema(*q, 8, *args, 0.9, 1, None, L.ptr(wk), WB, s) == L.JAT_OK     # the control: these are accepted (all zero: stays zero)
    rejected(lib.jat_k_adamw_ema(*q[:4], None, 8, *args, 0.9, 1, None, L.ptr(wk), WB, s))
    for decay in (1.0, -0.1, float("nan")):
        rejected(lib.jat_k_adamw_ema(*q, 8, *args, decay, 1, None, L.ptr(wk), WB, s))
    rejected(lib.jat_k_adamw_ema(*q, 6, *args, 0.9, 1, None, L.ptr(wk), WB, s))
    for alias in range(4):                                              # ema must not be one of p, g, m, v
        rejected(lib.jat_k_adamw_ema(*q[:4], q[alias], 8, *args, 0.9, 1, None, L.ptr(wk), WB, s))
    torch.cuda.synchronize()
    assert bool((f == 0).all())
    meta, m, tr = micro(use_grad_scaler=False)
    before = tr.params.clone()
    assert lib.jat_trainer_swap_ema(tr.ptr, s) == L.JAT_E_STATE
    for decay in (1.0, -0.1, float("nan")):
        rejected(lib.jat_trainer_set_ema(tr.ptr, L.ptr(f), decay))
    assert lib.jat_trainer_swap_ema(tr.ptr, s) == L.JAT_E_STATE          # a rejected set_ema set nothing
    torch.cuda.synchronize()
    assert same_bits(tr.params, before)
    with pytest.raises(L.JatError):
        with tr.ema_weights():
            pass
    with pytest.raises(L.JatError):
        tr.ema_state_dict()
    with pytest.raises(ValueError):
        micro(ema_decay=1.0)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the swap
# ---------------------------------------------------------------------------------------------------------------------
def test_swap_exchanges_and_restores():
    meta, m, tr = micro(use_grad_scaler=False, ema_decay=0.99)
    assert same_bits(tr.ema, tr.params) and tr.ema.data_ptr() != tr.params.data_ptr()
    tr.ema.copy_(gen((tr.ema.numel(),), 90))
    p0, e0 = tr.params.clone(), tr.ema.clone()
    call(L.lib().jat_trainer_swap_ema, tr.ptr, L.stream_ptr())
    assert same_bits(tr.params, e0) and same_bits(tr.ema, p0)
    call(L.lib().jat_trainer_swap_ema, tr.ptr, L.stream_ptr())
    assert same_bits(tr.params, p0) and same_bits(tr.ema, e0)


# ---------------------------------------------------------------------------------------------------------------------
# 5. Trainer: six steps, one of them skipped, beside a twin without the average
# ---------------------------------------------------------------------------------------------------------------------
LR = 1e-2          # large enough for the weights to move visibly in a handful of steps
BAD_STEP = 2


def run_steps(tr, meta, steps, first=0, record=None):
    """Steps first .. first + steps - 1 of a fixed sequence: injected t / noise / mask, mask seed = step index; step BAD_STEP
    gets a non-finite target, as test_skipped_step_advances_the_schedule_counter_not_adamw makes one."""
    hr, lr, noise, t, mask = step_inputs(meta)
    z_t, t2, cond = tr.prepare(hr, lr, noise=noise, cfg_mask=mask, t=t)
    bad = hr.clone()
    bad[0, 0, 0] = float("inf")
    for i in range(first, first + steps):
        tr.forward_backward(z_t, t2, cond, bad if i == BAD_STEP else hr, mask_seed=1000 + i)
        _, gn = tr.optimizer_step(lr=LR)
        if record is not None:
            record(i, gn)
    return z_t, t2, cond


@pytest.fixture(scope="module")
def six_steps():
    meta, m, tr = micro(use_grad_scaler=True, ema_decay=0.99, seed=5)
    _, m0, tr0 = micro(use_grad_scaler=True, seed=5)
    if FP16:          # the fp16-operand library: the dynamic scaler stays on, from a start that fp16 gradients do not overflow at
        tr.scaler.scale = tr0.scaler.scale = FP16_TEST_SCALE
    assert tr0.ema is None and same_bits(tr.params, tr0.params) and same_bits(tr.ema, tr.params)
    e = tr.ema.double().cpu().numpy()
    state = dict(e=e, S=float(np.abs(e).max()), N=0, skipped=[])

    def record(i, gn):
        p = tr.params.double().cpu().numpy()
        state["S"] = max(state["S"], float(np.abs(p).max()))
        if math.isfinite(gn):
            state["N"] += 1
            state["e"] = R.ema_update(state["e"], p, f32(R.ema_decay_at(state["N"], 0.99, True)))
            state["S"] = max(state["S"], float(np.abs(state["e"]).max()))
        else:
            state["skipped"].append(i)
    inputs = run_steps(tr, meta, 6, record=record)
    run_steps(tr0, meta, 6)
    return dict(meta=meta, m=m, tr=tr, tr0=tr0, inputs=inputs, **state)


def test_trainer_ema_follows_the_fp64_recurrence_and_does_not_perturb_training(six_steps):
    s = six_steps
    tr, tr0 = s["tr"], s["tr0"]
    assert s["skipped"] == [BAD_STEP] and s["N"] == 5
    assert tr.ema_updates == tr.opt_step == 5 and tr.global_step == 6
    assert (tr0.opt_step, tr0.global_step, tr0.ema_updates, tr0.scaler.scale) == (5, 6, 0, tr.scaler.scale)
    err = np.abs(tr.ema.double().cpu().numpy() - s["e"])
    bound = 3 * F32 * s["S"] * s["N"]
    print(f"trainer ema: worst error {err.max():.3e}, bound {bound:.3e} (S {s['S']:.3f}, N {s['N']})")
    assert err.max() <= bound
    assert float((tr.ema - tr.params).abs().max()) > 1e-3          # the average is not the last iterate
    assert same_bits(tr.params, tr0.params) and same_bits(tr.exp_avg, tr0.exp_avg) and same_bits(tr.exp_avg_sq, tr0.exp_avg_sq)


# ---------------------------------------------------------------------------------------------------------------------
# 5b. the average across steps the arithmetic itself skips
# ---------------------------------------------------------------------------------------------------------------------
def test_average_across_real_overflow_skips():
    """The loss scaler's skips made by the arithmetic, not by a planted inf: fp16 operands above 65504 at a 2^30 loss scale (the
    fp16 library; the bf16 one overflows nowhere at 2^16 and must take every step).  Until four steps are taken: a skipped step
    leaves the average bit for bit alone and does not count as an update; the average is the fp64 recurrence over the
    parameter snapshots of the taken steps alone, within 3 * 2^-24 * S per update (the bound of section 5)."""
    fp16 = L.operand_dtype() == "fp16"
    meta = dict(cfg="micro", norm="rms", salt=95, B=2, T=24, lr=1e-4, wd=0.1, clip=1.0)
    m, tr = make_trainer(meta, use_grad_scaler=True, condition_noise_ratio=0.0, ema_decay=0.99)
    tr.scaler.scale = 2.0 ** 30 if fp16 else 65536.0
    Cc = recipe.CONFIGS["micro"]["input_channels"]
    z_t, cond, target = (cuda(recipe.gaussian(n, (2, Cc, 24), 95 + i)) for i, n in enumerate(("zt", "cond", "target")))
    t = cuda(np.asarray([0.2, 0.8], np.float32))
    # the overflow skips all come before the first taken step, while a fresh average still equals the weights and an update on a
    # skipped step would change nothing: start from an average that is not the weights
    tr.ema.mul_(0.75)
    assert not same_bits(tr.ema, tr.params)
    e = tr.ema.double().cpu().numpy()
    S, N, skipped = float(np.abs(e).max()), 0, 0
    for step in range(40):
        if tr.opt_step == 4:
            break
        e0, s0 = tr.ema.clone(), tr.scaler.scale
        tr.forward_backward(z_t, t, cond, target)
        _, gn = tr.optimizer_step(lr=LR)
        if math.isfinite(gn):
            N += 1
            p = tr.params.double().cpu().numpy()
            e = R.ema_update(e, p, f32(R.ema_decay_at(N, 0.99, True)))
            S = max(S, float(np.abs(p).max()), float(np.abs(e).max()))
            assert tr.scaler.scale == s0 and not same_bits(tr.ema, e0)
        else:
            skipped += 1
            assert same_bits(tr.ema, e0) and tr.scaler.scale == s0 * 0.5
        assert tr.ema_updates == tr.opt_step == N and tr.global_step == N + skipped
    assert tr.ema_updates == tr.opt_step == N == 4
    err = np.abs(tr.ema.double().cpu().numpy() - e)
    bound = 3 * F32 * S * N
    print(f"{'fp16' if fp16 else 'bf16'}: {skipped} skipped, 4 taken; worst ema error {err.max():.3e}, bound {bound:.3e} (S {S:.3f})")
    assert err.max() <= bound
    assert float((tr.ema - tr.params).abs().max()) > 1e-3          # the average is not the last iterate
    if fp16:
        assert skipped >= 1, "a 2^30 loss scale must overflow fp16 operands at least once"
    else:
        assert skipped == 0


# ---------------------------------------------------------------------------------------------------------------------
# 6. ema_weights()
# ---------------------------------------------------------------------------------------------------------------------
def fresh_model(like, meta, sd):
    m2 = type(like)(**recipe.CONFIGS[meta["cfg"]], dropout=0.0, drop_path_rate=0.0)
    missing, unexpected = m2.load_state_dict(sd, strict=False)
    assert not unexpected
    return m2.to("cuda").eval()


def test_ema_weights_context(six_steps):
    s = six_steps
    meta, m, tr = s["meta"], s["m"], s["tr"]
    z_t, t2, cond = s["inputs"]
    hr, lr, noise, _, _ = step_inputs(meta)
    B, C, T = hr.shape
    m.eval()
    out_raw = m(z_t, t2, cond)
    p0, e0 = tr.params.clone(), tr.ema.clone()
    esd = tr.ema_state_dict()
    assert list(esd) == list(m.state_dict()) and all(v.device.type == "cpu" and v.dtype == torch.float32 for v in esd.values())
    assert all(esd[k].shape == v.shape for k, v in m.state_dict().items())
    held = jatsr_amd.Sampler(m, B, T, 4, 3.0)
    raw_sample = held.run(lr, noise)
    with tr.ema_weights():
        out_ema = m(z_t, t2, cond)
        assert same_bits(tr.params, e0) and same_bits(tr.ema, p0)
        inside_sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
        assert all(torch.equal(inside_sd[k], esd[k]) for k in esd)                    # model.state_dict() sees the average
        assert all(torch.equal(v, esd[k]) for k, v in tr.ema_state_dict().items())    # and ema_state_dict() still reads it
        for call_ in (lambda: tr.optimizer_step(lr=LR), lambda: tr.forward_backward(z_t, t2, cond, hr),
                      lambda: tr.load_checkpoint(dict(model_state_dict={})), lambda: tr.save_checkpoint(os.devnull)):
            with pytest.raises(L.JatError):
                call_()
        inside_sample = jatsr_amd.Sampler(m, B, T, 4, 3.0).run(lr, noise)
        held_inside = held.run(lr, noise)                                             # a held sampler is rebuilt (epoch bump)
    assert same_bits(out_ema, fresh_model(m, meta, esd)(z_t, t2, cond))
    assert not torch.equal(out_ema, out_raw)
    assert same_bits(tr.params, p0) and same_bits(tr.ema, e0)
    assert same_bits(m(z_t, t2, cond), out_raw)
    after_sample = jatsr_amd.Sampler(m, B, T, 4, 3.0).run(lr, noise)
    assert not torch.equal(inside_sample, after_sample)
    assert same_bits(after_sample, raw_sample) and same_bits(held_inside, inside_sample) and same_bits(held.run(lr, noise), raw_sample)
    # the trainer steps on as if nothing had happened: same bits as the twin that never swapped
    tr0 = s["tr0"]
    for x in (tr, tr0):
        x.forward_backward(z_t, t2, cond, hr, mask_seed=77)
        x.optimizer_step(lr=LR)
    assert same_bits(tr.params, tr0.params) and same_bits(tr.grads, tr0.grads)


# ---------------------------------------------------------------------------------------------------------------------
# 7. checkpoints and load_model
# ---------------------------------------------------------------------------------------------------------------------
def test_checkpoint_roundtrip_and_load_model(tmp_path):
    kw = dict(use_grad_scaler=True, ema_decay=0.99, seed=5)
    meta, ma, a = micro(**kw)
    run_steps(a, meta, 5)                                   # uninterrupted; step BAD_STEP is skipped in both runs
    _, mb, b = micro(**kw)
    run_steps(b, meta, 3)
    path = str(tmp_path / "ema.pt")
    ck = b.save_checkpoint(path, epoch=2)
    assert all(k in ck for k in EMA_KEYS) and (ck["ema_decay"], ck["ema_warmup"], ck["ema_updates"]) == (0.99, True, 2)
    assert list(ck["ema_state_dict"]) == list(ck["model_state_dict"])
    # different initial weights, decay and warm-up: the stored ones replace them
    mc, c = make_trainer(dict(meta, salt=meta["salt"] + 9), condition_noise_ratio=0.0, **dict(kw, ema_decay=0.5, ema_warmup=False))
    assert c.load_checkpoint(path) == 2
    assert (c.ema_decay, c.ema_warmup) == (0.99, True)
    assert c.ema_updates == 2 and same_bits(c.ema, b.ema) and same_bits(c.params, b.params)
    run_steps(c, meta, 2, first=3)
    assert c.ema_updates == a.ema_updates == 4 and c.opt_step == a.opt_step == 4
    assert same_bits(c.ema, a.ema) and same_bits(c.params, a.params)
    # a checkpoint written without the average: the average starts from the loaded weights
    _, mn, n = micro(use_grad_scaler=True, seed=5)
    run_steps(n, meta, 2)
    plain = str(tmp_path / "plain.pt")
    ckn = n.save_checkpoint(plain)
    assert not any(k in ckn for k in EMA_KEYS)
    c.load_checkpoint(plain)
    assert c.ema_updates == 0 and same_bits(c.ema, c.params) and same_bits(c.params, n.params)
    # ... and warms up from its own first update (2/11), although the restored optimiser is at step 3
    assert c.opt_step == 2
    e_old = c.ema.double().cpu().numpy()
    run_steps(c, meta, 1, first=3)
    p_new, e_new = c.params.double().cpu().numpy(), c.ema.double().cpu().numpy()
    err = np.abs(e_new - R.ema_update(e_old, p_new, f32(R.ema_decay_at(1, 0.99, True))))
    assert (err <= 3 * F32 * np.maximum(np.abs(p_new), np.abs(e_old))).all() and c.ema_updates == 1
    assert np.abs(e_new - R.ema_update(e_old, p_new, f32(R.ema_decay_at(3, 0.99, True)))).max() > 1e-4      # not the step-3 decay
    with pytest.warns(UserWarning, match="moving average"):       # a trainer without one ignores the keys, and says so
        assert n.load_checkpoint(path) == 2
    assert n.ema is None and same_bits(n.params, b.params)
    # load_model
    esd = b.ema_state_dict()
    me = jatsr_amd.load_model(path, cls=type(mb), use_ema=True)
    mr = jatsr_amd.load_model(path, cls=type(mb), use_ema=False)
    assert me.load_info["weights"] == "ema" and mr.load_info["weights"] == "raw"
    assert jatsr_amd.load_model(path, cls=type(mb)).load_info["weights"] == "raw"
    raw = dict(mb.named_parameters())
    differ = 0
    for k, p in me.named_parameters():
        assert torch.equal(p.data.cpu(), esd[k]), k
        assert torch.equal(dict(mr.named_parameters())[k].data, raw[k].data), k
        differ += int(not torch.equal(p.data, raw[k].data))
    assert differ > 0
    with pytest.raises(KeyError, match="ema_state_dict"):
        jatsr_amd.load_model(plain, cls=type(mb), use_ema=True)


# ---------------------------------------------------------------------------------------------------------------------
# 8. fit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fit_runs(tmp_path_factory):
    data = write_folder(str(tmp_path_factory.mktemp("prepared_ema")), TRAIN_LENGTHS, VAL_LENGTHS)
    base_e, base_p = str(tmp_path_factory.mktemp("ck_ema")), str(tmp_path_factory.mktemp("ck_plain"))
    first = F.run(fit_args(data, base_e, "--ema-decay", "0.9", "--max-steps", "4"))
    ck_first = torch.load(os.path.join(first["save_dir"], "last.pt"), map_location="cpu", weights_only=False)
    del first["trainer"]
    second = F.run(fit_args(data, base_e, "--ema-decay", "0.9", "--resume"))
    plain = F.run(fit_args(data, base_p, "--max-steps", "4"))
    return dict(first=first, ck_first=ck_first, second=second, plain=plain)


def test_fit_with_ema(fit_runs):
    first, second, plain, ck = (fit_runs[k] for k in ("first", "second", "plain", "ck_first"))
    per_epoch = len(TRAIN_LENGTHS) // BATCH
    assert first["global_step"] == per_epoch == 4 and second["global_step"] == 8 and second["save_dir"] == first["save_dir"]
    taken = int(float(ck["optimizer_state_dict"]["state"][0]["step"]))      # optimiser steps not skipped by the loss scaler
    assert all(k in ck for k in EMA_KEYS) and (ck["ema_decay"], ck["ema_warmup"], ck["ema_updates"]) == (0.9, True, taken)
    assert 0 < taken <= 4
    for name in ("last.pt", "best.pt", "interval_step_2.pt", "interval_step_6.pt"):
        c = torch.load(os.path.join(second["save_dir"], name), map_location="cpu", weights_only=False)
        assert all(k in c for k in EMA_KEYS), name
        assert list(c["ema_state_dict"]) == list(c["model_state_dict"])
    tr = second["trainer"]
    assert tr.ema_updates == tr.opt_step > taken                # the stored count plus the resumed run's own steps
    log = read_log(second["save_dir"])
    vals = [r for r in log if "Val/Loss" in r]
    assert [r["epoch"] for r in vals] == [0, 1]
    for r in vals:
        for k in ("Val/EMA_Loss", "Val/EMA_LatentPerc_TotalLoss", "Val/EMA_LatentPerc_FreqLoss", "Val/Loss", "Val/Loss_Std",
                  "Val/MSE_Loss", "Val/LatentPerc_TotalLoss"):
            assert isinstance(r[k], float) and math.isfinite(r[k]), (k, r)
        assert r["Val/EMA_Loss"] > 0 and r["Val/EMA_Loss"] != r["Val/Loss"]
    assert second["best_val_loss"] == min(r["Val/Loss"] for r in vals)      # best.pt is chosen by the raw loss
    # the raw tags are what a run without the flag logs, bit for bit: the average and its validation perturb nothing
    plain_log = read_log(plain["save_dir"])

    def strip(r):
        return {k: v for k, v in r.items() if "EMA" not in k}
    assert [r for r in plain_log if "Train/Loss" in r] == [r for r in log if "Train/Loss" in r][:4]
    assert [r for r in plain_log if "Val/Loss" in r] == [strip(vals[0])]
    assert not any("EMA" in k for r in plain_log for k in r)
    for name in ("last.pt", "interval_step_2.pt"):
        c = torch.load(os.path.join(plain["save_dir"], name), map_location="cpu", weights_only=False)
        assert not any(k in c for k in EMA_KEYS), name
    assert plain["trainer"].ema is None
