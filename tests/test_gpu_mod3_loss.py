"""The V3-MOD3 loss (train_ddp_v3mod3.py:955-969: rw * Charbonnier-or-MSE + lw * latent perceptual loss) on every launch path of the
latent loss kernels, through `jat_k_latent_loss_ex`, against the fp64 twin tests/mod3_loss_ref.py (pinned to the reference's own
functions by tests/test_mod3_cpu.py).

The reconstruction term lives in the general instances of the kernels of tests/test_gpu_loss_paths.py (csrc/train.hip:
latent_loss_kernel<FB, NB, LatentLossArgsEx>, latent_loss_fft_kernel<LatentLossArgsEx>, latent_loss_finish_kernel<...>), so the
lengths, the inputs and their preconditions (tests/loss_path_cases.py), the guarded NaN arenas and the gates are that file's: every
term within 2e-5 relative, d total / d pred within rel-L2 2e-4 for the tensor and for every row alone.  Charbonnier adds no kink
(sqrt(e^2 + eps) is smooth for eps > 0), and an fp32 evaluation of it on these inputs is within 1.1e-7 (value) / 5.2e-8 (per-row
gradient) of fp64, so the gates need no widening.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import jatsr_amd._lib as L  # noqa: E402
import loss_path_cases as K  # noqa: E402
import mod3_loss_ref as M3  # noqa: E402
from helpers import rel_l2  # noqa: E402

TERM_TOL, DPRED_TOL = 2e-5, 2e-4
GUARD = 64
NAN = float("nan")
EPS = 1e-6                                    # train_ddp_v3mod3.py:409
ALL_T = [T for T, _, _ in K.LENGTHS + K.EXTRA]


def guarded(shape, fill=None):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), NAN, dtype=torch.float32, device="cuda")
    view = buf[GUARD:GUARD + n].view(shape)
    if fill is not None:
        view.copy_(fill)
    return buf, view


def guards_intact(buf):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())


def work_bytes(T, rows):
    return (T * 8 + 255) // 256 * 256 + rows * 32        # include/jat_hip.h: the rule of jat_k_latent_loss


@functools.lru_cache(maxsize=None)
def case_inputs(T):
    x = K.make_inputs(T, K.SALT[T])
    pre = K.preconditions(*x)
    assert K.preconditions_hold(pre), f"T = {T}: the inputs miss the preconditions {pre} (bounds {K.PRE_BOUNDS})"
    for a in x:
        a.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _reference(T, eps, rw, weights):
    """fp64 twin on the inputs of length T, once per setting, shared read-only."""
    terms, dpred = M3.mod3_loss(*case_inputs(T), recon_eps=eps, recon_weight=rw, **dict(weights), **K.CUTS)
    dpred = dpred[0]
    dpred.setflags(write=False)
    return terms, dpred


def reference(T, eps, rw, weights=None):
    return _reference(T, eps, rw, tuple(sorted((weights or K.WEIGHTS).items())))


class Run:
    """One call of jat_k_latent_loss_ex (or, ex=False, jat_k_latent_loss) on the inputs of length T inside guarded arenas."""

    def __init__(self, T, eps=EPS, rw=1.0, weights=None, loss_scale=1.0, with_lr=True, work_short=0, rows_T=None, ex=True):
        L.require_gpu()
        w = dict(weights or K.WEIGHTS)
        if rows_T is None:
            x = case_inputs(T)
            self.rows = x[0].shape[1]
            self.inputs = [guarded((self.rows, T), torch.tensor(a[0], device="cuda")) for a in x]
        else:                                   # a shape no kernel takes: nothing is read
            self.rows = rows_T
            self.inputs = [guarded((self.rows, T), torch.zeros(self.rows, T, device="cuda")) for _ in range(3)]
        self.T, self.ex = T, ex
        self.dbuf, self.dpred = guarded((self.rows, T))
        self.obuf, self.out6 = guarded((6,))
        nwork = work_bytes(T, self.rows) - work_short
        self.wbuf = torch.full((nwork + 2 * GUARD * 4,), 0xFF, dtype=torch.uint8, device="cuda")
        head = (L.ptr(self.inputs[0][1]), L.ptr(self.inputs[1][1]), L.ptr(self.inputs[2][1]) if with_lr else None,
                L.ptr(self.dpred), L.ptr(self.out6), self.rows, T)
        tail = (w["latent_weight"], w["freq_weight"], w["ms_weight"], w["consistency_weight"], K.CUTS["low_freq_phase_ratio"],
                K.CUTS["strict_cutoff"], K.CUTS["soft_cutoff"], loss_scale, C.c_void_p(self.wbuf.data_ptr() + GUARD * 4), nwork,
                L.stream_ptr())
        self.args = head + ((eps, rw) if ex else ()) + tail

    def call(self):
        rc = (L.lib().jat_k_latent_loss_ex if self.ex else L.lib().jat_k_latent_loss)(*self.args)
        torch.cuda.synchronize()
        return rc

    def guards_ok(self):
        w = self.wbuf
        return (guards_intact(self.dbuf) and guards_intact(self.obuf) and bool((w[:GUARD * 4] == 0xFF).all())
                and bool((w[-GUARD * 4:] == 0xFF).all()) and all(guards_intact(b) for b, _ in self.inputs))

    def untouched(self):
        return bool(torch.isnan(self.dbuf).all()) and bool(torch.isnan(self.obuf).all()) and bool((self.wbuf == 0xFF).all())


def run_and_check(T, label, eps=EPS, rw=1.0, weights=None, loss_scale=1.0):
    """-> (out6 as a dict of python floats, dpred / loss_scale as fp32 numpy) after the checks every case gets."""
    terms_ref, dp_ref = reference(T, eps, rw, weights)
    r = Run(T, eps, rw, weights, loss_scale)
    L.check(r.call())
    out_a, dp_a = r.out6.clone(), r.dpred.clone()
    assert r.guards_ok(), f"{label}: a guard band was written"
    assert bool(torch.isfinite(dp_a).all()) and bool(torch.isfinite(out_a).all()), f"{label}: non-finite output"
    got = dict(zip(M3.TERMS, out_a.double().tolist()))
    dp = dp_a.cpu().numpy() / np.float32(loss_scale)
    term_err = {k: abs(got[k] - terms_ref[k]) / abs(terms_ref[k]) if terms_ref[k] != 0 else (0.0 if got[k] == 0 else np.inf)
                for k in M3.TERMS}
    whole = rel_l2(dp, dp_ref)
    per_row = [rel_l2(dp[i], dp_ref[i]) for i in range(dp.shape[0])]
    print(f"{label}: worst term {max(term_err, key=term_err.get)} {max(term_err.values()):.2e} (gate {TERM_TOL:.0e}); dpred rel-L2 "
          f"whole {whole:.2e}, rows {' '.join(f'{v:.2e}' for v in per_row)} (gate {DPRED_TOL:.0e})")
    for k, v in term_err.items():
        assert v <= TERM_TOL, f"{label}: {k} = {got[k]!r} vs {terms_ref[k]!r} (rel {v:.3e})"
    assert whole <= DPRED_TOL, f"{label}: dpred rel-L2 {whole:.3e}"
    for i, v in enumerate(per_row):      # a row the twin gives as exactly zero must be exactly zero: rel_l2 divides by 1e-30
        assert v <= DPRED_TOL, f"{label}: row {i} dpred rel-L2 {v:.3e}"
    return got, dp


@pytest.mark.parametrize("T", ALL_T)
def test_reference_settings_on_every_launch_path(T):
    """eps = 1e-6, rw = 1, the reference's weights, at every length of the table: every launch path and both chunk loops.  The tie
    row (pred == target): the reconstruction term gives it e / sqrt(e^2 + eps) = 0 exactly and every L1 term sign(0) = 0; the one
    thing that moves it is the consistency term, which compares the prediction with the clean LR row, not with the target (as
    tests/test_gpu_loss_paths.py notes).  So the row is exactly zero wherever the twin's is (empty bands), and exactly zero at EVERY
    length in a second call without the consistency term (cw = 0, no LR tensor)."""
    got, dp = run_and_check(T, f"T={T}")
    _, dp_ref = reference(T, EPS, 1.0)
    if not dp_ref[K.TIE].any():
        assert not dp[K.TIE].any()
    r = Run(T, EPS, 1.0, dict(K.WEIGHTS, consistency_weight=0.0), with_lr=False)
    L.check(r.call())
    assert r.guards_ok() and bool(torch.isfinite(r.dpred).all())
    assert not bool(r.dpred[K.TIE].any()), f"T={T}: the tie row moved without a consistency term"
    assert float(r.out6[4]) == 0.0


@pytest.mark.parametrize("T", K.SWEEP_T)
def test_eps_and_weight_sweep(T):
    """eps in {1e-12, 1e-2} x rw in {0, 0.25, 4}, and MSE (eps = 0) with rw = 0.25, on a factored, a direct and a chunked direct
    length; the loss scale does not reach the terms."""
    lw32 = float(np.float32(K.WEIGHTS["latent_weight"]))
    for eps in (1e-12, 1e-2):
        for rw in (0.0, 0.25, 4.0):
            got, _ = run_and_check(T, f"T={T} eps={eps:g} rw={rw:g}", eps=eps, rw=rw)
            if rw == 0.0:
                # out[0] = fp32(lw * latent), out[5] = fp32(latent): two roundings apart, 2 * 2^-24 relative
                assert abs(got["total"] - lw32 * got["latent"]) <= 2.0 ** -23 * abs(got["total"]), got
                assert got["mse"] > 0         # slot 1 is still the reconstruction mean (gated against the twin above)
    run_and_check(T, f"T={T} mse rw=0.25", eps=0.0, rw=0.25)
    base, _ = run_and_check(T, f"T={T} base", eps=EPS, rw=0.25)
    for scale in (2.0 ** -3, 1024.0):
        got, _ = run_and_check(T, f"T={T} loss_scale={scale}", eps=EPS, rw=0.25, loss_scale=scale)
        assert got == base, (scale, got, base)


@pytest.mark.parametrize("T", (35, 257, 521, 1543))
def test_default_reconstruction_is_jat_k_latent_loss_bit_for_bit(T):
    """eps = 0, rw = 1 goes to the instances jat_k_latent_loss runs: dpred and all six terms carry the same bits (one length per
    path class: factored, direct <1,2>, <2,4>, <3,6>)."""
    a, b = Run(T, 0.0, 1.0, ex=True), Run(T, ex=False)
    L.check(a.call())
    L.check(b.call())
    assert a.guards_ok() and b.guards_ok()
    assert bool(torch.isfinite(a.dpred).all())
    assert torch.equal(a.dpred, b.dpred) and torch.equal(a.out6, b.out6)


@pytest.mark.parametrize("T", (35, 521))
def test_latent_weight_zero_is_the_plain_charbonnier_kernel(T):
    """lw = 0, eps = 1e-6: what is left is charbonnier_grad_kernel's expression on another thread layout: dpred within rel-L2 1e-6
    of jat_k_recon_loss (the same fp32 statements: e, sqrt, divide, one product each), the loss within 2e-6 relative (a different
    summation order over rows * T <= 3126 terms)."""
    r = Run(T, EPS, 1.0, dict(K.WEIGHTS, latent_weight=0.0))
    L.check(r.call())
    assert r.guards_ok()
    pred, target = r.inputs[0][1], r.inputs[1][1]
    dref = torch.empty_like(pred)
    loss = torch.zeros(1, device="cuda")
    work = torch.empty(4104, dtype=torch.uint8, device="cuda")
    L.check(L.lib().jat_k_recon_loss(L.ptr(pred), L.ptr(target), L.ptr(dref), L.ptr(loss), pred.numel(), EPS, 1.0, L.ptr(work),
                                     work.numel(), L.stream_ptr()))
    torch.cuda.synchronize()
    d = rel_l2(r.dpred.cpu().numpy(), dref.cpu().numpy())
    rows = [rel_l2(r.dpred[i].cpu().numpy(), dref[i].cpu().numpy()) for i in range(r.rows)]
    lv, lref = float(r.out6[0]), float(loss[0])
    print(f"T={T} lw=0: dpred rel-L2 {d:.2e} rows {' '.join(f'{v:.2e}' for v in rows)} (gate 1e-6); loss {lv!r} vs {lref!r} "
          f"rel {abs(lv - lref) / lref:.2e} (gate 2e-6)")
    assert d <= 1e-6 and max(rows) <= 1e-6
    assert abs(lv - lref) <= 2e-6 * lref and float(r.out6[1]) == lv


def test_two_identical_calls_give_the_same_bits():
    r = Run(1378)
    L.check(r.call())
    dp, out = r.dpred.clone(), r.out6.clone()
    r.dpred.fill_(NAN)
    r.out6.fill_(NAN)
    L.check(r.call())
    assert bool(torch.isfinite(dp).all()) and torch.equal(r.dpred, dp) and torch.equal(r.out6, out) and r.guards_ok()


def test_rejections_launch_nothing():
    """A negative or NaN eps, a NaN weight, a length whose LDS image does not fit, a work buffer one byte short: an error code,
    `jat_last_error()` says why, and nothing was written to the outputs or the scratch."""
    lib = L.lib()
    cases = [("negative eps", Run(35, eps=-1e-6), L.JAT_E_INVALID, "recon_eps"),
             ("NaN eps", Run(35, eps=NAN), L.JAT_E_INVALID, "recon_eps"),
             ("NaN reconstruction weight", Run(35, rw=NAN), L.JAT_E_INVALID, "finite"),
             ("NaN latent weight", Run(35, weights=dict(K.WEIGHTS, latent_weight=NAN)), L.JAT_E_INVALID, "finite"),
             ("T too long", Run(K.REJECT_T, rows_T=2), L.JAT_E_INVALID, "too long"),
             ("work one byte short", Run(35, work_short=1), L.JAT_E_STATE, "work buffer too small")]
    for label, r, code, why in cases:
        rc = r.call()
        msg = lib.jat_last_error().decode()
        assert rc == code and why in msg, (label, rc, msg)
        assert r.untouched() and r.guards_ok(), label
        with pytest.raises((ValueError, L.JatError)):
            L.check(rc)
    torch.cuda.synchronize()                    # no launch failure is pending either
    run_and_check(35, "T=35 after the rejections")
