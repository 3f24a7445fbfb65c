"""Every launch path of the v3mod2 latent perceptual loss (csrc/train.hip: latent_loss_kernel<1,2>, <2,4>, <3,6> with its chunk
loops, latent_loss_fft_kernel, latent_loss_finish_kernel, all through `jat_k_latent_loss`) against the fp64 oracle
oracle/latent_loss_oracle.py, which tests/test_train_cpu.py pins to the reference's loss classes.

`launch_latent_loss` picks the path from the sequence length alone; tests/loss_path_cases.py holds the length table and
tests/test_loss_paths_cpu.py proves that it reaches every path.  Gates are the project's existing ones
(test_latent_loss_kernel_vs_reference_classes in tests/test_gpu_train.py): every term within 2e-5 relative, d total / d pred
within rel-L2 2e-4 — here for the whole tensor AND for every row on its own, since row 1 is 1000 x louder than the others
and would hide them in a global norm.  The inputs, not the tolerance, keep a correct fp32 kernel inside the gate: see the
preconditions in tests/loss_path_cases.py, asserted from fp64 numpy before the kernel runs.

pred / target / lr are exactly rows*T long inside NaN-filled arenas, dpred / out6 / work sit between NaN guard bands: a read
or write past a row's end shows as a NaN or a broken guard.
"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import jatsr_amd._lib as L  # noqa: E402
import loss_path_cases as K  # noqa: E402
from helpers import rel_l2  # noqa: E402
from oracle import latent_loss_oracle as LO  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TERM_TOL, DPRED_TOL = 2e-5, 2e-4
TERMS = ("total", "mse", "freq", "ms", "consistency", "latent")
GUARD = 64
NAN = float("nan")
DIRECT = os.environ.get("JAT_LOSS_DIRECT_DFT", "0").strip() not in ("", "0")     # the library's A/B switch, this process


def guarded(shape, dtype=torch.float32, fill=NAN):
    """(buffer, view): the view has `shape`, the buffer holds GUARD NaN elements before and after it (as in
    tests/test_gpu_train_kernels.py)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), NAN, dtype=dtype, device="cuda")
    view = buf[GUARD:GUARD + n].view(shape)
    if torch.is_tensor(fill):
        view.copy_(fill)
    return buf, view


def guards_intact(buf):
    return bool(torch.isnan(buf[:GUARD].float()).all()) and bool(torch.isnan(buf[-GUARD:].float()).all())


def work_bytes(T, rows):
    return (T * 8 + 255) // 256 * 256 + rows * 32        # what include/jat_hip.h states for jat_k_latent_loss


def plan(T):
    kind, a, b, lds = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1), C.c_int64(-1)
    L.check(L.lib().jat_k_latent_loss_plan(T, C.byref(kind), C.byref(a), C.byref(b), C.byref(lds)))
    return kind.value, a.value, b.value, lds.value


@functools.lru_cache(maxsize=None)
def case_inputs(T):
    x = K.make_inputs(T, K.SALT[T])
    for a in x:
        a.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _reference(T, weights, cuts):
    """fp64 oracle on the inputs of length T, computed once per (weights, cut-offs) and shared, read-only."""
    pred, target, lr = case_inputs(T)
    pre = K.preconditions(pred, target, lr, cuts=dict(cuts))
    assert K.preconditions_hold(pre), f"T = {T}: the inputs miss the preconditions {pre} (bounds {K.PRE_BOUNDS})"
    terms, dpred = LO.latent_loss(pred, target, lr, **dict(weights), **dict(cuts))
    dpred = dpred[0]
    dpred.setflags(write=False)
    return terms, dpred


def reference(T, weights=None, cuts=None):
    return _reference(T, tuple(sorted((weights or K.WEIGHTS).items())), tuple(sorted((cuts or K.CUTS).items())))


class Run:
    """One call of jat_k_latent_loss on the inputs of length T inside guarded arenas."""

    def __init__(self, T, weights=None, cuts=None, loss_scale=1.0, with_lr=True, work_short=0, rows_T=None):
        L.require_gpu()
        w, c = dict(weights or K.WEIGHTS), dict(cuts or K.CUTS)
        if rows_T is None:
            x = case_inputs(T)
            self.rows = x[0].shape[1]
            self.inputs = [guarded((self.rows, T), fill=torch.tensor(a[0], device="cuda")) for a in x]
        else:                                   # shapes no kernel takes: nothing is read, the data does not matter
            self.rows = rows_T
            self.inputs = [guarded((self.rows, T), fill=torch.zeros(self.rows, T, device="cuda")) for _ in range(3)]
        self.T = T
        self.dbuf, self.dpred = guarded((self.rows, T))
        self.obuf, self.out6 = guarded((6,))
        nwork = work_bytes(T, self.rows) - work_short
        self.wbuf = torch.full((nwork + 2 * GUARD * 4,), 0xFF, dtype=torch.uint8, device="cuda")   # 0xFFFFFFFF: a NaN
        self.args = (L.ptr(self.inputs[0][1]), L.ptr(self.inputs[1][1]), L.ptr(self.inputs[2][1]) if with_lr else None,
                     L.ptr(self.dpred), L.ptr(self.out6), self.rows, T, w["latent_weight"], w["freq_weight"], w["ms_weight"],
                     w["consistency_weight"], c["low_freq_phase_ratio"], c["strict_cutoff"], c["soft_cutoff"], loss_scale,
                     C.c_void_p(self.wbuf.data_ptr() + GUARD * 4), nwork, L.stream_ptr())

    def call(self):
        rc = L.lib().jat_k_latent_loss(*self.args)
        torch.cuda.synchronize()
        return rc

    def guards_ok(self):
        w = self.wbuf
        return (guards_intact(self.dbuf) and guards_intact(self.obuf) and bool((w[:GUARD * 4] == 0xFF).all())
                and bool((w[-GUARD * 4:] == 0xFF).all()) and all(guards_intact(b) for b, _ in self.inputs))

    def untouched(self):
        """Nothing was written anywhere: outputs and scratch still hold their fill."""
        return (bool(torch.isnan(self.dbuf).all()) and bool(torch.isnan(self.obuf).all()) and bool((self.wbuf == 0xFF).all()))


def run_and_check(T, label, weights=None, cuts=None, loss_scale=1.0, with_lr=True, skip_terms=()):
    """The checks every case gets; -> (out6 as a dict of python floats, dpred / loss_scale as fp32 numpy)."""
    terms_ref, dp_ref = reference(T, weights, cuts)
    r = Run(T, weights, cuts, loss_scale, with_lr)
    L.check(r.call())
    out_a, dp_a = r.out6.clone(), r.dpred.clone()
    assert r.guards_ok(), f"{label}: a guard band was written"
    assert bool(torch.isfinite(dp_a).all()) and bool(torch.isfinite(out_a).all()), f"{label}: non-finite output"
    # a second call: same bits
    r.dpred.fill_(NAN)
    r.out6.fill_(NAN)
    L.check(r.call())
    assert torch.equal(r.dpred, dp_a) and torch.equal(r.out6, out_a), f"{label}: the second call differs"
    assert r.guards_ok()
    got = dict(zip(TERMS, out_a.double().tolist()))
    dp = dp_a.cpu().numpy() / np.float32(loss_scale)
    # a term the oracle gives as exactly zero (an empty band, T / 2 == 0) must be exactly zero
    term_err = {k: abs(got[k] - terms_ref[k]) / abs(terms_ref[k]) if terms_ref[k] != 0 else (0.0 if got[k] == 0 else np.inf)
                for k in TERMS if k not in skip_terms}
    whole = rel_l2(dp, dp_ref)
    per_row = [rel_l2(dp[i], dp_ref[i]) for i in range(dp.shape[0])]
    zero_rows = [i for i in range(dp.shape[0]) if not dp_ref[i].any()]
    print(f"{label}: plan {plan(T)[:3]}, worst term {max(term_err, key=term_err.get)} {max(term_err.values()):.2e} "
          f"(gate {TERM_TOL:.0e}); dpred rel-L2 whole {whole:.2e}, rows {' '.join(f'{v:.2e}' for v in per_row)} "
          f"(gate {DPRED_TOL:.0e}); oracle-zero rows {zero_rows}")
    for k, v in term_err.items():
        assert v <= TERM_TOL, f"{label}: {k} = {got[k]!r} vs {terms_ref[k]!r} (rel {v:.3e})"
    assert whole <= DPRED_TOL, f"{label}: dpred rel-L2 {whole:.3e}"
    for i, v in enumerate(per_row):
        # a row the oracle gives as exactly zero (sign(0) = 0 on every branch) must be exactly zero: rel_l2 divides by 1e-30
        assert v <= DPRED_TOL, f"{label}: row {i} dpred rel-L2 {v:.3e}"
    return got, dp


@pytest.mark.parametrize("T", [T for T, _, _ in K.LENGTHS])
def test_every_launch_path_vs_fp64_oracle(T):
    """The length table in its order: factored lengths up to the largest LDS image, then the three direct instances up to the
    composite length that falls back to the direct kernel."""
    if not DIRECT:
        assert plan(T)[:3] == ({"direct": 1, "fft": 2}[K.PATH[T][0]],) + K.PATH[T][1:]
    got, dp = run_and_check(T, f"T={T}")
    _, dp_ref = reference(T)
    # the tie row: e == 0 everywhere, so only the consistency term against the clean LR row moves it; the zero row: P == 0,
    # so the log-magnitude and the band-magnitude terms give no gradient (sign(0) = 0, as the oracle's)
    F = T // 2 + 1
    if int(F * K.CUTS["soft_cutoff"]) == 0:
        assert not dp_ref[K.TIE].any() and not dp[K.TIE].any()


def test_small_lds_requests_after_the_largest_ones():
    """The launcher raises each kernel's dynamic-LDS limit only when a request exceeds the largest one so far.  A small
    request after the largest (factored: 149 KiB at T = 4096; direct <1,2>: T = 509) must still launch and be right."""
    assert plan(4096)[3] == 149128
    run_and_check(4096, "T=4096 (first)")
    run_and_check(509, "T=509 (first)")
    run_and_check(23, "T=23 after 509")
    run_and_check(8, "T=8 after 4096")


@pytest.mark.parametrize("T", K.SWEEP_T)
def test_argument_sweep(T):
    """What the trainer varies: the loss scale, each weight at zero, no clean-LR tensor, non-default band cut-offs."""
    base, dp_base = run_and_check(T, f"T={T} base")
    # loss_scale: the terms do not see it, bit for bit; dpred / scale meets the same gate
    for scale in (2.0 ** -3, 1024.0):
        got, _ = run_and_check(T, f"T={T} loss_scale={scale}", loss_scale=scale)
        assert got == base, (scale, got, base)
    # consistency off and no clean-LR tensor at all (v3mod2 without the consistency term)
    w = dict(K.WEIGHTS, consistency_weight=0.0)
    got, dp = run_and_check(T, f"T={T} cw=0 lr=NULL", weights=w, with_lr=False, skip_terms=("consistency",))
    assert got["consistency"] == 0.0
    assert not dp[K.TIE].any()                  # pred == target and nothing else pulls on the row
    for name in ("freq_weight", "ms_weight"):
        run_and_check(T, f"T={T} {name}=0", weights=dict(K.WEIGHTS, **{name: 0.0}))
    # latent weight 0: dpred is the MSE gradient alone, 2 e / n, to fp32 rounding (e, 1/n and two products: 4 * 2^-24 = 2.4e-7
    # relative per element; gated at twice that)
    _, dp = run_and_check(T, f"T={T} lw=0", weights=dict(K.WEIGHTS, latent_weight=0.0))
    pred, target, _ = case_inputs(T)
    mse_grad = 2.0 * (pred[0].astype(np.float64) - target[0].astype(np.float64)) / pred[0].size
    assert np.all(np.abs(dp - mse_grad) <= 4.8e-7 * np.abs(mse_grad))
    # band cut-offs: the same arguments to the kernel and to the oracle
    F = T // 2 + 1
    for name, cuts in K.sweep_cuts(T).items():
        lo, st, so = (int(F * cuts[k]) for k in ("low_freq_phase_ratio", "strict_cutoff", "soft_cutoff"))
        assert {"band0": lo == 0 and so == st, "band1": so - st == 1, "soft1": so == F}[name]
        run_and_check(T, f"T={T} {name} (low, strict, soft) = ({lo}, {st}, {so})", cuts=cuts)


def test_rejections_launch_nothing():
    """A length whose LDS image does not fit, band cut-offs out of order, a phase ratio above 1, a work buffer one byte short:
    an error code, `jat_last_error()` says why, and nothing was written to the outputs or the scratch."""
    lib = L.lib()
    cases = [("T too long", Run(K.REJECT_T, rows_T=2), "too long"),
             ("soft < strict", Run(35, cuts=dict(K.CUTS, strict_cutoff=0.36, soft_cutoff=0.30)), "band ratios"),
             ("phase ratio > 1", Run(35, cuts=dict(K.CUTS, low_freq_phase_ratio=1.25)), "band ratios"),
             ("work one byte short", Run(35, work_short=1), "work buffer too small")]
    assert plan(K.REJECT_T)[0] == 0
    for label, r, why in cases:
        rc = r.call()
        msg = lib.jat_last_error().decode()
        assert rc != L.JAT_OK and why in msg, (label, rc, msg)
        assert r.untouched() and r.guards_ok(), label
        with pytest.raises((ValueError, L.JatError)):
            L.check(rc)
    torch.cuda.synchronize()                    # no launch failure is pending either
    run_and_check(35, "T=35 after the rejections")


BOTH_BUILDS_T = (35, 257)            # a factored and a direct-DFT length of the table


def both_builds_outputs():
    """what the child on libjat_hip_fp16.so and this process both compute: `jat_k_latent_loss_ex` at a factored and a direct
    length, as the v3mod2 loss (recon_eps = 0: the base instances) and as the v3mod3 loss (recon_eps = 1e-6: the general ones)"""
    out = {}
    w, c = K.WEIGHTS, K.CUTS
    for T in BOTH_BUILDS_T:
        assert plan(T)[0] == {"direct": 1, "fft": 2}[K.PATH[T][0]] or DIRECT
        pred, target, lr = (torch.tensor(a[0], device="cuda") for a in case_inputs(T))
        rows = pred.shape[0]
        work = torch.zeros(work_bytes(T, rows), dtype=torch.uint8, device="cuda")
        for eps in (0.0, 1e-6):
            dpred, out6 = torch.full((rows, T), NAN, device="cuda"), torch.full((6,), NAN, device="cuda")
            L.check(L.lib().jat_k_latent_loss_ex(L.ptr(pred), L.ptr(target), L.ptr(lr), L.ptr(dpred), L.ptr(out6), rows, T, eps, 1.0,
                                                 w["latent_weight"], w["freq_weight"], w["ms_weight"], w["consistency_weight"],
                                                 c["low_freq_phase_ratio"], c["strict_cutoff"], c["soft_cutoff"], 1.0, L.ptr(work),
                                                 work.numel(), L.stream_ptr()))
            torch.cuda.synchronize()
            out[f"dpred_T{T}_eps{eps}"], out[f"out6_T{T}_eps{eps}"] = dpred.cpu().numpy(), out6.cpu().numpy()
    return out


def test_fp16_library_gives_the_same_bits(tmp_path):
    """latent_loss_kernel / latent_loss_fft_kernel are fp32 kernels inside train.hip, which the fp16 build compiles with
    -DJAT_FP16: libjat_hip_fp16.so, in a child process, computes the bits this process computes (also the entry of
    tests/test_gpu_mod3_loss.py in tests/fp16_matrix.py)"""
    code = ("import sys, numpy as np\n"
            "sys.path.insert(0, 'tests')\n"
            "import jatsr_amd._lib as L\n"
            "from test_gpu_loss_paths import both_builds_outputs\n"
            "assert L.operand_dtype() == 'fp16'\n"
            "np.savez(sys.argv[1], **both_builds_outputs())\n")
    env = dict(os.environ, JAT_OPERAND_DTYPE="fp16")
    env.pop("JAT_LIB_PATH", None)
    path = str(tmp_path / "fp16.npz")
    out = subprocess.run([sys.executable, "-c", code, path], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
    got, mine = dict(np.load(path)), both_builds_outputs()
    assert sorted(got) == sorted(mine) and len(mine) == 8
    for k, v in mine.items():
        assert v.dtype == np.float32 and np.isfinite(v).all() and np.abs(v).max() > 0, k
        assert np.array_equal(v, got[k]) and v.tobytes() == got[k].tobytes(), k
    for T in BOTH_BUILDS_T:                 # the two losses differ: the Charbonnier instances did run
        assert not np.array_equal(mine[f"dpred_T{T}_eps0.0"], mine[f"dpred_T{T}_eps1e-06"])


AB_LENGTHS = (1378, 128)


def test_ab_lengths_on_the_path_the_environment_selects():
    """T = 1378 and T = 128 on whichever kernel this process's JAT_LOSS_DIRECT_DFT selects (default: factored), same checks."""
    for T in AB_LENGTHS:
        assert plan(T)[0] == (1 if DIRECT else 2)
        run_and_check(T, f"T={T} {'direct (JAT_LOSS_DIRECT_DFT)' if DIRECT else 'factored'}")


def test_direct_dft_switch_in_a_child_process():
    """The A/B switch is read once per process: a fresh child runs the test above with JAT_LOSS_DIRECT_DFT=1, so the direct
    and the factored kernels meet the same oracle on identical inputs."""
    env = dict(os.environ, JAT_LOSS_DIRECT_DFT="1")
    out = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-s", "-p", "no:cacheprovider", "-m", "gpu",
                          "tests/test_gpu_loss_paths.py", "-k", "test_ab_lengths_on_the_path_the_environment_selects"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    tail = (out.stdout + out.stderr)[-3000:]
    print(tail)
    assert out.returncode == 0 and "1 passed" in out.stdout, tail
    assert "direct (JAT_LOSS_DIRECT_DFT)" in out.stdout
