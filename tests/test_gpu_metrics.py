"""The audio-quality metrics on the GPU (csrc/metrics.hip, jatsr_amd.metrics) against the fp64 restatement of their
definitions (tests/metrics_ref.py): the transform, the three public functions and `evaluate`, lsd_frames and the dB
matrices element-wise, edge lengths, the gain identities, determinism, the fp16-operand library, `load_audio`, the
refusals that need a handle, and `infer --simulate-lr --metrics` end to end.

Gates.  The yardstick is the same formula run in fp32 on the CPU (the restatement with dtype=np.float32) against fp64 on the
exact test signals; the gates are about 10x that (another summation order over up to 2048 terms, another transform
factorisation).  The metric gates and their yardsticks are in tests/metrics_ref.py.  For the transform the yardstick is
max-abs 5.4e-8 .. 6.0e-8 of max |X| and rel-L2 4.2e-8 over the three scales, so: max-abs <= 6e-7 max |X|, rel-L2 <= 5e-7.

Measured on MI355X (GPU vs fp64; every test prints its figures before it asserts):
  STFT          max-abs 7.4e-8 .. 2.0e-7 of max |X|, rel-L2 7.8e-8 .. 1.3e-7 (n_fft 64 .. 4096, alone and paired)
  lsd_db        rel 6.6e-9 .. 7.7e-7 (gate 7e-6)
  lsd_frames    max-abs 3.5e-6 (degraded, 2048 / 512; yardstick 1.8e-6), 9.7e-6 and 1.4e-5 (degraded, 1024 / 256, 100001
                samples, B = 1 and 3; yardsticks 1.0e-6 and 9e-6), 1.9e-4 (LR with its floor; yardstick 4.8e-5), 1.0e-4
                (simulate_lr fixture; yardstick 2e-5): one to ten times the fp32 CPU distance of the same case
  mel l1 / l2   6e-9 .. 2.1e-6 dB (gate 2e-5);  dB matrices max-abs 3.9e-5 .. 8.1e-4 (gate 1e-3; the largest on 128 bands
                at 512 / 128, where a band holds one or two bins)
  identities    pred = c gt (c = 0.5, 0.7, 3): every lsd_frames value within 4.3e-7 of |log10 c|; mel l1 3.0e-6, 3.4e-6,
                7.0e-6 and l2 4.8e-6, 5.2e-6, 8.7e-6 dB against 0 .. 1.2e-6 in fp64 (fp32 CPU: 1.8e-6 .. 3.8e-6; gate 2e-5)
                pred == gt: lsd_db 1.8e-5 (two independent fp32 roundings: 1.24e-5, gate 1.2e-4), mel l1 / l2 1.3e-6 /
                2.7e-6, multi-scale 1.3e-6 / 3.0e-6 (gate 2e-5); not 0: the two spectra share the rounding of one transform
  other sizes   (64 .. 4096, empty bands, as many bands as bins) lsd_frames 0.9 .. 9.5 times the fp32 CPU distance of the
                case (6.6e-4 against 6.9e-5 at n_fft 64), dB matrices 1.8 .. 4.6 times

Input conditioning.  LSD takes the log of magnitudes clamped at 1e-8, so on bins that hold nothing but rounding noise the
formula does not define the answer: on a brick-wall low-passed copy (every bin above 8 kHz exactly zero) the fp32 and fp64
CPU restatements already disagree by 2.4 % in lsd_db (tests/test_metrics_cpu.py).  Every signal used for LSD parity
therefore carries a broadband floor of at least 1e-4 rms.  The exact-zero-band input is kept as a robustness case: results
must be finite and the mel metrics must meet their normal gate; no LSD parity is asserted on it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import metrics_ref as M  # noqa: E402
import jatsr_amd  # noqa: E402
import jatsr_amd.io as jio  # noqa: E402
import jatsr_amd.metrics as metrics  # noqa: E402
import jatsr_amd.recipe as recipe  # noqa: E402
from jatsr_amd import _lib as L  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STFT_ABS_GATE, STFT_REL_GATE = 6e-7, 5e-7
SR = 44100
RAGGED = 3 * SR + 77                                   # 132377, odd: a multiple of no hop


def cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def fixtures(rows=1, n=3 * SR):
    """gt, the degraded pred, and the band-limited 'LR' with its 1e-4 rms floor: float32 [rows, n]"""
    gt = M.test_signal(n, rows=rows)
    return gt, M.degraded(gt), M.brickwall(gt, floor_rms=1e-4)


def stft_errors(X, ref):
    X = X.cpu().numpy().astype(np.complex128)
    assert X.shape == ref.shape, (X.shape, ref.shape)
    return float(np.abs(X - ref).max() / max(np.abs(ref).max(), 1e-30)), float(np.linalg.norm(X - ref) / max(np.linalg.norm(ref), 1e-30))


# ---- the transform ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n_fft,hop,_", M.SCALES)
def test_stft_against_fp64(n_fft, hop, _, B):
    x = M.test_signal(3 * SR, rows=B, seed=B)
    X = metrics.stft(cuda(x), n_fft, hop)
    assert X.dtype == torch.complex64 and X.shape == (B, 1 + n_fft // 2, 1 + 3 * SR // hop)
    mx, rel = stft_errors(X, M.stft(x, n_fft, hop))
    print(f"stft {n_fft}/{hop} B={B}: max-abs / max|X| {mx:.2e} (gate {STFT_ABS_GATE:.0e}), rel-L2 {rel:.2e} (gate {STFT_REL_GATE:.0e})")
    assert mx <= STFT_ABS_GATE and rel <= STFT_REL_GATE
    # 1-D in, 2-D out; and two signals sharing one complex transform, as the metrics run it
    assert torch.equal(metrics.stft(cuda(x[0]), n_fft, hop), X[0])
    y = M.degraded(x)
    Xp, Yp = metrics.stft(cuda(x), n_fft, hop, y=cuda(y))
    for name, got, sig in (("x", Xp, x), ("y", Yp, y)):
        mx, rel = stft_errors(got, M.stft(sig, n_fft, hop))
        print(f"  paired {name}: max-abs / max|X| {mx:.2e}, rel-L2 {rel:.2e}")
        assert mx <= STFT_ABS_GATE and rel <= STFT_REL_GATE


@pytest.mark.parametrize("n_fft,hop", [(512, 128), (1024, 256), (2048, 512), (64, 16), (128, 100), (4096, 1024)])
def test_stft_lengths(n_fft, hop):
    rng = np.random.default_rng(n_fft)
    for n in (1, hop - 1, hop, n_fft // 2, n_fft + 1, RAGGED if n_fft >= 512 else 7001):
        x = (0.3 * rng.standard_normal((2, n))).astype(np.float32)
        X = metrics.stft(cuda(x), n_fft, hop)
        ref = M.stft(x, n_fft, hop)
        assert X.shape == (2, 1 + n_fft // 2, 1 + n // hop), (n, X.shape)
        mx, rel = stft_errors(X, ref)
        print(f"stft {n_fft}/{hop} L={n}: max-abs / max|X| {mx:.2e}, rel-L2 {rel:.2e}")
        assert mx <= STFT_ABS_GATE and rel <= STFT_REL_GATE, n


# ---- the metrics -------------------------------------------------------------------------------------------------------------------
def check_lsd(pred, gt, n_fft=2048, hop=512):
    frames_gate = M.lsd_frames_gate(pred, gt, n_fft, hop)           # 10x the fp32 CPU yardstick on these very signals
    lsd, frames = metrics.calculate_lsd(cuda(pred), cuda(gt), n_fft, hop)
    r_lsd, r_frames = M.calculate_lsd(pred, gt, n_fft, hop)
    lsd, frames = lsd.cpu().numpy(), frames.cpu().numpy()
    assert lsd.shape == r_lsd.shape and frames.shape == r_frames.shape and frames.dtype == np.float32
    rel = float(np.max(np.abs(lsd - r_lsd) / r_lsd))
    mx = float(np.abs(frames - r_frames).max())
    print(f"lsd {n_fft}/{hop} {pred.shape}: lsd_db {np.ravel(r_lsd)[0]:.4f} rel {rel:.2e} (gate {M.LSD_REL_GATE:.0e}), "
          f"lsd_frames max-abs {mx:.2e} (gate {frames_gate:.0e})")
    assert rel <= M.LSD_REL_GATE and mx <= frames_gate


def check_mel(pred, gt, n_fft=2048, hop=512, n_mels=80, sr=SR):
    l1, l2, a, b = metrics.calculate_mel_loss(cuda(pred), cuda(gt), sr, n_mels, n_fft, hop)
    r1, r2, ra, rb = M.calculate_mel_loss(pred, gt, sr, n_mels, n_fft, hop)
    assert a.shape == ra.shape and b.shape == rb.shape and a.dtype == torch.float32 and l1.shape == r1.shape
    e1, e2 = float(np.abs(l1.cpu().numpy() - r1).max()), float(np.abs(l2.cpu().numpy() - r2).max())
    ed = max(float(np.abs(a.cpu().numpy() - ra).max()), float(np.abs(b.cpu().numpy() - rb).max()))
    print(f"mel {n_fft}/{hop}/{n_mels} {pred.shape}: l1 {np.ravel(r1)[0]:.4f} err {e1:.2e}, l2 {np.ravel(r2)[0]:.4f} err {e2:.2e} "
          f"(gate {M.MEL_GATE:.0e}), dB max-abs {ed:.2e} (gate {M.DB_GATE:.0e})")
    assert e1 <= M.MEL_GATE and e2 <= M.MEL_GATE and ed <= M.DB_GATE
    assert float(a.max()) == 0.0 and float(b.max()) == 0.0 and float(a.min()) >= -80.0 and float(b.min()) >= -80.0


@pytest.mark.parametrize("B", [1, 3])
def test_lsd_against_fp64(B):
    gt, pred, lr = fixtures(B)
    check_lsd(pred, gt)
    check_lsd(lr, gt)
    check_lsd(pred[0], gt[0])                                    # 1-D in, scalars out
    check_lsd(pred[:, :100001], gt[:, :100001], 1024, 256)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n_fft,hop,n_mels", M.SCALES)
def test_mel_loss_against_fp64(n_fft, hop, n_mels, B):
    gt, pred, lr = fixtures(B)
    check_mel(pred, gt, n_fft, hop, n_mels)
    check_mel(lr, gt, n_fft, hop, n_mels)
    if B == 1:
        check_mel(pred[0, :100001], gt[0, :100001], n_fft, hop, n_mels)
        check_mel(pred[0], gt[0], n_fft, hop, 128, sr=22050)


@pytest.mark.parametrize("n_fft,hop,n_mels", [(64, 16, 20), (64, 16, 33), (256, 64, 129), (4096, 1024, 128), (128, 100, 30)])
def test_other_sizes(n_fft, hop, n_mels):
    """Sizes outside the three scales: sixteen frames side by side in a block (64), one block per CU (4096), as many bands
    as bins and empty bands (their power is 0, so they sit on the -80 dB floor in both signals).  The fixed gates come from
    the three scales, so here every gate is 10x the fp32 CPU distance on these very signals, or the fixed gate where that is
    larger (a scalar is a sum of signed errors and can come out small by accident)."""
    gt, pred, _ = fixtures(2, SR)
    y32 = (M.calculate_lsd(pred, gt, n_fft, hop, np.float32), M.calculate_mel_loss(pred, gt, SR, n_mels, n_fft, hop, np.float32))
    y64 = (M.calculate_lsd(pred, gt, n_fft, hop), M.calculate_mel_loss(pred, gt, SR, n_mels, n_fft, hop))
    lsd, frames = metrics.calculate_lsd(cuda(pred), cuda(gt), n_fft, hop)
    l1, l2, a, b = metrics.calculate_mel_loss(cuda(pred), cuda(gt), SR, n_mels, n_fft, hop)
    got = (lsd.cpu().numpy(), frames.cpu().numpy(), l1.cpu().numpy(), l2.cpu().numpy(), a.cpu().numpy(), b.cpu().numpy())
    ref = (y64[0][0], y64[0][1], y64[1][0], y64[1][1], y64[1][2], y64[1][3])
    yard = (y32[0][0], y32[0][1], y32[1][0], y32[1][1], y32[1][2], y32[1][3])
    floors = (M.LSD_REL_GATE * ref[0].max(), 0.0, M.MEL_GATE, M.MEL_GATE, M.DB_GATE, M.DB_GATE)
    for name, g, r, y, floor in zip(("lsd_db", "lsd_frames", "mel_l1", "mel_l2", "pred_db", "gt_db"), got, ref, yard, floors):
        assert g.shape == r.shape, name
        err, gate = float(np.abs(g - r).max()), max(floor, 10 * float(np.abs(y - r).max()))
        print(f"{n_fft}/{hop}/{n_mels} {name}: max-abs {err:.2e} (fp32 CPU {np.abs(y - r).max():.2e}, gate {gate:.1e})")
        assert err <= gate, name


def test_simulated_lr_fixture():
    # the other LR fixture: jatsr_amd.simulate_lr of a noisy signal (its own noise above the cut-off is filtered to about
    # -56 dB, far above rounding), plus the 1e-4 rms floor
    gt = M.test_signal(3 * 48000, sr=48000, rows=1)
    lr = jatsr_amd.simulate_lr(cuda(gt)).cpu().numpy()
    lr = (lr + 1e-4 * np.random.default_rng(5).standard_normal(lr.shape)).astype(np.float32)
    l64, f64 = M.calculate_lsd(lr, gt)
    l32, f32 = M.calculate_lsd(lr, gt, dtype=np.float32)
    print(f"simulate_lr fixture, fp32 CPU vs fp64: lsd_db rel {abs(l32 - l64).max() / l64.max():.1e}, lsd_frames {np.abs(f32 - f64).max():.1e}")
    assert np.abs(l32 - l64).max() / l64.max() < M.LSD_REL_GATE
    check_lsd(lr, gt)
    check_mel(lr, gt)


def assert_report(got, ref, tag):
    for k in metrics.METRIC_KEYS:
        gate = M.LSD_REL_GATE * ref[k] if k == "lsd" else M.MEL_GATE
        print(f"{tag} {k}: {got[k]:.6f} vs {ref[k]:.6f} (err {abs(got[k] - ref[k]):.2e}, gate {gate:.1e})")
        assert abs(got[k] - ref[k]) <= gate, (tag, k)
    for s, v in ref["ms_detail"].items():
        for n in ("l1", "l2"):
            assert abs(got["ms_detail"][s][n] - v[n]) <= M.MEL_GATE, (tag, s, n)


def test_multi_scale_and_evaluate_against_fp64():
    gt, pred, lr = (v[0] for v in fixtures())
    m1, m2, det = metrics.calculate_multi_scale_mel_loss(cuda(pred), cuda(gt))
    r1, r2, rdet = M.calculate_multi_scale_mel_loss(pred, gt)
    assert sorted(det) == sorted(rdet) == ["fft1024", "fft2048", "fft512"]
    assert abs(float(m1) - r1) <= M.MEL_GATE and abs(float(m2) - r2) <= M.MEL_GATE
    for k in rdet:
        assert abs(float(det[k]["l1"]) - rdet[k]["l1"]) <= M.MEL_GATE and abs(float(det[k]["l2"]) - rdet[k]["l2"]) <= M.MEL_GATE
    rep = metrics.evaluate(cuda(pred), cuda(gt), cuda(lr))
    assert sorted(rep) == ["generated", "improvement", "lr_input", "lsd_grade", "mel_grade"]
    ref_g, ref_l = M.evaluate_pair(pred, gt), M.evaluate_pair(lr, gt)
    assert_report(rep["generated"], ref_g, "generated")
    assert_report(rep["lr_input"], ref_l, "lr_input")
    for k in metrics.METRIC_KEYS:
        assert rep["improvement"][k]["abs"] == rep["lr_input"][k] - rep["generated"][k]
        assert rep["improvement"][k]["rel"] == 1.0 - rep["generated"][k] / rep["lr_input"][k]
    assert rep["lsd_grade"] == metrics.lsd_grade(ref_g["lsd"]) and rep["mel_grade"] == metrics.mel_grade(ref_g["mel_l1"])
    # the 2048 / 512 pass of evaluate is the pass of the single functions: the same bits
    assert rep["generated"]["lsd"] == float(metrics.calculate_lsd(cuda(pred), cuda(gt))[0])
    assert rep["generated"]["mel_l1"] == float(metrics.calculate_mel_loss(cuda(pred), cuda(gt))[0])
    assert rep["generated"]["ms_l1"] == float(m1) and rep["generated"]["ms_l2"] == float(m2)
    only = metrics.evaluate(cuda(pred), cuda(gt))
    assert sorted(only) == ["generated", "lsd_grade", "mel_grade"] and only["generated"] == rep["generated"]
    json.dumps(rep)
    # a batch gives lists
    gb, pb, _ = fixtures(2, SR)
    repb = metrics.evaluate(cuda(pb), cuda(gb))
    for row in range(2):
        one = metrics.evaluate(cuda(pb[row]), cuda(gb[row]))
        assert all(repb["generated"][k][row] == one["generated"][k] for k in metrics.METRIC_KEYS)
    print(metrics.format_report(rep))


def test_unequal_lengths_are_cut_to_the_shorter():
    gt, pred, _ = (v[0] for v in fixtures())
    a = metrics.evaluate(cuda(pred[:100000]), cuda(gt))
    b = metrics.evaluate(cuda(pred), cuda(gt[:100000]))
    c = metrics.evaluate(cuda(pred[:100000]), cuda(gt[:100000]))
    assert a == b == c
    assert_report(a["generated"], M.evaluate_pair(pred[:100000], gt), "cut")
    assert metrics.calculate_lsd(cuda(pred[:100000]), cuda(gt))[1].shape == (1 + 100000 // 512,)
    assert metrics.calculate_mel_loss(cuda(pred), cuda(gt[:100000]))[2].shape == (80, 1 + 100000 // 512)


@pytest.mark.parametrize("c", [0.5, 0.7, 3.0])
def test_gain_identities(c):
    """pred = c gt on a signal with a 0.02 rms noise floor (no bin reaches the clamps): lsd_db = 20 |log10 c| and the mel loss
    is 0, because ref=max removes a gain.  In lsd_frames the rounding errors of the bins are signed and average out, so the
    relative gate of lsd_db holds for every frame.  The mel losses are compared with the restatement's value under the gate
    of every other mel loss (the fp32 CPU restatement gives l1 1.8e-6 .. 2.7e-6 and l2 3.0e-6 .. 3.8e-6 dB here, against
    0 .. 1.2e-6 in fp64: 10x that is the fixed gate)."""
    gt = M.test_signal(3 * SR)[0]
    pred = (np.float32(c) * gt).astype(np.float32)
    want = 20 * abs(np.log10(float(np.float32(c))))
    lsd, frames = metrics.calculate_lsd(cuda(pred), cuda(gt))
    l1, l2, _, _ = metrics.calculate_mel_loss(cuda(pred), cuda(gt))
    r1, r2, _, _ = M.calculate_mel_loss(pred, gt)
    print(f"gain {c}: lsd_db {float(lsd):.7f} (closed form {want:.7f}), mel l1 {float(l1):.2e} (fp64 {r1:.2e}), "
          f"l2 {float(l2):.2e} (fp64 {r2:.2e}), gate {M.MEL_GATE:.0e}")
    # every frame's value is |log10 c|: an rms over bins, a scalar of the kind lsd_db is the mean of, under the same relative
    # gate (the per-case fp32 yardstick is no guide here: for c = 0.5 the scaling is exact in fp32 and it degenerates to 1.5e-8)
    err = float((frames.double().cpu() - want / 20).abs().max())
    print(f"  lsd_frames max |value - |log10 c|| {err:.2e} (gate {M.LSD_REL_GATE * want / 20:.1e})")
    assert err <= M.LSD_REL_GATE * want / 20 and abs(float(lsd) - want) <= M.LSD_REL_GATE * want
    assert abs(float(l1) - r1) <= M.MEL_GATE and abs(float(l2) - r2) <= M.MEL_GATE


def test_identical_signals():
    """pred == gt.  The two spectra come out of one complex transform and differ by its rounding, so the result is not
    exactly 0 as it is where the same code runs twice (which is why the fp32 CPU restatement gives 0 here and cannot serve
    as the yardstick directly).  The yardstick is what two independent fp32 roundings of gt's own spectrum give: with
    e = log10 |X_fp32| - log10 |X_fp64| of gt, d is the difference of two such errors, so lsd_db = 20 mean_f sqrt(2 mean_k e^2),
    1.24e-5 dB on this signal; the gate is 10x that.  The mel losses take the fixed gate, which is 10x the fp32 distance of
    the neighbouring case pred = c gt (test_gain_identities)."""
    gt = M.test_signal(3 * SR)[0]
    e = np.log10(np.maximum(np.abs(M.stft(gt, dtype=np.float32)), 1e-8).astype(np.float64)) - np.log10(np.maximum(np.abs(M.stft(gt)), 1e-8))
    yard = 20 * float(np.mean(np.sqrt(2 * np.mean(e ** 2, axis=0))))
    same = metrics.evaluate(cuda(gt), cuda(gt))["generated"]
    print(f"identical: lsd_db {same['lsd']:.2e} (two fp32 roundings {yard:.2e}, gate {10 * yard:.1e}), mel_l1 {same['mel_l1']:.2e}, "
          f"mel_l2 {same['mel_l2']:.2e}, ms_l1 {same['ms_l1']:.2e}, ms_l2 {same['ms_l2']:.2e} (gate {M.MEL_GATE:.0e})")
    assert 0 <= same["lsd"] <= 10 * yard
    assert all(0 <= same[k] <= M.MEL_GATE for k in ("mel_l1", "mel_l2", "ms_l1", "ms_l2"))


def test_exact_zero_band_and_silence_stay_finite():
    gt = M.test_signal(3 * SR)[0]
    lr0 = M.brickwall(gt)                                # no LSD parity on it: see the module docstring
    rep = metrics.evaluate(cuda(lr0), cuda(gt))["generated"]
    assert all(np.isfinite(rep[k]) for k in metrics.METRIC_KEYS)
    for n_fft, hop, n_mels in M.SCALES:
        check_mel(lr0, gt, n_fft, hop, n_mels)
    frames = metrics.calculate_lsd(cuda(lr0), cuda(gt))[1]
    assert bool(torch.isfinite(frames).all())
    # all-zero pred: every pred power sits below the 1e-10 clamp, its dB matrix is all 0
    z = np.zeros_like(gt)
    l1, l2, a, b = metrics.calculate_mel_loss(cuda(z), cuda(gt))
    lsd, fr = metrics.calculate_lsd(cuda(z), cuda(gt))
    assert np.isfinite([float(l1), float(l2), float(lsd)]).all() and bool(torch.isfinite(fr).all())
    assert not bool(a.any()) and float(b.min()) >= -80.0
    r1, r2, _, rb = M.calculate_mel_loss(z, gt)
    assert abs(float(l1) - r1) <= M.MEL_GATE and abs(float(l2) - r2) <= M.MEL_GATE
    both = metrics.evaluate(cuda(z), cuda(z))["generated"]
    assert all(both[k] == 0.0 for k in metrics.METRIC_KEYS)


def test_determinism_and_batch_independence():
    gt, pred, lr = fixtures(3, 2 * SR + 11)
    g, p = cuda(gt), cuda(pred)
    for n_fft, hop, n_mels in M.SCALES:
        a = metrics.calculate_mel_loss(p, g, SR, n_mels, n_fft, hop)
        b = metrics.calculate_mel_loss(p, g, SR, n_mels, n_fft, hop)
        la, lb = metrics.calculate_lsd(p, g, n_fft, hop), metrics.calculate_lsd(p, g, n_fft, hop)
        X = metrics.stft(p, n_fft, hop)
        assert all(torch.equal(u, v) for u, v in zip(a, b)) and all(torch.equal(u, v) for u, v in zip(la, lb))
        assert torch.equal(X, metrics.stft(p, n_fft, hop))
        for row in range(3):
            one = metrics.calculate_mel_loss(p[row].clone(), g[row].clone(), SR, n_mels, n_fft, hop)
            assert all(torch.equal(u[row], v) for u, v in zip(a, one)), (n_fft, row)
            lone = metrics.calculate_lsd(p[row].clone(), g[row].clone(), n_fft, hop)
            assert torch.equal(la[0][row], lone[0]) and torch.equal(la[1][row], lone[1]), (n_fft, row)
            assert torch.equal(X[row], metrics.stft(p[row].clone(), n_fft, hop))
    # a long row cuts its blocks differently from a short one: a frame keeps its bits
    long_p, long_g = cuda(np.tile(pred[0], 12)), cuda(np.tile(gt[0], 12))
    n = 20 * 512
    fa = metrics.calculate_lsd(long_p, long_g)[1]
    fb = metrics.calculate_lsd(long_p[:n + 2048].clone(), long_g[:n + 2048].clone())[1]
    assert torch.equal(fa[:18], fb[:18])


def test_fp16_library_gives_the_same_bits(tmp_path):
    code = ("import sys, numpy as np, torch\n"
            "sys.path.insert(0, 'tests')\n"
            "import jatsr_amd._lib as L\n"
            "import jatsr_amd.metrics as metrics\n"
            "from test_gpu_metrics import fixtures, cuda\n"
            "assert L.operand_dtype() == sys.argv[2]\n"
            "gt, pred, lr = fixtures(2, 44100 + 13)\n"
            "lsd, frames = metrics.calculate_lsd(cuda(pred), cuda(gt))\n"
            "l1, l2, a, b = metrics.calculate_mel_loss(cuda(lr), cuda(gt), 44100, 64, 1024, 256)\n"
            "X = torch.view_as_real(metrics.stft(cuda(pred), 512, 128))\n"
            "np.savez(sys.argv[1], **{k: v.cpu().numpy() for k, v in dict(lsd=lsd, frames=frames, l1=l1, l2=l2, a=a, b=b, X=X).items()})\n")
    got = {}
    for dtype in ("bf16", "fp16"):
        env = dict(os.environ, JAT_OPERAND_DTYPE=dtype)
        env.pop("JAT_LIB_PATH", None)
        path = str(tmp_path / f"{dtype}.npz")
        out = subprocess.run([sys.executable, "-c", code, path, dtype], cwd=ROOT, env=env, capture_output=True, text=True,
                             timeout=600)
        assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
        got[dtype] = dict(np.load(path))
    assert sorted(got["bf16"]) == sorted(got["fp16"]) and len(got["bf16"]) == 7
    for k, v in got["bf16"].items():
        assert v.tobytes() == got["fp16"][k].tobytes(), k
    gt, pred, lr = fixtures(2, 44100 + 13)
    ref = M.calculate_lsd(pred, gt)[0]
    assert (np.abs(got["fp16"]["lsd"] - ref) <= M.LSD_REL_GATE * ref).all()


def test_handle_refusals():
    """the refusals that need a handle: never a fault"""
    lib, C = L.lib(), metrics.C
    h = metrics._handle(SR, 2048, 512, 80, torch.device("cuda", torch.cuda.current_device()))
    sz = C.c_size_t()
    assert lib.jat_audio_metrics_workspace_bytes(h.ptr, 1, SR, C.byref(sz)) == 0 and sz.value > 0
    for B, n in ((0, SR), (-1, SR), (65536, SR), (1, 0), (1, -5), (1, 2 ** 31 - 2048), (1, 2 ** 40)):
        assert lib.jat_audio_metrics_workspace_bytes(h.ptr, B, n, C.byref(sz)) == L.JAT_E_INVALID, (B, n)
    small = metrics._handle(SR, 64, 1, 0, h.device)                       # 33 bins a sample: frames * bins passes 31 bits
    assert lib.jat_audio_metrics_workspace_bytes(small.ptr, 1, 2 ** 26, C.byref(sz)) == L.JAT_E_INVALID
    assert lib.jat_audio_metrics_workspace_bytes(small.ptr, 1, 2 ** 20, C.byref(sz)) == 0
    x = torch.zeros(1, SR, device="cuda")
    out = torch.zeros(1, 3, dtype=torch.float64, device="cuda")
    need = C.c_size_t()
    lib.jat_audio_metrics_workspace_bytes(h.ptr, 1, SR, C.byref(need))
    work = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    args = lambda wb, **kw: (h.ptr, L.ptr(x), L.ptr(x), kw.get("B", 1), kw.get("n", SR), 1, L.ptr(out), None, None, None,  # noqa: E731
                             L.ptr(work), wb, L.stream_ptr())
    assert lib.jat_audio_metrics_run(*args(need.value - 1)) == L.JAT_E_STATE
    assert lib.jat_audio_metrics_run(*args(0)) == L.JAT_E_STATE
    assert lib.jat_audio_metrics_run(*args(need.value, B=0)) == L.JAT_E_INVALID
    assert lib.jat_audio_metrics_run(*args(need.value, n=0)) == L.JAT_E_INVALID
    assert lib.jat_audio_metrics_run(*args(need.value)) == 0
    assert lib.jat_stft(h.ptr, L.ptr(x), None, 1, 0, L.ptr(out), None, L.stream_ptr()) == L.JAT_E_INVALID
    assert lib.jat_stft(h.ptr, L.ptr(x), L.ptr(x), 1, SR, L.ptr(out), None, L.stream_ptr()) == L.JAT_E_INVALID
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        metrics.calculate_lsd(x, x, n_fft=1000)
    with pytest.raises(ValueError):
        metrics.calculate_lsd(x[:, :0], x[:, :0])
    with pytest.raises(ValueError):
        metrics.calculate_mel_loss(x, x, n_mels=2000)
    with pytest.raises(L.JatError):
        metrics.calculate_lsd(x, x[0])
    with pytest.raises(L.JatError):
        metrics.calculate_lsd(x.double(), x.double())
    assert jatsr_amd.calculate_lsd(x, x)[1].shape == (1, 1 + SR // 512)
    torch.cuda.synchronize()


# ---- files -----------------------------------------------------------------------------------------------------------------------------
def test_load_audio_round_trip(tmp_path):
    from jatsr_amd.resample import resample
    x = M.test_signal(48000, sr=48000, rows=2)                            # 1 s of 48 kHz stereo
    jio.write_wav_float32(tmp_path / "st.wav", x, 48000)
    back, sr = jio.read_wav(tmp_path / "st.wav", mono=False)
    assert sr == 48000 and np.array_equal(back, x)
    y, sr = metrics.load_audio(tmp_path / "st.wav")
    assert sr == 44100 and y.is_cuda and y.shape == (44100,)
    assert torch.equal(y, resample(cuda(x), 48000, 44100).mean(dim=0))    # resample each channel, then average
    jio.write_wav_float32(tmp_path / "mono.wav", x[0], 44100)
    y, _ = metrics.load_audio(tmp_path / "mono.wav")
    assert torch.equal(y, cuda(x[0]))                                      # at the target rate a mono file comes back as it is
    rep = metrics.main(["--pred", str(tmp_path / "st.wav"), "--gt", str(tmp_path / "mono.wav"), "--lr", str(tmp_path / "st.wav"),
                        "--json", str(tmp_path / "rep.json")])
    assert json.loads((tmp_path / "rep.json").read_text()) == rep and "improvement" in rep


def _infer_setup(tmp_path):
    """the setup of tests/test_gpu_prepare.py: synthetic DAC weights, a micro checkpoint, unit statistics, a 22.05 kHz WAV"""
    full = {"decoder." + k: torch.from_numpy(v) for k, v in recipe.make_dac_state_dict().items()}
    full.update({k: torch.from_numpy(v) for k, v in recipe.make_dac_encoder_state_dict().items()})
    torch.save(full, tmp_path / "dac.pt")
    cfg = dict(recipe.CONFIGS["micro"], input_channels=1024, cond_channels=1024)
    torch.save({"model_state_dict": {k: torch.from_numpy(v) for k, v in recipe.make_state_dict(cfg).items()},
                "config": dict(cfg)}, tmp_path / "last.pt")
    ones, zeros = [1.0] * 1024, [0.0] * 1024
    (tmp_path / "stats.json").write_text(json.dumps({"hr_mean": zeros, "hr_std": ones, "lr_mean": zeros, "lr_std": ones}))
    x = recipe.make_dac_audio(1, int(round(3.0 * 22050)), 63, sample_rate=22050)[0, 0]
    jio.write_wav_float32(tmp_path / "song.wav", x, 22050)
    return ["--checkpoint", str(tmp_path / "last.pt"), "--stats-file", str(tmp_path / "stats.json"), "--steps", "2",
            "--seed", "3", "--dac-weights", str(tmp_path / "dac.pt"), "--input-audio", str(tmp_path / "song.wav"), "--simulate-lr"]


def test_infer_metrics_from_a_latent_file(tmp_path):
    """A latent file with hr_latent is the other input with a ground truth: the HR audio is its decoded hr_latent, and the
    JSON carries the `_cfgX` suffix of the generated files.  A file without hr_latent is refused."""
    from jatsr_amd.infer import main as infer_main
    args = _infer_setup(tmp_path)
    base = args[:args.index("--input-audio")] + ["--cfg-scale", "2.0"]
    hr, lr = (torch.from_numpy(recipe.gaussian(name, (1024, 258), 70 + i)) for i, name in enumerate(("hr_latent", "lr_latent")))
    jio.save_latent_file(tmp_path / "pair.pt", hr_latent=hr, lr_latent=lr)
    jio.save_latent_file(tmp_path / "lronly.pt", lr_latent=lr)
    infer_main(base + ["--input-file", str(tmp_path / "pair.pt"), "--output-dir", str(tmp_path / "o"), "--metrics"])
    names = sorted(os.listdir(tmp_path / "o"))
    assert names == ["pair_generated_cfg2.0.pt", "pair_generated_cfg2.0.wav", "pair_hr_gt.wav", "pair_lr_input.wav",
                     "pair_metrics_cfg2.0.json"]
    rep = json.loads((tmp_path / "o" / "pair_metrics_cfg2.0.json").read_text())
    gen, gt, low = (metrics.load_audio(tmp_path / "o" / n)[0] for n in ("pair_generated_cfg2.0.wav", "pair_hr_gt.wav", "pair_lr_input.wav"))
    assert gt.shape == (258 * 512,) and rep == metrics.evaluate(gen, gt, low)
    with pytest.raises(SystemExit, match="hr_latent"):
        infer_main(base + ["--input-file", str(tmp_path / "lronly.pt"), "--output-dir", str(tmp_path / "o2"), "--metrics"])
    assert os.listdir(tmp_path / "o2") == []                          # refused before anything is sampled or written


def test_infer_simulate_lr_metrics_end_to_end(tmp_path):
    from jatsr_amd.infer import main as infer_main
    base = _infer_setup(tmp_path)
    infer_main(base + ["--output-dir", str(tmp_path / "plain")])
    infer_main(base + ["--output-dir", str(tmp_path / "m"), "--metrics"])
    wavs = ["song_generated.wav", "song_hr_gt.wav", "song_lr_input.wav"]
    assert sorted(os.listdir(tmp_path / "plain")) == sorted(wavs + ["song_generated.pt"])         # no JSON without the flag
    assert sorted(os.listdir(tmp_path / "m")) == sorted(wavs + ["song_generated.pt", "song_metrics.json"])
    for name in wavs:
        assert (tmp_path / "plain" / name).read_bytes() == (tmp_path / "m" / name).read_bytes(), name
    a, b = (torch.load(tmp_path / d / "song_generated.pt", weights_only=False) for d in ("plain", "m"))
    assert torch.equal(a["generated_latent"], b["generated_latent"])       # the .pt metadata holds a wall time: not compared as bytes
    rep = json.loads((tmp_path / "m" / "song_metrics.json").read_text())
    gen, hr, lr = (metrics.load_audio(tmp_path / "m" / name)[0] for name in wavs)
    assert rep == metrics.evaluate(gen, hr, lr)
    assert sorted(rep) == ["generated", "improvement", "lr_input", "lsd_grade", "mel_grade"]
    assert all(np.isfinite(rep[s][k]) for s in ("generated", "lr_input") for k in metrics.METRIC_KEYS)
