"""Host side of the audio-quality metrics (jatsr_amd.metrics, csrc/jat_metrics.cpp) and their fp64 restatement
(tests/metrics_ref.py): the restatement against independent implementations (torch.stft, librosa's published mel values),
the host entry points of the C ABI, every refusal that needs no device handle, closed-form signals, the fp32 yardstick the
GPU gates are derived from, and the command lines.  No GPU.  (The refusals that need a handle — L, B, the 31-bit limits, a
short workspace — are in tests/test_gpu_metrics.py: a handle uploads its tables when it is created.)"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import metrics_ref as M
import jatsr_amd.metrics as metrics
from jatsr_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def built_lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.lib()


# ---- the restatement against independent implementations --------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,hop,_", M.SCALES)
def test_restatement_stft_equals_torch_stft(n_fft, hop, _):
    x = M.test_signal(3 * 44100)[0]
    ours = M.stft(x, n_fft, hop)
    ref = torch.stft(torch.from_numpy(x).double(), n_fft, hop, window=torch.hann_window(n_fft, periodic=True, dtype=torch.float64),
                     center=True, pad_mode="constant", return_complex=True).numpy()
    assert ours.shape == ref.shape == (1 + n_fft // 2, 1 + len(x) // hop)
    err = np.abs(ours - ref).max()
    print(f"n_fft {n_fft}: max-abs {err:.1e}")                     # measured: 1.6e-14, 3.2e-14, 6.2e-14
    assert err < 1e-12
    # a batch is its rows
    xb = M.test_signal(5000, rows=2)
    assert np.array_equal(M.stft(xb, n_fft, hop)[1], M.stft(xb[1], n_fft, hop))


def test_restatement_mel_scale_reproduces_librosa_documentation():
    assert abs(M.hz_to_mel(60) - 0.9) < 1e-12 and abs(M.mel_to_hz(3) - 200.0) < 1e-12 and abs(M.hz_to_mel(1000) - 15.0) < 1e-12
    assert np.allclose(M.mel_frequencies(40, fmax=11025.0)[:3], [0.0, 85.317, 170.635], atol=1e-3)
    w = M.mel_filterbank(22050, 2048, 128)
    assert w.shape == (128, 1025) and np.allclose(w[0, :3], [0.0, 0.01618, 0.03237], atol=5e-6)
    assert np.allclose(M.mel_to_hz(M.hz_to_mel(np.array([10.0, 999.0, 1000.0, 4000.0, 22050.0]))),
                       [10.0, 999.0, 1000.0, 4000.0, 22050.0], rtol=1e-12)


# ---- host entry points ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr,n_fft,n_mels,nnz,widest", [(44100, 512, 40, 486, 47), (44100, 1024, 64, 991, 62),
                                                         (44100, 2048, 80, 1995, 100), (22050, 2048, 128, None, None)])
def test_mel_filterbank_against_the_restatement(sr, n_fft, n_mels, nnz, widest):
    w = metrics.mel_filterbank(sr, n_fft, n_mels).numpy()
    ref = M.mel_filterbank(sr, n_fft, n_mels)
    assert w.shape == ref.shape == (n_mels, 1 + n_fft // 2) and w.dtype == np.float32
    ulp = np.spacing(np.float32(ref.max()))
    err = np.abs(w.astype(np.float64) - ref).max()
    print(f"{sr} {n_fft} {n_mels}: max-abs {err:.2e}, one fp32 ulp of the maximum {ulp:.2e}")
    assert err <= ulp
    assert np.array_equal(w > 0, ref.astype(np.float32) > 0)
    per_band = (w > 0).sum(axis=1)
    if nnz is not None:
        assert (int(per_band.sum()), int(per_band.max())) == (nnz, widest) and per_band.min() >= 1


def test_stft_frames():
    for n, hop in ((1, 512), (511, 512), (512, 512), (513, 512), (2097152, 512), (705536, 128), (7, 1)):
        assert metrics.frames_for(n, hop) == 1 + n // hop == M.n_frames(n, hop)
    out = C.c_int64()
    assert L.lib().jat_stft_frames(0, 512, C.byref(out)) == L.JAT_E_INVALID
    assert L.lib().jat_stft_frames(100, 0, C.byref(out)) == L.JAT_E_INVALID
    assert L.lib().jat_stft_frames(100, 512, None) == L.JAT_E_INVALID


def test_refusals_that_need_no_handle():
    lib = L.lib()
    h = C.c_void_p()
    bad = [dict(n_fft=32), dict(n_fft=8192), dict(n_fft=1000), dict(n_fft=0), dict(n_fft=-2048), dict(hop=0), dict(hop=-1),
           dict(n_mels=-1), dict(n_mels=1026), dict(sr=0), dict(sr=-44100)]
    for over in bad:
        a = dict(sr=44100, n_fft=2048, hop=512, n_mels=80)
        a.update(over)
        rc = lib.jat_audio_metrics_create(a["sr"], a["n_fft"], a["hop"], a["n_mels"], None, C.byref(h))
        assert rc == L.JAT_E_INVALID and not h.value and lib.jat_last_error(), over
        if "hop" not in over:
            assert lib.jat_mel_filterbank(a["sr"], a["n_fft"], a["n_mels"], None) == L.JAT_E_INVALID, over
    assert lib.jat_audio_metrics_create(44100, 2048, 512, 80, None, None) == L.JAT_E_INVALID
    # a null handle is refused by every entry point that takes one
    sz = C.c_size_t()
    assert lib.jat_audio_metrics_workspace_bytes(None, 1, 1000, C.byref(sz)) == L.JAT_E_INVALID
    assert lib.jat_audio_metrics_run(None, None, None, 1, 1000, 1, None, None, None, None, None, 0, None) == L.JAT_E_INVALID
    assert lib.jat_stft(None, None, None, 1, 1000, None, None, None) == L.JAT_E_INVALID
    lib.jat_audio_metrics_destroy(None)
    with pytest.raises(ValueError):
        metrics.mel_filterbank(44100, 1000, 40)
    # the Python layer: no CPU path, fp32 only, matching shapes
    x = torch.zeros(1000)
    for fn in (metrics.calculate_lsd, metrics.calculate_mel_loss, metrics.calculate_multi_scale_mel_loss, metrics.evaluate):
        with pytest.raises(L.JatError):
            fn(x, x)
    with pytest.raises(L.JatError):
        metrics.stft(x)


# ---- closed forms through the restatement -----------------------------------------------------------------------------------------
def test_identical_signals_give_zero():
    x = M.test_signal(44100)[0]
    lsd, frames = M.calculate_lsd(x, x)
    l1, l2, a, b = M.calculate_mel_loss(x, x)
    assert lsd == 0 and not frames.any() and l1 == 0 and l2 == 0 and np.array_equal(a, b) and a.max() == 0 and a.min() >= -80
    m1, m2, det = M.calculate_multi_scale_mel_loss(x, x)
    assert m1 == 0 and m2 == 0 and sorted(det) == ["fft1024", "fft2048", "fft512"]


@pytest.mark.parametrize("c", [0.5, 0.7, 3.0])
def test_a_gain_moves_lsd_by_its_log_and_leaves_the_mel_loss(c):
    # the signal carries a 0.02 rms noise floor: no bin reaches the 1e-8 or 1e-10 clamps
    gt = M.test_signal(44100)[0].astype(np.float64)
    lsd, frames = M.calculate_lsd(c * gt, gt)
    assert abs(lsd - 20 * abs(np.log10(c))) < 1e-9 and np.allclose(frames, abs(np.log10(c)), atol=1e-10)
    l1, l2, a, b = M.calculate_mel_loss(c * gt, gt)
    assert l1 < 1e-9 and l2 < 1e-9                                  # ref=max removes a gain
    # unequal lengths are cut to the shorter
    assert M.calculate_lsd(c * gt, gt[:30000])[1].shape == (1 + 30000 // 512,)


def test_all_zero_pred_is_finite():
    gt = M.test_signal(44100)[0]
    for dtype in (np.float64, np.float32):
        lsd, frames = M.calculate_lsd(np.zeros_like(gt), gt, dtype=dtype)
        l1, l2, a, b = M.calculate_mel_loss(np.zeros_like(gt), gt, dtype=dtype)
        assert np.isfinite([lsd, l1, l2]).all() and np.isfinite(frames).all()
        assert not a.any() and b.min() >= -80                        # every pred power sits on the clamp: 0 dB everywhere
        G = np.maximum(np.abs(M.stft(gt, dtype=dtype)), 1e-8)
        assert np.allclose(frames, np.sqrt(np.mean((-8 - np.log10(G)) ** 2, axis=0)), rtol=1e-5)


# ---- the fp32 yardstick behind the GPU gates ------------------------------------------------------------------------------------
def test_fp32_yardstick_sits_below_the_gpu_gates():
    gt = M.test_signal(3 * 44100, rows=3)
    worst = dict(lsd=0.0, l1=0.0, l2=0.0, db=0.0)
    for name, pred in (("degraded", M.degraded(gt)), ("band-limited + 1e-4 floor", M.brickwall(gt, floor_rms=1e-4))):
        for n_fft, hop, n_mels in M.SCALES:
            l64, f64 = M.calculate_lsd(pred, gt, n_fft, hop)
            l32, f32 = M.calculate_lsd(pred, gt, n_fft, hop, np.float32)
            r64 = M.calculate_mel_loss(pred, gt, 44100, n_mels, n_fft, hop)
            r32 = M.calculate_mel_loss(pred, gt, 44100, n_mels, n_fft, hop, np.float32)
            rel, fr = np.abs(l32 - l64) / l64, np.abs(f32 - f64).max(axis=-1)
            e1, e2 = np.abs(r32[0] - r64[0]), np.abs(r32[1] - r64[1])
            ed = max(np.abs(r32[2] - r64[2]).max(), np.abs(r32[3] - r64[3]).max())
            print(f"{name} {n_fft}: lsd_db rel {rel.max():.1e}, lsd_frames max-abs {fr.min():.1e} .. {fr.max():.1e}, "
                  f"mel l1 {e1.max():.1e}, l2 {e2.max():.1e}, dB {ed:.1e}")
            worst = dict(lsd=max(worst["lsd"], rel.max()), l1=max(worst["l1"], e1.max()), l2=max(worst["l2"], e2.max()),
                         db=max(worst["db"], ed))
            assert abs(M.lsd_frames_gate(pred, gt, n_fft, hop) - 10 * fr.max()) < 1e-12
    print(f"largest: {worst}; gates {M.LSD_REL_GATE:.0e}, {M.MEL_GATE:.0e}, {M.DB_GATE:.0e}")
    # each gate is about 10x the largest yardstick: not below 3x it, not above 30x it
    for got, gate in ((worst["lsd"], M.LSD_REL_GATE), (max(worst["l1"], worst["l2"]), M.MEL_GATE), (worst["db"], M.DB_GATE)):
        assert 3 * got < gate < 30 * got, (got, gate)


def test_exact_zero_band_is_ill_conditioned_for_lsd_only():
    # every bin above 8 kHz exactly zero: LSD takes the log of rounding noise there, so fp32 and fp64 already disagree on
    # the CPU; the mel metrics do not care.  The broadband floor of the parity fixtures removes the disagreement.
    gt = M.test_signal(3 * 44100)[0]
    lr0 = M.brickwall(gt)
    l64, l32 = M.calculate_lsd(lr0, gt)[0], M.calculate_lsd(lr0, gt, dtype=np.float32)[0]
    print(f"exact-zero band: lsd_db fp64 {l64:.2f}, fp32 {l32:.2f}")                  # measured: 98.19, 95.79
    assert abs(l32 - l64) / l64 > 100 * M.LSD_REL_GATE
    r64, r32 = M.calculate_mel_loss(lr0, gt), M.calculate_mel_loss(lr0, gt, dtype=np.float32)
    assert abs(r32[0] - r64[0]) < M.MEL_GATE and abs(r32[1] - r64[1]) < M.MEL_GATE


# ---- command lines -----------------------------------------------------------------------------------------------------------------
def test_metrics_parser_and_grades():
    a = metrics.build_parser().parse_args(["--pred", "a.wav", "--gt", "b.wav"])
    assert (a.pred, a.gt, a.lr, a.json, a.sr) == ("a.wav", "b.wav", None, None, 44100)
    a = metrics.build_parser().parse_args(["--pred", "a.wav", "--gt", "b.wav", "--lr", "c.wav", "--json", "o.json"])
    assert (a.lr, a.json) == ("c.wav", "o.json")
    with pytest.raises(SystemExit):
        metrics.build_parser().parse_args(["--pred", "a.wav"])
    assert [metrics.lsd_grade(v) for v in (0.5, 1.2, 1.7, 2.2, 13.08)] == ["Excellent", "Very Good", "Good", "Fair", "Poor"]
    assert [metrics.mel_grade(v) for v in (2.0, 4.30, 6.0, 9.0)] == ["Excellent", "Very Good", "Good", "Fair"]
    rep = {"generated": dict(M.evaluate_pair(M.degraded(M.test_signal(8000)[0]), M.test_signal(8000)[0])),
           "lsd_grade": "Poor", "mel_grade": "Excellent"}
    text = metrics.format_report(rep)
    assert text.isascii() and "LSD (dB)" in text and "Multi-Scale L2 (dB)" in text and "fft512" in text
    low = dict(rep["generated"], lsd=2 * rep["generated"]["lsd"])
    rep.update(lr_input=low, improvement={k: {"abs": low[k] - rep["generated"][k], "rel": 1 - rep["generated"][k] / low[k]}
                                          for k in metrics.METRIC_KEYS})
    text = metrics.format_report(rep)
    assert text.isascii() and "LR vs GT" in text and "(50.0%)" in text


@pytest.mark.parametrize("module,needle", [("jatsr_amd.metrics", "--pred"), ("jatsr_amd.infer", "--metrics")])
def test_help_of_both_tools(module, needle):
    out = subprocess.run([sys.executable, "-m", module, "--help"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and needle in out.stdout, out.stdout + out.stderr


def test_infer_refuses_metrics_without_a_ground_truth(tmp_path):
    from jatsr_amd import infer
    assert infer.build_parser().parse_args([]).metrics is False
    base = ["--checkpoint", str(tmp_path / "none.pt"), "--output-dir", str(tmp_path / "o"), "--metrics"]
    for extra in ([],                                                                   # no --dac-weights: nothing is decoded
                  ["--input-audio", "x.wav", "--dac-weights", "dac.pt"],                  # audio in, no HR recording
                  ["--input-audio", "x.wav", "--dac-weights", "dac.pt", "--resample"]):
        with pytest.raises(SystemExit, match="--metrics"):
            infer.main(base + extra)
    assert not (tmp_path / "o").exists()
