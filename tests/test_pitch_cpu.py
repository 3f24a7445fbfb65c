"""The pitch tracker without a GPU: the fp64 statement (tests/pitch_ref.py) against a brute-force double loop, on a pure tone
and on zeros; the fp32 statement against the fp64 one on the very signals the GPU tests use (so those inputs are known to
stay inside the GPU test's 1 % cap on differing decisions); the period range of the library against the Python formula; the
parser, the refusals and the report arithmetic of jatsr_amd.pitch."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pitch_ref as P  # noqa: E402
import jatsr_amd._lib as L  # noqa: E402
import jatsr_amd.pitch as pitch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_against_a_double_loop_on_one_frame():
    sr, fl, hop = 8000, 64, 16
    x = P.mix(sr, 400, 5, fl)
    lo, hi = P.periods(sr, 150.0, 1500.0, fl)
    assert (lo, hi) == (5, 31)                       # ceil(8000 / 150) = 54 is capped at frame_length - W - 1
    r = P.yin(x, sr, 150.0, 1500.0, fl, hop, 0.1)
    f = 7
    xp = np.concatenate([np.zeros(fl // 2), x.astype(np.float64), np.zeros(fl // 2)])[f * hop:f * hop + fl]
    W = fl // 2
    d = [0.0]
    for tau in range(1, hi + 1):
        s = 0.0
        for j in range(W):
            s += (xp[j] - xp[j + tau]) ** 2
        d.append(s)
    c = [1.0] + [d[t] / (sum(d[1:t + 1]) / t + P.TINY) for t in range(1, hi + 1)]
    assert np.allclose(r["d"][f], d, rtol=1e-13, atol=0) and np.allclose(r["cmndf"][f], c, rtol=1e-13, atol=0)
    y = c[lo:]
    thr = float(np.float32(0.1))
    troughs = [i for i in range(len(y) - 1) if (y[i] < y[i + 1] if i == 0 else (y[i] < y[i - 1] and y[i] <= y[i + 1]))]
    under = [i for i in troughs if y[i] < thr]
    k = under[0] if under else int(np.argmin(y))
    assert r["index"][f] == k and bool(r["voiced"][f]) == bool(under) and r["aperiodicity"][f] == r["cmndf"][f][lo + k]
    sh = 0.0
    if 0 < k < len(y) - 1:
        a, b = y[k + 1] + y[k - 1] - 2 * y[k], (y[k + 1] - y[k - 1]) / 2
        sh = -b / a if abs(b) < abs(a) else 0.0
    assert np.isclose(r["f0"][f], sr / (lo + k + sh), rtol=1e-12)


def test_pure_tone_at_a_non_integer_period():
    """period 44100 / 317.3 = 138.99 samples: the parabola through three samples of a near-quadratic dip recovers it to well
    under a cent on the frames that lie wholly inside the tone"""
    sr, f = 44100, 317.3
    x = (0.5 * np.sin(2 * np.pi * f * np.arange(3 * 4096) / sr)).astype(np.float32)
    r = P.yin(x, sr)
    inner = slice(2, -3)                             # frames that do not reach into the zero padding
    assert r["voiced"][inner].all() and (r["aperiodicity"][inner] < 1e-3).all()
    assert np.abs(P.cents(r["f0"][inner], f)).max() < 0.5
    assert (np.abs(r["index"][inner] + P.periods(sr, 50.0, 1000.0, 2048)[0] - sr / f) <= 1).all()


def test_zeros_are_unvoiced():
    for dtype in (np.float64, np.float32):
        r = P.yin(np.zeros(5000, np.float32), dtype=dtype)
        assert not r["voiced"].any() and (r["cmndf"][:, 1:] == 0).all() and (r["index"] == 0).all()
        assert (r["aperiodicity"] == 0).all() and np.allclose(r["f0"], 44100 / 44)


@pytest.mark.parametrize("name", sorted(P.CASES))
def test_fp32_statement_decides_as_fp64_on_the_gpu_test_signals(name):
    """the inputs of tests/test_pitch_gpu.py stay inside its cap: the fp32 statement differs from fp64 on at most 1 % of the
    frames (0 where this was written), and its d, cmndf and f0 errors are the yardsticks the GPU gates are derived against"""
    sr, fl, hop, fmin, fmax, n, seeds, thr = P.CASES[name]
    x, r64, r32 = P.case(name)
    assert x.shape == (len(seeds), n) and x.dtype == np.float32
    W, (lo, hi) = fl // 2, P.periods(sr, fmin, fmax, fl)
    for a, b in zip(r64, r32):
        frames = 1 + n // hop
        assert a["index"].shape == (frames,) and a["d"].shape == (frames, hi + 1)
        differ = int(((a["index"] != b["index"]) | (a["voiced"] != b["voiced"])).sum())
        same = a["index"] == b["index"]
        rel_d = float((np.abs(b["d"] - a["d"]) / np.maximum(a["d"], 1e-300)).max())
        rel_c = float((np.abs(b["cmndf"] - a["cmndf"]) / np.maximum(a["cmndf"], 1e-300)).max())
        worst = float(np.abs(P.cents(b["f0"][same], a["f0"][same])).max())
        print(f"{name}: frames {frames}, voiced {int(a['voiced'].sum())}, differ {differ}, d {rel_d:.2e}, cmndf {rel_c:.2e}, "
              f"cents {worst:.2e}")
        assert differ <= 0.01 * frames
        assert rel_d <= (W + 2) * 2.0 ** -24 and rel_c <= (2 * (W + 2) + hi + 4) * 2.0 ** -24
        if n >= fl:
            assert 0 < a["voiced"].sum() < frames          # the signal has voiced and unvoiced stretches


def test_period_range_of_the_library_against_the_formula():
    lib = L.lib()
    lo, hi = C.c_int32(), C.c_int32()
    n = 0
    for sr in (8000, 16000, 44100, 48000):
        for fl in (16, 64, 1024, 2048, 4096, 8192):
            for fmin, fmax in ((50.0, 1000.0), (43.0, 2000.0), (30.0, 1200.0), (20.0, 3999.9), (400.0, 401.0), (0.5, 100.0)):
                want = P.periods(sr, fmin, fmax, fl)
                rc = lib.jat_yin_periods(sr, fmin, fmax, fl, C.byref(lo), C.byref(hi))
                if fmax >= sr / 2 or want[1] - want[0] < 2:
                    assert rc == L.JAT_E_INVALID, (sr, fl, fmin, fmax)
                else:
                    assert rc == 0 and (lo.value, hi.value) == want, (sr, fl, fmin, fmax)
                    n += 1 + (want[1] == fl - fl // 2 - 1)
    assert n > 60
    assert pitch.periods(44100, 43.0, 2000.0, 2048) == (22, 1023)          # the cap frame_length - W - 1
    assert pitch.periods() == (44, 882)
    for bad in ((0, 50.0, 1000.0, 2048), (44100, 50.0, 1000.0, 2047), (44100, 50.0, 1000.0, 14), (44100, 50.0, 1000.0, 8194),
                (44100, 0.0, 1000.0, 2048), (44100, -1.0, 1000.0, 2048), (44100, 50.0, 50.0, 2048), (44100, 50.0, 22050.0, 2048),
                (44100, float("nan"), 1000.0, 2048), (44100, 50.0, float("nan"), 2048), (44100, 20000.0, 22000.0, 2048)):
        assert lib.jat_yin_periods(*bad, C.byref(lo), C.byref(hi)) == L.JAT_E_INVALID, bad
        assert lib.jat_last_error()
    assert lib.jat_yin_periods(44100, 50.0, 1000.0, 2048, None, C.byref(hi)) == L.JAT_E_INVALID


def test_parser_and_refusals():
    a = pitch.build_parser().parse_args(["--pred", "a.wav", "--gt", "b.wav"])
    assert (a.sr, a.fmin, a.fmax, a.frame_length, a.hop_length, a.trough_threshold, a.gross_cents) == \
        (44100, 50.0, 1000.0, 2048, 512, 0.1, 50.0) and a.lr is None and a.json is None and a.track is None
    with pytest.raises(SystemExit):
        pitch.build_parser().parse_args(["--pred", "a.wav"])
    out = subprocess.run([sys.executable, "-m", "jatsr_amd.pitch", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "--track" in out.stdout and "--gt" in out.stdout, out.stdout + out.stderr
    x = torch.zeros(4096)
    with pytest.raises(L.JatError, match="no CPU path"):
        pitch.yin(x)
    with pytest.raises(L.JatError, match="no CPU path"):
        pitch.f0_metrics(x, x)
    with pytest.raises(L.JatError, match="no CPU path"):
        pitch.compare_f0(x, x > 0, x, x > 0)
    with pytest.raises(L.JatError, match=r"\[L\] or \[B, L\]"):
        pitch.yin(np.zeros(16, np.float32))
    with pytest.raises(ValueError, match="integer"):
        pitch.periods(44100.5)
    with pytest.raises(ValueError, match="frame_length"):
        pitch.periods(frame_length=2047)
    with pytest.raises(ValueError, match="fmax"):
        pitch.periods(fmax=30000.0)


def test_infer_and_prepare_flags_parse_and_default_off():
    from jatsr_amd import infer, prepare
    assert infer.build_parser().parse_args([]).f0_metrics is False
    assert infer.build_parser().parse_args(["--f0-metrics"]).f0_metrics is True
    base = ["--source-dir", "w", "--output-dir", "o", "--dac-weights", "d.pt"]
    assert prepare.build_parser().parse_args(base).f0 is False and prepare.build_parser().parse_args(base + ["--f0"]).f0 is True


def test_infer_refuses_f0_metrics_without_a_ground_truth(tmp_path):
    from jatsr_amd import infer
    base = ["--checkpoint", str(tmp_path / "none.pt"), "--output-dir", str(tmp_path / "o"), "--f0-metrics"]
    for extra in ([], ["--input-audio", "x.wav", "--dac-weights", "dac.pt"],
                  ["--input-audio", "x.wav", "--dac-weights", "dac.pt", "--resample"]):
        with pytest.raises(SystemExit, match="--f0-metrics"):
            infer.main(base + extra)
    assert not (tmp_path / "o").exists()


def test_report_arithmetic_from_hand_made_counts():
    r = pitch.report_from_counts([80.0, 60.0, 25.0, 6.0, 900.0, 108.0], 200)
    assert r["voicing_error_rate"] == 25 / 200 and r["gross_error_rate"] == 6 / 60 and r["raw_pitch_accuracy"] == 54 / 80
    assert r["mean_abs_cents"] == 900 / 60 and r["fine_mean_abs_cents"] == 108 / 54
    assert [r[k] for k in pitch.COUNT_KEYS] == [200, 80, 60, 25, 6] and all(isinstance(r[k], int) for k in pitch.COUNT_KEYS)
    assert set(r) == set(pitch.COUNT_KEYS) | set(pitch.RATE_KEYS)
    z = pitch.report_from_counts([0.0, 0.0, 3.0, 0.0, 0.0, 0.0], 10)       # no voiced frame: no division by zero
    assert z["voicing_error_rate"] == 0.3 and all(z[k] == 0.0 for k in pitch.RATE_KEYS[1:])
    g = pitch.report_from_counts([5.0, 5.0, 0.0, 5.0, 6000.0, 0.0], 5)      # all gross
    assert g["gross_error_rate"] == 1.0 and g["raw_pitch_accuracy"] == 0.0 and g["fine_mean_abs_cents"] == 0.0
    # the numpy statement of the counts on a hand-made pair
    f_ref = np.array([100.0, 200.0, 300.0, 400.0, 0.0], np.float32)
    f_a = np.array([100.0, 200.0 * 2 ** (25 / 1200), 600.0, 123.0, 50.0], np.float32)
    c = P.compare_counts(f_a, [1, 1, 1, 0, 1], f_ref, [1, 1, 1, 1, 0])
    assert list(c[:4]) == [4, 3, 2, 1] and np.isclose(c[4], 1225.0, rtol=1e-6) and np.isclose(c[5], 25.0, rtol=1e-5)
    text = pitch.format_report({"generated": r, "lr_input": g})
    assert text.isascii() and "Raw pitch accuracy" in text and "80/200" in text
