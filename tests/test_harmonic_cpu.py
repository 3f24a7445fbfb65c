"""Host side of the harmonic analysis, template and comparison, no GPU: the entry points are declared in
include/jat_hip_harm.h (and nowhere in include/jat_hip.h), bound in `_lib.HARM_SIGNATURES` and exported from both libraries; the
Makefile lines; every argument refusal of the library, which comes before any device call; the Python refusals; and the fp64
reference of tests/harmonic_ref.py against closed forms: a tone with whole cycles per frame, the guard, the integer phase, and
the round trip analyze(synthesize(f0, amp)) on a constant f0.

The round trip's limit: harmonics must be at least about four bins apart (f0 >= 4 sr / N).  At 55 Hz (2.6 bins apart, H = 64)
the worst relative error of the same flat fixture is 4.5e-2, with amplitudes 1 / h 6e-2 (measured with harmonic_ref.round_trip);
that is the documented limit of the analysis, not a test.  The four fixtures come out at 1.4e-3, 3.3e-4, 6.9e-5 and 1.7e-4."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import harmonic_ref as HR
import jatsr_amd
from jatsr_amd import _lib, infer, prepare
from jatsr_amd import harmonic as HM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jatsr-just-audio-transformer-super-solution_amd", "csrc")
SYMBOLS = ("jat_harmonic_analyze", "jat_harmonic_synth_workspace_bytes", "jat_harmonic_synth", "jat_harmonic_compare")
INV = _lib.JAT_E_INVALID
P = 4096          # a non-null address that is never read: every refusal comes before a launch


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


# ---- symbols ------------------------------------------------------------------------------------------------------------
def test_symbols_declared_bound_and_exported(built):
    header = open(os.path.join(ROOT, "include", "jat_hip_harm.h")).read()
    old = open(os.path.join(ROOT, "include", "jat_hip.h")).read() + open(os.path.join(ROOT, "include", "jat_hip_ms.h")).read()
    assert '#include "jat_hip.h"' in header
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.HARM_SIGNATURES and name not in _lib.SIGNATURES and name not in _lib.MS_SIGNATURES, name
        assert name not in old, name
        assert getattr(built, name).argtypes == _lib.HARM_SIGNATURES[name][1]
    assert set(re.findall(r"\bint (jat_[a-z0-9_]+)\(", header)) == set(_lib.HARM_SIGNATURES) == set(SYMBOLS)
    assert int(re.search(r"#define JAT_HARM_MAX (\d+)", header).group(1)) == _lib.HARM_MAX == 128
    assert [len(_lib.HARM_SIGNATURES[n][1]) for n in SYMBOLS] == [13, 4, 14, 11]
    for so in ("libjat_hip.so", "libjat_hip_fp16.so"):
        nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(CSRC, so)], capture_output=True, text=True,
                            check=True).stdout
        exported = set(re.findall(r" T (jat_[a-z0-9_]+)", nm))
        assert set(SYMBOLS) <= exported, (so, set(SYMBOLS) - exported)
    for name in ("harmonic_metrics", "generate_harmonics"):
        assert name in jatsr_amd.__all__
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "OBJS += harmonic.o jat_harmonic.o\n" in mk and "FP16OBJS += harmonic_fp16.o jat_harmonic_fp16.o\n" in mk
    assert mk.count("../../include/jat_hip_harm.h") == 2              # the two %.cpp pattern rules
    assert mk.count("jat_harmonic_kernels.h") == 4                    # every pattern rule


def test_parsers():
    a = infer.build_parser().parse_args([])
    assert a.harmonic_metrics is False
    assert infer.build_parser().parse_args(["--harmonic-metrics"]).harmonic_metrics is True
    base = ["--source-dir", "s", "--output-dir", "o", "--dac-weights", "w"]
    assert prepare.build_parser().parse_args(base).harmonics == 0
    assert prepare.build_parser().parse_args(base + ["--f0", "--harmonics", "8"]).harmonics == 8
    h = HM.build_parser().parse_args(["--pred", "a.wav", "--gt", "b.wav"])
    assert (h.n_harmonics, h.method, h.cutoff_hz, h.template, h.lr) == (64, "yin", None, None, None)


# ---- refusals, all reached without a GPU --------------------------------------------------------------------------------
def test_analyze_refusals(built):
    fn = built.jat_harmonic_analyze

    def call(x=P, B=2, L=1000, f0=P, voiced=P, frames=None, H=8, sr=44100, N=256, hop=64, amp=P, energy=P):
        frames = 1 + L // max(hop, 1) if frames is None else frames
        return fn(x, B, L, f0, voiced, frames, H, sr, N, hop, amp, energy, None)
    for bad in (dict(H=0), dict(H=129), dict(H=-1), dict(N=14), dict(N=8194), dict(N=255), dict(N=0), dict(hop=0), dict(hop=-3),
                dict(frames=15), dict(frames=17), dict(frames=0), dict(L=0), dict(L=-5), dict(B=0), dict(B=65536), dict(sr=0),
                dict(x=None), dict(f0=None), dict(voiced=None), dict(amp=None),
                dict(L=2 ** 31 * 4, hop=4), dict(L=2 ** 31, hop=1, H=1), dict(L=2 ** 26, hop=1, H=128)):
        assert call(**bad) == INV, bad
        assert built.jat_last_error()
    assert "fit 31 bits" in (call(L=2 ** 26, hop=1, H=128), built.jat_last_error().decode())[1]


def test_synth_refusals(built):
    fn, wb = built.jat_harmonic_synth, built.jat_harmonic_synth_workspace_bytes
    need = C.c_size_t()
    assert wb(2, 1000, 64, C.byref(need)) == 0 and need.value == 2 * 16 * 4
    assert wb(1, 1, 512, C.byref(need)) == 0 and need.value == 4
    for bad in ((0, 1000, 64), (65536, 1000, 64), (2, 0, 64), (2, 1000, 0), (1, 2 ** 33, 1)):
        assert wb(*bad, C.byref(need)) == INV, bad
    assert wb(2, 1000, 64, None) == INV

    def call(f0=P, voiced=P, amp=P, B=2, frames=None, H=8, L=1000, sr=44100, hop=64, y=P, phase=None, work=P, bytes_=128):
        frames = 1 + L // max(hop, 1) if frames is None else frames
        return fn(f0, voiced, amp, B, frames, H, L, sr, hop, y, phase, work, bytes_, None)
    for bad in (dict(H=0), dict(H=129), dict(hop=0), dict(frames=15), dict(frames=17), dict(L=0), dict(B=0), dict(B=65536),
                dict(sr=0), dict(sr=-1), dict(f0=None), dict(voiced=None), dict(amp=None), dict(y=None), dict(work=None),
                dict(bytes_=127), dict(bytes_=0), dict(work=P + 2), dict(L=2 ** 33, hop=2), dict(L=2 ** 26, hop=1, H=128)):
        assert call(**bad) == INV, bad


def test_compare_refusals(built):
    fn = built.jat_harmonic_compare

    def call(a=P, r=P, f0=P, v=P, B=2, frames=10, H=8, cutoff=4000.0, floor=1e-5, out=P):
        return fn(a, r, f0, v, B, frames, H, cutoff, floor, out, None)
    for bad in (dict(H=0), dict(H=129), dict(frames=0), dict(B=0), dict(B=65536), dict(cutoff=-1.0), dict(cutoff=float("nan")),
                dict(floor=0.0), dict(floor=-1.0), dict(floor=float("inf")), dict(floor=float("nan")), dict(a=None), dict(r=None),
                dict(f0=None), dict(v=None), dict(out=None), dict(frames=2 ** 24, H=128)):
        assert call(**bad) == INV, bad


def test_python_refusals():
    x, f0, v = torch.zeros(1000), torch.full((16,), 100.0), torch.ones(16, dtype=torch.uint8)
    amp = torch.zeros(16, 4)
    with pytest.raises(_lib.JatError, match="CUDA"):
        HM.analyze(x, f0, v)
    with pytest.raises(_lib.JatError, match="CUDA"):
        HM.synthesize(f0, v, amp, 1000)
    with pytest.raises(_lib.JatError, match="CUDA"):
        HM.generate_harmonics(f0)
    with pytest.raises(_lib.JatError, match="CUDA"):
        HM.compare(amp, amp, f0, v)
    with pytest.raises(_lib.JatError, match="CUDA"):
        HM.harmonic_metrics(x, x)
    with pytest.raises(ValueError, match="method"):
        HM.reference_track(x, method="crepe")
    with pytest.raises(TypeError, match="n_thresholds"):
        HM.reference_track(x, method="yin", n_thresholds=50)                    # an argument of the other tracker
    with pytest.raises(TypeError, match="unknown"):
        HM.reference_track(x, method="yin", window="hann")


def test_report_arithmetic():
    row = [2.0, -4.0, 10.0, 4.0, 3.0, 6.0, 30.0, 9.0]
    rep = HM.report_from_sums(row, True)
    assert rep["kept"] == {"n_cells": 2, "bias_db": -2.0, "rms_db": 5.0 ** 0.5, "mean_abs_db": 2.0}
    assert rep["regenerated"] == {"n_cells": 3, "bias_db": 2.0, "rms_db": 10.0 ** 0.5, "mean_abs_db": 3.0}
    assert rep["all"] == {"n_cells": 5, "bias_db": 0.4, "rms_db": 8.0 ** 0.5, "mean_abs_db": 2.6}
    assert sorted(HM.report_from_sums(row, False)) == ["all"]
    assert HM.band_from_sums([0, 0, 0, 0]) == {"n_cells": 0, "bias_db": 0.0, "rms_db": 0.0, "mean_abs_db": 0.0}
    assert HR.band_report(np.array(row[:4])) == rep["kept"]
    amp, energy = torch.tensor([[0.5, 0.25], [1.0, 0.0]]), torch.tensor([0.0, 2048 * 0.375 * 0.5])
    assert HM.harmonicity(amp, energy).tolist() == [0.0, 1.0]


# ---- the reference against closed forms -----------------------------------------------------------------------------------
def test_phase_arithmetic():
    sr = 44100
    assert HR.turns(np.array([0.0, sr / 4.0, sr / 8.0]), sr).tolist() == [0, 2 ** 30, 2 ** 29]
    assert HR.turns(220.0, sr) == np.uint32(round(220.0 / sr * 2 ** 32))
    a = HR.angle(np.array([0, 2 ** 30, 2 ** 31, 2 ** 32 - 2 ** 30], np.uint32))
    assert np.allclose(a, [0.0, np.pi / 2, -np.pi, -np.pi / 2], rtol=0, atol=1e-15) and (a >= -np.pi).all() and (a < np.pi).all()
    big = HR.angle(np.array([2 ** 31 - 1], np.uint32))              # float(int32) rounds up to 2^31: the angle stays in range
    assert big[0] == np.pi
    # the prefix is numpy's uint32 cumulative sum, whatever the split
    f0 = np.array([3000.0, 9000.0, 0.0, 15000.0, 4000.0], np.float32)
    t = HR.synth_track(f0, np.ones(5, np.uint8), sr, 100, 450)
    assert t["phase"][0] == 0 and np.array_equal(t["phase"][1:], np.cumsum(t["inc"].astype(np.uint64))[:-1] % 2 ** 32)
    assert (np.cumsum(t["inc"].astype(np.uint64)) > 2 ** 32).any()                   # it wrapped
    # one-voiced-neighbour rule: frame 2 is unvoiced (f0 = 0), so frames 1 and 2 hold their voiced neighbour's f0
    assert (t["f0n"][100:200] == 9000.0).all() and (t["f0n"][200:300] == 15000.0).all()
    assert t["f0n"][50] == 0.5 * 3000.0 + 0.5 * 9000.0 and t["f0n"][449] == 4000.0   # interpolation; the last frame clamped


def test_whole_cycles_give_the_amplitude():
    sr, N, hop = 32768, 256, 64                                     # sr / N = 128 Hz a bin: every f0 below is a whole bin
    L = hop * 12
    n = np.arange(L)
    for k, a, ph in ((8, 0.5, 0.3), (20, 0.125, 2.0), (3, 1.0, 0.0)):
        f0_hz = k * sr / N
        x = a * np.cos(2 * np.pi * f0_hz * n / sr + ph)
        f0 = np.full(13, f0_hz, np.float32)
        r = HR.analyze(x, f0, np.ones(13, np.uint8), 1, sr, N, hop)
        inner = r["amp"][2:-2, 0]                                   # frames without padding
        # fp64 rounding: the window is the fp32-rounded one (its error cancels in c / sum w only to 1e-8), the phases
        # float(int32) (an angle error of at most pi 2^-24)
        assert np.abs(inner - a).max() <= 4e-7 * a, (k, np.abs(inner - a).max())
        assert np.abs(r["energy"][2:-2] - a * a * 0.5 * 0.375 * N).max() <= 1e-6 * a * a * N
        assert np.abs(HR.harmonicity(r["amp"], r["energy"], N)[2:-2] - 1.0).max() <= 2e-6


def test_whole_cycles_exact_window():
    """with the fp64 window and exact phases (f0 a whole bin: s n is a multiple of 2^32 / N, float() is exact) amp = a to rounding"""
    sr, N = 32768, 256
    n = np.arange(N)
    w = 0.5 - 0.5 * np.cos(2 * np.pi * n / N)
    for k, a in ((8, 0.5), (20, 0.125)):
        x = a * np.cos(2 * np.pi * k * n / N + 0.7)
        s = HR.turns(k * sr / N, sr)
        assert int(s) == k * 2 ** 32 // N
        ang = HR.angle(s * n.astype(np.uint32))
        c = np.sum(w * x * np.exp(-1j * ang))
        assert abs(2 * abs(c) / w.sum() - a) <= 1e-14


def test_guard_and_unvoiced_give_zero():
    sr, N, hop, H = 44100, 2048, 512, 64
    x = HR.case_signal(1, hop * 6, 0)[0]
    f0 = np.array([400.0, 400.0, 0.0, np.nan, 343.0, np.inf, -50.0], np.float32)
    voiced = np.array([1, 0, 1, 1, 1, 1, 1], np.uint8)
    r = HR.analyze(x, f0, voiced, H, sr, N, hop)
    limit = sr / 2 - 2 * sr / N
    assert r["live"][0].sum() == int(np.floor(limit / 400.0)) == 55 and not r["live"][[1, 2, 3, 5, 6]].any()
    assert r["live"][4].sum() == 64 and 64 * 343.0 < limit < 65 * 343.0
    assert (r["amp"][~r["live"]] == 0).all() and (r["amp"][r["live"]] > 0).all() and (r["energy"] > 0).all()
    # synthesis drops what reaches Nyquist: at f0 = 4000 Hz only h = 1 .. 5 sound
    f0s = np.full(3, 4000.0, np.float32)
    amp = np.ones((3, 8), np.float32)
    s = HR.synthesize(f0s, np.ones(3, np.uint8), amp, sr, 64, 128)
    assert np.allclose(s["absum"], 5.0)
    s2 = HR.synthesize(f0s, np.ones(3, np.uint8), amp[:, :5], sr, 64, 128)
    assert np.array_equal(s["y"], s2["y"])


@pytest.mark.parametrize("f0_hz,H", HR.ROUND_TRIP)
def test_round_trip_on_a_constant_f0(f0_hz, H):
    worst, live = HR.round_trip(f0_hz, H)
    print(f"round trip {f0_hz} Hz, H = {H}: worst relative error {worst:.2e} over {int(live.sum())} live cells")
    assert live.all() and live.shape[1] == H
    assert worst <= 2e-3


def test_compare_reference():
    f0 = np.array([100.0, 200.0, 0.0, 100.0], np.float32)
    voiced = np.array([1, 1, 1, 0], np.uint8)
    ref = np.array([[1.0, 0.5, 1e-7], [1.0, 1.0, 1.0], [1.0, 1.0, 1.0], [1.0, 1.0, 1.0]], np.float32)
    a = ref * np.float32(0.5)
    out = HR.compare(a, ref, f0, voiced, 200.0, 1e-5)
    # kept: (0, h = 1) only (h f0 = 100); h f0 = 200 lies ON the cutoff and is regenerated; (0, 3) is under the floor
    assert out[0] == 1 and out[4] == 1 + 3
    e = 20 * np.log10((0.5 + 1e-5) / (1 + 1e-5))
    assert abs(out[1] - e) < 1e-12 and abs(out[5] - (3 * e + 20 * np.log10((0.25 + 1e-5) / (0.5 + 1e-5)))) < 1e-12
    assert np.array_equal(HR.compare(a, ref, f0, voiced, np.inf, 1e-5)[4:], np.zeros(4))
