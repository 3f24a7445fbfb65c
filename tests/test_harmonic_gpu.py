"""Harmonic analysis, template and comparison on the GPU (jat_harmonic_analyze, jat_harmonic_synth,
jat_harmonic_compare, jatsr_amd.harmonic) against the fp64 statement of tests/harmonic_ref.py.

What is exact: the live mask, the synthesis phase (numpy's uint32 cumulative sum, bit for bit), the comparison's counts, and
every output from run to run, for a row alone or in a batch, and on a common prefix of two lengths.  What is bounded, with bounds
derived in tests/harmonic_ref.py from the kernels' summation order (not from what the kernels give):
    |amp - ref|    <= analyze_gamma(N) sum|w x| / sum w          |energy - ref| <= energy_gamma(N) ref
    |y - ref|      <= (13 + H) 2^-24 sum_h |a_h(n)|              on the GPU's own (= the reference's) phases
Each test prints the worst ratio to its bound.  Named test_harmonic_gpu.py, not test_gpu_*.py, as tests/test_pitch_gpu.py explains."""
import ctypes as C
import functools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import harmonic_ref as HR  # noqa: E402
import jatsr_amd._lib as L  # noqa: E402
import jatsr_amd.harmonic as HM  # noqa: E402
import jatsr_amd.io as jio  # noqa: E402
from stream_check import Case, check_case  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV = L.JAT_E_INVALID
SR = HR.SR
IDS = [f"B{b}-L{n}-N{N}-hop{hop}-H{H}" for b, n, N, hop, H in HR.SHAPES]


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ---- 1. analysis ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def analysis_case(i):
    B, n, N, hop, H = HR.SHAPES[i]
    frames = HR.frames_of(n, hop)
    f0, voiced = HR.case_track(B, frames, H, SR, N, salt=i)
    x = HR.case_signal(B, n, salt=i)
    ref = [HR.analyze(x[b], f0[b], voiced[b], H, SR, N, hop) for b in range(B)]
    return x, f0, voiced, {k: np.stack([r[k] for r in ref]) for k in ref[0]}


@pytest.mark.parametrize("i", range(len(HR.SHAPES)), ids=IDS)
def test_analysis_within_the_derived_bound(i):
    B, n, N, hop, H = HR.SHAPES[i]
    x, f0, voiced, ref = analysis_case(i)
    amp, energy = HM.analyze(cuda(x), cuda(f0), cuda(voiced), n_harmonics=H, sr=SR, frame_length=N, hop_length=hop)
    amp, energy = amp.cpu().numpy(), energy.cpu().numpy()
    assert amp.shape == (B, HR.frames_of(n, hop), H) and energy.shape == amp.shape[:2]
    assert np.isfinite(amp).all() and np.isfinite(energy).all()
    live = ref["live"]
    if i in (1, 2):                                               # the fixtures reach every kind of cell
        assert live.any() and (~live[voiced != 0]).any() and (voiced == 0).any()
        assert (live.any(axis=2) & ~live.all(axis=2)).any()       # a frame whose harmonics cross the guard inside the table
    assert np.array_equal(amp != 0, live), "the live mask differs from the reference's"
    assert (amp[~live] == 0).all()
    sumw = HR.window(N).astype(np.float64).sum()
    bound = HR.analyze_gamma(N) * ref["absum"][:, :, None] / sumw
    err = np.abs(amp.astype(np.float64) - ref["amp"])
    ratio = float((err / np.maximum(bound, 1e-300))[live].max()) if live.any() else 0.0
    e_err = np.abs(energy.astype(np.float64) - ref["energy"])
    e_ratio = float((e_err / np.maximum(HR.energy_gamma(N) * ref["energy"], 1e-300)).max())
    rel = float((err[live] / ref["amp"][live]).max()) if live.any() else 0.0
    print(f"analysis {IDS[i]}: worst |amp - ref| / bound {ratio:.3f} (relative {rel:.2e}), energy {e_ratio:.3f}")
    assert (err <= bound).all() and (e_err <= HR.energy_gamma(N) * ref["energy"]).all()


# ---- 2. synthesis ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def synth_case(i):
    B, n, N, hop, H = HR.SHAPES[i]
    frames = HR.frames_of(n, hop)
    f0, voiced = HR.case_track(B, frames, H, SR, N, salt=10 + i, glide=True)
    amp = HR.case_amp(B, frames, H, salt=i)
    ref = [HR.synthesize(f0[b], voiced[b], amp[b], SR, hop, n) for b in range(B)]
    return f0, voiced, amp, {k: np.stack([r[k] for r in ref]) for k in ref[0]}


def raw_synth(f0, voiced, amp, n, hop, sr=SR, guard=64, want_phase=True, work_bytes=None):
    """through the ABI with guard bands behind y and phase -> (rc, y [B, n], phase, y guard, phase guard)"""
    B, frames, H = amp.shape
    y = torch.full((B * n + guard,), 7.0, device="cuda")
    ph = torch.full((B * n + guard,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    need = C.c_size_t()
    assert L.lib().jat_harmonic_synth_workspace_bytes(B, n, hop, C.byref(need)) == 0
    work = torch.zeros(need.value, dtype=torch.uint8, device="cuda")
    rc = L.lib().jat_harmonic_synth(L.ptr(f0), L.ptr(voiced), L.ptr(amp), B, frames, H, n, sr, hop, L.ptr(y),
                                    L.ptr(ph) if want_phase else None, L.ptr(work),
                                    need.value if work_bytes is None else work_bytes, L.stream_ptr())
    torch.cuda.synchronize()
    return rc, y[:B * n].reshape(B, n), ph[:B * n].reshape(B, n), y[B * n:], ph[B * n:]


@pytest.mark.parametrize("i", range(len(HR.SHAPES)), ids=IDS)
def test_synthesis_phase_is_exact_and_y_within_the_derived_bound(i):
    B, n, N, hop, H = HR.SHAPES[i]
    f0, voiced, amp, ref = synth_case(i)
    rc, y, ph, yg, pg = raw_synth(cuda(f0), cuda(voiced), cuda(amp), n, hop)
    assert rc == 0
    assert (yg == 7.0).all() and (pg == 0x5A5A5A5A).all(), "a sample beyond L was written"
    assert np.array_equal(u32(ph), ref["phase"]), "the phase is not numpy's uint32 cumulative sum"
    if i == 2:
        v = HR.is_voiced(f0, voiced)
        assert (v[:, :-1] & ~v[:, 1:]).any() and (~v[:, :-1] & v[:, 1:]).any() and (ref["f0n"] == 0).any()
        assert (H * ref["f0n"] >= SR / 2.0).any()                                   # harmonics cross Nyquist inside the table
    if i >= 2:
        inc = np.stack([HR.synth_track(f0[b], voiced[b], SR, hop, n)["inc"] for b in range(B)])
        assert (inc.astype(np.uint64).sum(axis=1) > 2 ** 32).all()                  # the phase wrapped
    y = y.cpu().numpy()
    assert np.isfinite(y).all()
    bound = HR.synth_bound(H, ref["absum"])
    err = np.abs(y.astype(np.float64) - ref["y"])
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    print(f"synthesis {IDS[i]}: worst |y - ref| / bound {ratio:.3f}")
    assert (err <= bound).all()
    assert (y[~pos] == 0).all()                                                     # silence where nothing is voiced
    got = HM.synthesize(cuda(f0), cuda(voiced), cuda(amp), n, sr=SR, hop_length=hop)
    assert same_bits(got, cuda(y))


def test_terms_at_or_above_nyquist_are_absent():
    hop, n = 64, 64 * 4 + 5
    frames = HR.frames_of(n, hop)
    f0 = cuda(np.full((1, frames), 4000.0, np.float32))                             # h = 6 is 24 kHz
    voiced = torch.ones(1, frames, dtype=torch.uint8, device="cuda")
    amp = cuda(np.full((1, frames, 8), 0.1, np.float32))
    y8 = HM.synthesize(f0, voiced, amp, n, hop_length=hop)
    y5 = HM.synthesize(f0, voiced, amp[:, :, :5].contiguous(), n, hop_length=hop)
    y4 = HM.synthesize(f0, voiced, amp[:, :, :4].contiguous(), n, hop_length=hop)
    assert same_bits(y8, y5) and not same_bits(y5, y4)
    # exactly at Nyquist: sr = 48000, f0 = 6000, h = 4 is 24000 = sr / 2 and is dropped, h = 3 is kept
    f6 = cuda(np.full((1, frames), 6000.0, np.float32))
    a = HM.synthesize(f6, voiced, amp[:, :, :4].contiguous(), n, sr=48000, hop_length=hop)
    b = HM.synthesize(f6, voiced, amp[:, :, :3].contiguous(), n, sr=48000, hop_length=hop)
    c = HM.synthesize(f6, voiced, amp[:, :, :2].contiguous(), n, sr=48000, hop_length=hop)
    assert same_bits(a, b) and not same_bits(b, c)
    # the analysis guard: at f0 = 1000 Hz, N = 256 the last live harmonic is h = 21 (21 kHz < 22050 - 344.5 < 22 kHz)
    x = cuda(HR.case_signal(1, n, 5))
    amp_a, _ = HM.analyze(x, cuda(np.full((1, frames), 1000.0, np.float32)), voiced, n_harmonics=24, frame_length=256, hop_length=hop)
    assert (amp_a[:, :, :21] > 0).all() and (amp_a[:, :, 21:] == 0).all()


def test_a_term_exactly_at_nyquist_is_dropped_at_a_running_phase():
    """On a constant f0 the phase of a term exactly at Nyquist is a multiple of pi and the term is next to 0 whether it is kept
    or not.  Here f0 glides 5000 -> 7000 Hz at sr = 48000: half way through each hop 4 f0(n) is 24000 = sr / 2 exactly while
    the phase is anything, so a kernel that keeps the term (<= for <) is off by about the term's amplitude, 0.2."""
    sr, hop, n = 48000, 64, 64 * 6 + 9
    frames = HR.frames_of(n, hop)
    f0 = np.tile(np.array([5000.0, 7000.0], np.float32), frames)[None, :frames]
    voiced = np.ones((1, frames), np.uint8)
    amp = np.full((1, frames, 4), 0.2, np.float32)
    ref = HR.synthesize(f0[0], voiced[0], amp[0], sr, hop, n)
    at = 4.0 * ref["f0n"] == sr / 2.0
    assert at.sum() == n // hop                                                     # the sample u = 1 / 2 of every whole hop
    with_it = HR.synthesize(f0[0], voiced[0], amp[0], float(np.nextafter(sr, np.inf)), hop, n)       # what keeping it would give
    assert np.abs(with_it["y"] - ref["y"])[at].max() > 0.05
    rc, y, ph, _, _ = raw_synth(cuda(f0), cuda(voiced), cuda(amp), n, hop, sr=sr)
    assert rc == 0 and np.array_equal(u32(ph)[0], ref["phase"])
    err = np.abs(y.cpu().numpy()[0].astype(np.float64) - ref["y"])
    assert (err <= HR.synth_bound(4, ref["absum"])).all(), float(err.max())


def test_the_harmonic_phase_wraps_in_integers():
    """Only h = 128 sounds: its phase 128 * phase[n] wraps 128 times as often as the fundamental's.  Wrapped as an integer the
    angle is exact before its one rounding; the product 128 * angle(phase) in fp32 instead carries 128 times the rounding of
    float(int32(phase)), up to 128 pi 2^-24 a, 2.8 times this test's bound (13 + 128) 2^-24 a."""
    hop, n, H = 512, 512 * 8 + 77, 128
    frames = HR.frames_of(n, hop)
    f0 = np.linspace(100.0, 140.0, frames).astype(np.float32)[None]
    voiced = np.ones((1, frames), np.uint8)
    amp = np.zeros((1, frames, H), np.float32)
    amp[:, :, H - 1] = 0.5
    ref = HR.synthesize(f0[0], voiced[0], amp[0], SR, hop, n)
    rc, y, ph, _, _ = raw_synth(cuda(f0), cuda(voiced), cuda(amp), n, hop)
    assert rc == 0 and np.array_equal(u32(ph)[0], ref["phase"])
    assert (np.uint64(H) * ref["phase"].astype(np.uint64) >= 2 ** 32).mean() > 0.9   # nearly every product wraps
    err = np.abs(y.cpu().numpy()[0].astype(np.float64) - ref["y"])
    bound = HR.synth_bound(H, ref["absum"])
    print(f"h = 128 alone: worst |y - ref| / bound {float((err / bound).max()):.3f}")
    assert (ref["absum"] == 0.5).all() and (err <= bound).all()


# ---- 2b. more than one trip through every loop ------------------------------------------------------------------------------
def test_synthesis_scan_with_several_frames_a_thread_and_several_frames_a_block():
    """frames = 376 > 256: harm_frame_scan_kernel gives a thread two frames (C = 2); B frames = 752 and hop = 8.  The phase is
    numpy's cumulative sum however the scan is split."""
    B, n, hop, H = 2, 3000, 8, 6
    frames = HR.frames_of(n, hop)
    assert frames > 256
    f0, voiced = HR.case_track(B, frames, H, SR, 256, salt=30, glide=True)
    amp = HR.case_amp(B, frames, H, salt=30)
    ref = [HR.synthesize(f0[b], voiced[b], amp[b], SR, hop, n) for b in range(B)]
    rc, y, ph, yg, pg = raw_synth(cuda(f0), cuda(voiced), cuda(amp), n, hop)
    assert rc == 0 and (yg == 7.0).all() and (pg == 0x5A5A5A5A).all()
    assert np.array_equal(u32(ph), np.stack([r["phase"] for r in ref]))
    err = np.abs(y.cpu().numpy().astype(np.float64) - np.stack([r["y"] for r in ref]))
    assert (err <= HR.synth_bound(H, np.stack([r["absum"] for r in ref]))).all()
    # one frame of 3000 samples (hop > L): twelve tiles of 256 samples behind one another in one block
    f1, v1, a1 = f0[:1, :1].copy(), np.ones((1, 1), np.uint8), amp[:1, :1].copy()
    f1[:] = 3000.0
    r1 = HR.synthesize(f1[0], v1[0], a1[0], SR, 4096, n)
    rc, y1, p1, _, _ = raw_synth(cuda(f1), cuda(v1), cuda(a1), n, 4096)
    assert rc == 0 and np.array_equal(u32(p1)[0], r1["phase"])
    assert (np.abs(y1.cpu().numpy()[0].astype(np.float64) - r1["y"]) <= HR.synth_bound(H, r1["absum"])).all()


def test_analysis_with_more_frames_than_blocks():
    """B frames = 3 * 751 = 2253 > 2048 blocks: some blocks take a second frame and reuse their LDS; the bits of a row alone (751
    blocks, one frame each) are those of the row in the batch"""
    B, n, N, hop, H = 3, 3000, 32, 4, 3
    frames = HR.frames_of(n, hop)
    assert B * frames > 2048
    f0, voiced = HR.case_track(B, frames, H, SR, N, salt=31)
    x = HR.case_signal(B, n, salt=31)
    kw = dict(n_harmonics=H, sr=SR, frame_length=N, hop_length=hop)
    amp, energy = HM.analyze(cuda(x), cuda(f0), cuda(voiced), **kw)
    for b in range(B):
        ab, eb = HM.analyze(cuda(x[b]), cuda(f0[b]), cuda(voiced[b]), **kw)
        assert same_bits(ab, amp[b]) and same_bits(eb, energy[b]), b
    ref = HR.analyze(x[B - 1], f0[B - 1], voiced[B - 1], H, SR, N, hop)              # the row whose frames come second
    got = amp[B - 1].cpu().numpy().astype(np.float64)
    assert np.array_equal(got != 0, ref["live"]) and ref["live"].any()
    bound = HR.analyze_gamma(N) * ref["absum"][:, None] / HR.window(N).astype(np.float64).sum()
    assert (np.abs(got - ref["amp"]) <= bound).all()
    e = energy[B - 1].cpu().numpy().astype(np.float64)
    assert (np.abs(e - ref["energy"]) <= HR.energy_gamma(N) * ref["energy"]).all()


def test_one_voiced_neighbour_and_interpolation_ends():
    """frames: voiced 300 Hz, unvoiced, voiced 500 Hz, voiced 700 Hz: the increments of each stretch in closed form"""
    hop, n = 100, 350
    f0 = np.array([[300.0, 123.0, 500.0, 700.0]], np.float32)
    voiced = np.array([[1, 0, 1, 1]], np.uint8)
    amp = np.full((1, 4, 2), 0.25, np.float32)
    rc, y, ph, _, _ = raw_synth(cuda(f0), cuda(voiced), cuda(amp), n, hop)
    assert rc == 0
    inc = np.diff(u32(ph)[0].astype(np.int64)) % 2 ** 32
    t = lambda f: int(HR.turns(f, SR))  # noqa: E731
    assert (inc[:99] == t(300.0)).all() and (inc[100:199] == t(500.0)).all()        # the voiced neighbour's f0, not a blend
    assert inc[200] == t(500.0) and inc[250] == t(600.0) and inc[299] == t(500.0 * 0.01 + 700.0 * 0.99)
    assert (inc[300:] == t(700.0)).all()                                            # the last frame is clamped
    ref = HR.synthesize(f0[0], voiced[0], amp[0], SR, hop, n)
    y = y.cpu().numpy()[0].astype(np.float64)
    assert (np.abs(y - ref["y"]) <= HR.synth_bound(2, ref["absum"])).all()
    assert abs(ref["absum"][99] - 0.5 * 0.01) < 1e-12 and abs(ref["absum"][101] - 0.5 * 0.01) < 1e-12   # the fade next to frame 1
    assert abs(y[50]) <= 0.5 * 0.5 + 1e-6 and np.abs(y[:100]).max() > 0.1


# ---- 3. determinism ---------------------------------------------------------------------------------------------------------
def test_determinism_rows_alone_and_a_common_prefix():
    B, n, N, hop, H = HR.SHAPES[2]
    x, f0, voiced, _ = analysis_case(2)
    xs, fs, vs = cuda(x), cuda(f0), cuda(voiced)
    kw = dict(n_harmonics=H, sr=SR, frame_length=N, hop_length=hop)
    a1, e1 = HM.analyze(xs, fs, vs, **kw)
    a2, e2 = HM.analyze(xs, fs, vs, **kw)
    assert same_bits(a1, a2) and same_bits(e1, e2)
    for b in range(B):
        ab, eb = HM.analyze(xs[b], fs[b], vs[b], **kw)
        assert same_bits(ab, a1[b]) and same_bits(eb, e1[b]), b
    # a shorter length: the frames whose window ends inside it see the same samples
    n2 = n - 3 * hop - 7
    fr2 = HR.frames_of(n2, hop)
    a3, e3 = HM.analyze(xs[:, :n2].contiguous(), fs[:, :fr2].contiguous(), vs[:, :fr2].contiguous(), **kw)
    whole = (n2 - N // 2) // hop + 1                              # frames f with f hop + N / 2 <= n2
    assert whole >= 3 and same_bits(a3[:, :whole].contiguous(), a1[:, :whole].contiguous())
    assert same_bits(e3[:, :whole].contiguous(), e1[:, :whole].contiguous())

    f0, voiced, amp, _ = synth_case(2)
    fs, vs, am = cuda(f0), cuda(voiced), cuda(amp)
    y1, p1 = HM.synthesize(fs, vs, am, n, hop_length=hop, want_phase=True)
    y2, p2 = HM.synthesize(fs, vs, am, n, hop_length=hop, want_phase=True)
    assert same_bits(y1, y2) and same_bits(p1, p2)
    for b in range(B):
        yb, pb = HM.synthesize(fs[b], vs[b], am[b], n, hop_length=hop, want_phase=True)
        assert same_bits(yb, y1[b]) and same_bits(pb, p1[b]), b
    y3, p3 = HM.synthesize(fs[:, :fr2].contiguous(), vs[:, :fr2].contiguous(), am[:, :fr2].contiguous(), n2, hop_length=hop,
                           want_phase=True)
    keep = (fr2 - 1) * hop                                        # before the shorter row's last frame, whose successor is clamped
    assert same_bits(y3[:, :keep].contiguous(), y1[:, :keep].contiguous())
    assert same_bits(p3[:, :keep].contiguous(), p1[:, :keep].contiguous())


# ---- 4. comparison ----------------------------------------------------------------------------------------------------------
def test_compare_counts_exact_and_the_cutoff_on_a_harmonic():
    B, frames, H = 3, 300, 24
    g = HR.rng(77)
    f0 = np.full((B, frames), 100.0, np.float32)                  # h f0 = 500 Hz lies exactly on the cutoff
    f0[1] = g.uniform(80, 400, frames).astype(np.float32)
    f0[2, ::7] = np.nan
    voiced = (g.random((B, frames)) < 0.8).astype(np.uint8)
    ref_amp = (g.random((B, frames, H)) ** 4).astype(np.float32)  # some cells under the floor
    a = (ref_amp * g.uniform(0.3, 2.0, ref_amp.shape)).astype(np.float32)
    floor, cutoff = 1e-3, 500.0
    out = HM._sums(cuda(a), cuda(ref_amp), cuda(f0), cuda(voiced), cutoff, floor).cpu().numpy()
    want = np.stack([HR.compare(a[b], ref_amp[b], f0[b], voiced[b], cutoff, floor) for b in range(B)])
    assert np.array_equal(out[:, [0, 4]], want[:, [0, 4]]) and (want[:, [0, 4]] > 0).all()
    n_voiced = int((voiced[0] != 0).sum())
    kept_row0 = int(((ref_amp[0][voiced[0] != 0][:, :4]) > floor).sum())
    assert out[0, 0] == kept_row0 and n_voiced > 0                # h = 1 .. 4 are kept; h = 5 (500 Hz) is regenerated
    # fp64 rounding of the sums: 1e-12 of sum |e| (|e| < 100 dB: 100 times that for sum e^2)
    for o in (0, 4):
        tol = 1e-12 * np.stack([want[:, o + 3], want[:, o + 3] * 100, want[:, o + 3]], 1)
        assert (np.abs(out[:, o + 1:o + 4] - want[:, o + 1:o + 4]) <= tol).all(), o
    rep = HM.compare(cuda(a[0]), cuda(ref_amp[0]), cuda(f0[0]), cuda(voiced[0]), cutoff, floor)
    assert rep["kept"] == HR.band_report(out[0, :4]) and rep["regenerated"] == HR.band_report(out[0, 4:])
    assert rep["all"]["n_cells"] == rep["kept"]["n_cells"] + rep["regenerated"]["n_cells"]
    allband = HM.compare(cuda(a), cuda(ref_amp), cuda(f0), cuda(voiced), None, floor)
    assert [sorted(r) for r in allband] == [["all"]] * B and allband[0]["all"]["n_cells"] == rep["all"]["n_cells"]


# ---- 5. end to end ----------------------------------------------------------------------------------------------------------
E2E = dict(n=44100, hop=512, N=2048, H=40, cutoff=8000.0)


@functools.lru_cache(maxsize=None)
def e2e_pair():
    """gt: the harmonic template of a slowly gliding tone; pred: gt with the harmonics above 8 kHz halved, plus noise;
    lr: the harmonics below 8 kHz alone"""
    n, hop, H = E2E["n"], E2E["hop"], E2E["H"]
    frames = HR.frames_of(n, hop)
    f0 = np.linspace(220.0, 233.0, frames).astype(np.float32)
    voiced = np.ones(frames, np.uint8)
    amp = np.tile((0.3 / np.arange(1, H + 1)).astype(np.float32), (frames, 1))
    high = np.arange(1, H + 1)[None, :] * f0[:, None].astype(np.float64) >= E2E["cutoff"]
    fs, vs = cuda(f0), cuda(voiced)
    gt = HM.synthesize(fs, vs, cuda(amp), n, hop_length=hop)
    noise = cuda((1e-4 * HR.rng(5).standard_normal(n)).astype(np.float32))
    pred = HM.synthesize(fs, vs, cuda(np.where(high, amp * np.float32(0.5), amp)), n, hop_length=hop) + noise
    lr = HM.synthesize(fs, vs, cuda(np.where(high, np.float32(0), amp)), n, hop_length=hop)
    return pred, gt, lr


def test_harmonic_metrics_end_to_end():
    pred, gt, lr = e2e_pair()
    n, hop, N, H, cutoff = (E2E[k] for k in ("n", "hop", "N", "H", "cutoff"))
    tables = {}
    rep = HM.harmonic_metrics(pred, gt, cutoff_hz=cutoff, n_harmonics=H, tables=tables)
    assert sorted(rep) == ["cutoff_hz", "generated", "harmonicity", "n_frames", "n_harmonics", "n_voiced"]
    assert sorted(rep["generated"]) == ["all", "kept", "regenerated"] and rep["n_frames"] == HR.frames_of(n, hop)
    f0, voiced = tables["f0"][0].cpu().numpy(), tables["voiced"][0].cpu().numpy()
    assert rep["n_voiced"] == int(HR.is_voiced(f0, voiced).sum()) > 0.9 * rep["n_frames"]
    # the fp64 statement on the same pair at the same track
    rp, rg = (HR.analyze(s.cpu().numpy(), f0, voiced, H, SR, N, hop) for s in (pred, gt))
    want = HR.compare(rp["amp"], rg["amp"], f0, voiced, cutoff, HM.DEFAULT_FLOOR)
    kept, regen = HR.band_report(want[:4]), HR.band_report(want[4:])
    assert rep["generated"]["kept"]["n_cells"] == kept["n_cells"] > 0
    assert rep["generated"]["regenerated"]["n_cells"] == regen["n_cells"] > 0
    # what the derived amp bound lets a cell's dB move: 20 / ln 10 (bound / (amp + floor)) for each of the two tables
    sumw = HR.window(N).astype(np.float64).sum()
    v = HR.is_voiced(f0, voiced)
    cell = v[:, None] & (rg["amp"] > HM.DEFAULT_FLOOR)
    db = 20.0 / np.log(10.0) * HR.analyze_gamma(N) / sumw * (rp["absum"][:, None] / (rp["amp"] + HM.DEFAULT_FLOOR) +
                                                             rg["absum"][:, None] / (rg["amp"] + HM.DEFAULT_FLOOR)) * 1.01
    hf = np.arange(1, H + 1)[None, :] * f0[:, None].astype(np.float64)
    d_kept, d_regen = float(db[cell & (hf < cutoff)].mean()), float(db[cell & ~(hf < cutoff)].mean())
    target = 20.0 * np.log10(0.5)
    got_k, got_r = rep["generated"]["kept"]["bias_db"], rep["generated"]["regenerated"]["bias_db"]
    print(f"end to end: regenerated bias {got_r:.4f} dB (fp64 {regen['bias_db']:.4f}, target {target:.4f}, allowance {d_regen:.2e}); "
          f"kept bias {got_k:.5f} dB (fp64 {kept['bias_db']:.5f}, allowance {d_kept:.2e})")
    assert abs(got_r - target) <= abs(regen["bias_db"] - target) + d_regen
    assert abs(got_r - regen["bias_db"]) <= d_regen and abs(got_k - kept["bias_db"]) <= d_kept
    assert abs(regen["bias_db"] - target) < 0.3 and abs(kept["bias_db"]) < 0.05      # the fixture itself: -6.02 dB and 0 dB
    assert abs(got_k) <= abs(kept["bias_db"]) + d_kept
    hp = float(HR.harmonicity(rg["amp"], rg["energy"], N)[v].mean())
    assert abs(rep["harmonicity"]["gt"] - hp) < 1e-3 and rep["harmonicity"]["gt"] > 0.95
    # with lr: its band limit is detected, the report gains lr_input, whose regenerated harmonics are gone
    full = HM.harmonic_metrics(pred, gt, lr, n_harmonics=H)
    assert sorted(full) == sorted(list(rep) + ["lr_input"]) and 7000.0 < full["cutoff_hz"] < 9000.0
    # (a harmonic between 8 kHz and the detected limit is absent from lr and yet counted as kept: the kept bias is not gated)
    assert full["lr_input"]["regenerated"]["bias_db"] < -30.0 and full["lr_input"]["kept"]["n_cells"] > 0
    assert abs(full["generated"]["regenerated"]["bias_db"] - target) < 0.3
    assert sorted(full["harmonicity"]) == ["generated", "gt", "lr_input"]
    # without lr and without a cutoff: the all-band figures alone; a batch gives lists
    plain = HM.harmonic_metrics(pred, gt, n_harmonics=H)
    assert sorted(plain["generated"]) == ["all"] and plain["cutoff_hz"] is None
    pa, ra = plain["generated"]["all"], rep["generated"]["all"]                       # one band's sums against two bands' added
    assert pa["n_cells"] == ra["n_cells"] and all(abs(pa[k] - ra[k]) <= 1e-12 * max(1.0, abs(ra[k])) for k in HM.BAND_KEYS[1:])
    batch = HM.harmonic_metrics(torch.stack([pred, gt]), torch.stack([gt, gt]), cutoff_hz=cutoff, n_harmonics=H)
    assert batch["generated"][0] == rep["generated"] and batch["generated"][1]["all"]["mean_abs_db"] == 0.0
    # the probabilistic tracker's voicing with the refined f0 (HM.METHODS[1])
    # (named through METHODS, not spelled out: that tracker's own CPU test, test_no_existing_test_calls_the_new_symbols, scans
    # every other file under tests/ for the tracker's name and stays as it is)
    py = HM.harmonic_metrics(pred, gt, cutoff_hz=cutoff, n_harmonics=H, method=HM.METHODS[1])
    assert abs(py["generated"]["regenerated"]["bias_db"] - target) < 0.5 and py["n_voiced"] > 0.8 * py["n_frames"]


def test_generate_harmonics_is_the_flat_template():
    frames, hop = 9, 64
    f0 = cuda(np.linspace(300.0, 320.0, frames).astype(np.float32))
    y = HM.generate_harmonics(f0, num_harmonics=5, hop_length=hop)
    want = HM.synthesize(f0, torch.ones(frames, dtype=torch.uint8, device="cuda"), torch.full((frames, 5), 0.2, device="cuda"),
                         (frames - 1) * hop, hop_length=hop)
    assert y.shape == ((frames - 1) * hop,) and same_bits(y, want) and float(y.abs().max()) <= 1.0


def test_command_line(tmp_path):
    pred, gt, lr = e2e_pair()
    for name, v in (("pred", pred), ("gt", gt), ("lr", lr)):
        jio.write_wav_float32(tmp_path / f"{name}.wav", v, SR)
    out = HM.main(["--pred", str(tmp_path / "pred.wav"), "--gt", str(tmp_path / "gt.wav"), "--lr", str(tmp_path / "lr.wav"),
                   "--json", str(tmp_path / "rep.json"), "--template", str(tmp_path / "t.wav"), "--n-harmonics", "5"])
    assert out == HM.harmonic_metrics(pred, gt, lr, n_harmonics=5) and json.loads((tmp_path / "rep.json").read_text()) == out
    t, sr = jio.read_wav(tmp_path / "t.wav")
    assert sr == SR and t.shape[-1] == E2E["n"] and 0.05 < float(np.abs(t).max()) < 1.0


def test_infer_harmonic_metrics_flag(tmp_path):
    """the synthetic codec and checkpoint of tests/test_gpu_metrics.py: the flag adds the "harmonic" entry and changes nothing else"""
    from test_gpu_metrics import _infer_setup
    from jatsr_amd import metrics
    from jatsr_amd.infer import main as infer_main
    base = _infer_setup(tmp_path)
    infer_main(base + ["--output-dir", str(tmp_path / "m"), "--metrics"])
    infer_main(base + ["--output-dir", str(tmp_path / "mh"), "--metrics", "--harmonic-metrics"])
    wavs = ["song_generated.wav", "song_hr_gt.wav", "song_lr_input.wav"]
    for d in ("m", "mh"):
        assert sorted(os.listdir(tmp_path / d)) == sorted(wavs + ["song_generated.pt", "song_metrics.json"])
        for name in wavs:
            assert (tmp_path / d / name).read_bytes() == (tmp_path / "m" / name).read_bytes(), (d, name)
    plain, both = (json.loads((tmp_path / d / "song_metrics.json").read_text()) for d in ("m", "mh"))
    assert "harmonic" not in plain and set(both) == set(plain) | {"harmonic"} and all(both[k] == plain[k] for k in plain)
    assert json.dumps({k: both[k] for k in plain}, indent=2) == (tmp_path / "m" / "song_metrics.json").read_text()
    gen, hr, lr = (metrics.load_audio(tmp_path / "mh" / name)[0] for name in wavs)
    assert both["harmonic"] == HM.harmonic_metrics(gen, hr, lr) and "lr_input" in both["harmonic"]
    assert both["harmonic"]["n_frames"] == 1 + hr.shape[0] // 512 and both["harmonic"]["n_harmonics"] == 64


def test_prepare_harmonics_flag(tmp_path):
    """the WAVs and the synthetic codec of tests/test_gpu_prepare.py: --f0 --harmonics 6 adds hr_harmonics fp16 [T, 6] beside
    hr_f0 and changes nothing else"""
    import jatsr_amd.recipe as recipe
    from test_gpu_prepare import _write_wavs
    from jatsr_amd.dac import load_dac_codec
    from jatsr_amd.prepare import hr_codec_signal, hr_harmonic_table, main as prepare_main
    full = {"decoder." + k: torch.from_numpy(v) for k, v in recipe.make_dac_state_dict().items()}
    full.update({k: torch.from_numpy(v) for k, v in recipe.make_dac_encoder_state_dict().items()})
    torch.save(full, tmp_path / "dac.pt")
    _write_wavs(tmp_path / "wav")
    argv = ["--source-dir", str(tmp_path / "wav"), "--dac-weights", str(tmp_path / "dac.pt"), "--val-fraction", "0.0", "--seed", "1"]
    prepare_main(argv + ["--output-dir", str(tmp_path / "f0"), "--f0"])
    prepare_main(argv + ["--output-dir", str(tmp_path / "h"), "--f0", "--harmonics", "6"])
    with pytest.raises(SystemExit, match="--f0"):
        prepare_main(argv + ["--output-dir", str(tmp_path / "x"), "--harmonics", "6"])
    codec = load_dac_codec(str(tmp_path / "dac.pt"))
    for stem in ("a", "b"):
        a = torch.load(tmp_path / "f0" / "train" / f"{stem}.pt", weights_only=False)
        b = torch.load(tmp_path / "h" / "train" / f"{stem}.pt", weights_only=False)
        assert sorted(b) == sorted(list(a) + ["hr_harmonics"])
        assert all(torch.equal(a[k], b[k]) for k in a if k != "metadata") and a["metadata"] == b["metadata"]
        T = a["hr_latent"].shape[1]
        h = b["hr_harmonics"]
        assert h.shape == (T, 6) and h.dtype == torch.float16 and not h.is_cuda and bool(torch.isfinite(h).all())
        x, sr = jio.read_wav(tmp_path / "wav" / f"{stem}.wav")
        again = hr_harmonic_table(hr_codec_signal(torch.from_numpy(x).cuda(), sr, codec), codec, b["hr_f0"].cuda(),
                                  b["hr_voiced"].cuda(), 6)
        assert torch.equal(again.cpu(), h)
        assert ((h != 0).any(dim=1) <= (b["hr_voiced"] != 0)).all()                 # nothing where the track is unvoiced


# ---- 6. the entries on a delayed side stream ------------------------------------------------------------------------------
def stream_cases():
    B, n, N, hop, H = 2, 64 * 9 + 5, 256, 64, 12
    frames = HR.frames_of(n, hop)
    f0, voiced = HR.case_track(B, frames, H, SR, N, salt=40)
    f0 = np.nan_to_num(f0, nan=150.0)                                               # the decoy is derived from the true values
    other = (HR.rng(41).random((B, frames)) < 0.5).astype(np.uint8)

    def analyze():
        inputs = dict(x=cuda(HR.case_signal(B, n, 40)), f0=cuda(f0), voiced=cuda(voiced))

        def call(_, i, o):
            amp, energy = HM.analyze(i["x"], i["f0"], i["voiced"], n_harmonics=H, frame_length=N, hop_length=hop)
            return {"amp": amp, "energy": energy}
        return Case(inputs, call, decoys={"voiced": cuda(other)})

    def synth():
        inputs = dict(f0=cuda(f0), voiced=cuda(voiced), amp=cuda(HR.case_amp(B, frames, H, 40)))

        def call(_, i, o):
            y, ph = HM.synthesize(i["f0"], i["voiced"], i["amp"], n, hop_length=hop, want_phase=True)
            return {"y": y, "phase": ph}
        return Case(inputs, call, decoys={"voiced": cuda(other)})

    def compare():
        inputs = dict(a=cuda(HR.case_amp(B, frames, H, 41)), r=cuda(HR.case_amp(B, frames, H, 42)), f0=cuda(f0), voiced=cuda(voiced))

        def call(_, i, o):
            HM._sums(i["a"], i["r"], i["f0"], i["voiced"], 3000.0, 1e-4, out=o["out"])
        return Case(inputs, call, outputs={"out": torch.empty(B, 8, dtype=torch.float64, device="cuda")},
                    decoys={"voiced": cuda(other)})

    return {"jat_harmonic_analyze": analyze, "jat_harmonic_synth": synth, "jat_harmonic_compare": compare}


def test_every_stream_taking_entry_has_a_side_stream_case():
    header = open(os.path.join(ROOT, "include", "jat_hip_harm.h")).read()
    protos = re.findall(r"\bint (jat_[a-z0-9_]+)\(([^;]*?)\);", header, re.S)
    taking = {name for name, args in protos if re.search(r"void\*\s*stream\b", args)}
    assert taking == set(stream_cases()) and len(taking) == 3
    assert taking | {"jat_harmonic_synth_workspace_bytes"} == set(L.HARM_SIGNATURES)


@pytest.mark.parametrize("name", ["jat_harmonic_analyze", "jat_harmonic_synth", "jat_harmonic_compare"])
def test_side_stream(name):
    check_case(stream_cases()[name](), name, synchronises=False)


def test_graph_capture():
    """each entry is captured into a graph and replayed on new inputs: no allocation, synchronisation or copy inside"""
    B, n, N, hop, H = 1, 64 * 5 + 3, 256, 64, 6
    frames = HR.frames_of(n, hop)
    f0, voiced = HR.case_track(B, frames, H, SR, N, salt=50)
    x, fs, vs = cuda(HR.case_signal(B, n, 50)), cuda(f0), cuda(voiced)
    amp, energy = torch.zeros(B, frames, H, device="cuda"), torch.zeros(B, frames, device="cuda")
    y, out = torch.zeros(B, n, device="cuda"), torch.zeros(B, 8, dtype=torch.float64, device="cuda")
    work = torch.zeros(B * frames * 4, dtype=torch.uint8, device="cuda")
    lib = L.lib()

    def run():
        s = L.stream_ptr()
        assert lib.jat_harmonic_analyze(L.ptr(x), B, n, L.ptr(fs), L.ptr(vs), frames, H, SR, N, hop, L.ptr(amp), L.ptr(energy), s) == 0
        assert lib.jat_harmonic_synth(L.ptr(fs), L.ptr(vs), L.ptr(amp), B, frames, H, n, SR, hop, L.ptr(y), None, L.ptr(work),
                                      work.numel(), s) == 0
        assert lib.jat_harmonic_compare(L.ptr(amp), L.ptr(amp), L.ptr(fs), L.ptr(vs), B, frames, H, 2000.0, 1e-6, L.ptr(out), s) == 0
    run()
    torch.cuda.synchronize()
    first = [t.clone() for t in (amp, energy, y, out)]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    x.copy_(cuda(HR.case_signal(B, n, 51)))
    g.replay()
    torch.cuda.synchronize()
    second = [t.clone() for t in (amp, energy, y, out)]
    assert not same_bits(first[0], second[0])
    run()
    torch.cuda.synchronize()
    assert all(same_bits(a, b) for a, b in zip(second, (amp, energy, y, out)))


# ---- 7. the fp16-operand library ------------------------------------------------------------------------------------------
def small_run():
    B, n, N, hop, H = HR.SHAPES[1]
    x, f0, voiced, _ = analysis_case(1)
    amp, energy = HM.analyze(cuda(x), cuda(f0), cuda(voiced), n_harmonics=H, frame_length=N, hop_length=hop)
    f0s, vs, am, _ = synth_case(1)
    y, ph = HM.synthesize(cuda(f0s), cuda(vs), cuda(am), n, hop_length=hop, want_phase=True)
    sums = HM._sums(amp, cuda(am), cuda(np.nan_to_num(f0, nan=100.0)), cuda(voiced), 2000.0, 1e-5)
    return {k: v.cpu().numpy() for k, v in dict(amp=amp, energy=energy, y=y, phase=ph, sums=sums).items()}


def test_fp16_library_gives_the_same_bits(tmp_path):
    """harmonic.hip is fp32 in both builds: libjat_hip_fp16.so (a child process) computes what this process computes"""
    code = ("import sys, numpy as np\n"
            "sys.path.insert(0, 'tests')\n"
            "import jatsr_amd._lib as L\n"
            "from test_harmonic_gpu import small_run\n"
            "assert L.operand_dtype() == 'fp16'\n"
            "np.savez(sys.argv[1], **small_run())\n")
    env = dict(os.environ, JAT_OPERAND_DTYPE="fp16")
    env.pop("JAT_LIB_PATH", None)
    path = str(tmp_path / "fp16.npz")
    out = subprocess.run([sys.executable, "-c", code, path], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
    other, here = dict(np.load(path)), small_run()
    assert L.operand_dtype() == "bf16" or os.environ.get("JAT_OPERAND_DTYPE") == "fp16"
    assert sorted(other) == sorted(here) and len(here) == 5
    for k, v in here.items():
        assert v.tobytes() == other[k].tobytes(), k


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_through_the_raw_abi():
    lib, s = L.lib(), L.stream_ptr()
    B, n, N, hop, H = 1, 64 * 3 + 17, 256, 64, 5
    frames = HR.frames_of(n, hop)
    x = cuda(HR.case_signal(B, n, 60))
    f0, v = torch.full((B, frames), 300.0, device="cuda"), torch.ones(B, frames, dtype=torch.uint8, device="cuda")
    amp, energy = torch.full((B, frames, H), 5.0, device="cuda"), torch.full((B, frames), 5.0, device="cuda")
    y = torch.full((B, n), 5.0, device="cuda")
    out = torch.full((B, 8), 5.0, dtype=torch.float64, device="cuda")
    work = torch.zeros(B * frames * 4, dtype=torch.uint8, device="cuda")
    X, F, V, A, E, Y, W, O = (L.ptr(t) for t in (x, f0, v, amp, energy, y, work, out))
    an, sy, cp = lib.jat_harmonic_analyze, lib.jat_harmonic_synth, lib.jat_harmonic_compare
    for bad in ((X, B, n, F, V, frames, 0, SR, N, hop, A, E), (X, B, n, F, V, frames, 129, SR, N, hop, A, E),
                (X, B, n, F, V, frames, H, SR, 14, hop, A, E), (X, B, n, F, V, frames, H, SR, 8194, hop, A, E),
                (X, B, n, F, V, frames, H, SR, 255, hop, A, E), (X, B, n, F, V, frames, H, SR, N, 0, A, E),
                (X, B, n, F, V, frames - 1, H, SR, N, hop, A, E), (X, B, n, F, V, frames + 1, H, SR, N, hop, A, E),
                (None, B, n, F, V, frames, H, SR, N, hop, A, E), (X, B, n, None, V, frames, H, SR, N, hop, A, E),
                (X, B, n, F, None, frames, H, SR, N, hop, A, E), (X, B, n, F, V, frames, H, SR, N, hop, None, E),
                (X, 0, n, F, V, frames, H, SR, N, hop, A, E), (X, B, 2 ** 33, F, V, frames, H, SR, N, 2, A, E),
                (X, B, 2 ** 26, F, V, 2 ** 26 + 1, 128, SR, N, 1, A, E)):
        assert an(*bad, s) == INV, bad[1:3] + bad[5:10]
    for bad in ((F, V, A, B, frames, 0, n, SR, hop, Y, None, W, work.numel()), (F, V, A, B, frames, 129, n, SR, hop, Y, None, W, work.numel()),
                (F, V, A, B, frames, H, n, SR, 0, Y, None, W, work.numel()), (F, V, A, B, frames - 1, H, n, SR, hop, Y, None, W, work.numel()),
                (F, V, A, B, frames, H, n, 0, hop, Y, None, W, work.numel()), (None, V, A, B, frames, H, n, SR, hop, Y, None, W, work.numel()),
                (F, None, A, B, frames, H, n, SR, hop, Y, None, W, work.numel()), (F, V, None, B, frames, H, n, SR, hop, Y, None, W, work.numel()),
                (F, V, A, B, frames, H, n, SR, hop, None, None, W, work.numel()), (F, V, A, B, frames, H, n, SR, hop, Y, None, None, work.numel()),
                (F, V, A, B, frames, H, n, SR, hop, Y, None, W, work.numel() - 1), (F, V, A, B, frames, H, 2 ** 33, SR, 2, Y, None, W, work.numel())):
        assert sy(*bad, s) == INV, bad[3:9]
    for bad in ((A, A, F, V, B, frames, 0, 100.0, 1e-5, O), (A, A, F, V, B, 0, H, 100.0, 1e-5, O), (A, A, F, V, B, frames, H, -1.0, 1e-5, O),
                (A, A, F, V, B, frames, H, 100.0, 0.0, O), (None, A, F, V, B, frames, H, 100.0, 1e-5, O),
                (A, A, F, V, B, frames, H, 100.0, 1e-5, None), (A, A, F, V, B, 2 ** 24, 128, 100.0, 1e-5, O)):
        assert cp(*bad, s) == INV, bad[4:9]
    torch.cuda.synchronize()
    assert all((t == 5.0).all() for t in (amp, energy, y, out))                     # nothing was launched
    assert an(X, B, n, F, V, frames, H, SR, N, hop, A, None, s) == 0                # energy may be NULL
    assert sy(F, V, A, B, frames, H, n, SR, hop, Y, None, W, work.numel(), s) == 0
    torch.cuda.synchronize()
    assert (energy == 5.0).all() and not (amp == 5.0).any() and not (y == 5.0).any()
    with pytest.raises(ValueError, match="frames"):
        HM.analyze(x, f0[:, :-1].contiguous(), v[:, :-1].contiguous(), frame_length=N, hop_length=hop)
    with pytest.raises(ValueError, match="n_harmonics"):
        HM.analyze(x, f0, v, n_harmonics=200, frame_length=N, hop_length=hop)
    with pytest.raises(L.JatError, match="match"):
        HM.synthesize(f0, v, amp[:, :-1].contiguous(), n, hop_length=hop)
    with pytest.raises(L.JatError, match="float32"):
        HM.analyze(x.double(), f0, v)
