#!/usr/bin/env python3
"""Time the harmonic analysis, the harmonic template and harmonic_metrics (csrc/harmonic.hip) with HIP events on one
stream after warm-up:
    python tools/harmonic_bench.py [--seconds 16 47.6] [--harmonics 64] [--reps 5] [--rounds 5]
at 44.1 kHz, frame_length 2048, hop 512, B = 1, on a gliding harmonic tone with unvoiced stretches, against the same algorithm
as a user composes it from PyTorch on the same GPU: integer phases (int64 products masked to 32 bits), the [frames, H, N] basis
of cosines and sines built in chunks of frames (all at once it is tens of GB) and contracted with the windowed frames; the
oscillator bank from a cumulative sum of the per-sample increments and an [L, H] table of sines built in chunks of samples.
harmonic_metrics is the whole call (YIN track of the ground truth, two analyses, the comparison, one host copy); its torch side
keeps the library's YIN and replaces the analyses and the comparison.
The variants alternate in rounds within one process; the median round counts and the range of the rounds is printed, so that a
ratio inside it reads as a tie.  The analysis is also given as fp32 VALU work: 2 fmas and one sincosf a term.
Before anything is timed the two sides are compared: the run ends with an error when the library and the torch composition differ
by more than AGREE (both are fp32 evaluations of one formula; 1e-6 was seen)."""
import argparse
import hashlib
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from retrieval_bench import peak_temp_bytes, timed  # noqa: E402

SR, N, HOP = 44100, 2048, 512
TURN = 2.0 * math.pi * 2.0 ** -32
AGREE = 1e-5          # largest |library - torch composition| accepted, amplitudes and samples of order 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, nargs="+", default=[16.0, 47.6])
    ap.add_argument("--harmonics", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frame-chunk", type=int, default=128)
    ap.add_argument("--sample-chunk", type=int, default=1 << 17)
    a = ap.parse_args()
    import torch
    from jatsr_amd import _lib
    from jatsr_amd import harmonic as HM
    from jatsr_amd import pitch
    _lib.require_gpu()
    print(f"library {os.path.basename(_lib.LIB_PATH)} sha256 {hashlib.sha256(open(_lib.LIB_PATH, 'rb').read()).hexdigest()[:16]}")
    H = a.harmonics
    window = torch.hann_window(N, periodic=True, device="cuda", dtype=torch.float64).float()
    limit = SR / 2.0 - 2.0 * SR / N

    def turns(f):
        return torch.round(f / SR * 4294967296.0).to(torch.int64)

    def angle(p):
        return (p & 0xFFFFFFFF).to(torch.int32).float() * TURN

    def torch_analyze(x, f0, voiced):
        frames = f0.shape[0]
        xp = torch.nn.functional.pad(x, (N // 2, N // 2 + N))
        fr = xp.unfold(0, N, HOP)[:frames] * window
        hs = torch.arange(1, H + 1, device="cuda", dtype=torch.float64)
        n = torch.arange(N, device="cuda", dtype=torch.int64)
        amp = torch.empty(frames, H, device="cuda")
        for c0 in range(0, frames, a.frame_chunk):
            c1 = min(c0 + a.frame_chunk, frames)
            hf = hs[None, :] * f0[c0:c1, None].double()
            live = (voiced[c0:c1, None] != 0) & (hf > 0) & (hf < limit)
            ang = angle(turns(torch.where(live, hf, torch.zeros_like(hf)))[:, :, None] * n)
            re = torch.einsum("fhn,fn->fh", torch.cos(ang), fr[c0:c1])
            im = torch.einsum("fhn,fn->fh", torch.sin(ang), fr[c0:c1])
            amp[c0:c1] = torch.where(live, torch.sqrt(re * re + im * im) * (4.0 / N), torch.zeros_like(re))
        return amp, (fr * fr).sum(1)

    def torch_synth(f0, voiced, amp, n_samples):
        frames = f0.shape[0]
        n = torch.arange(n_samples, device="cuda")
        f = n // HOP
        fb = (f + 1).clamp_max(frames - 1)
        u = (n - f * HOP).double() / HOP
        v = (voiced != 0) & (f0 > 0)
        f64 = torch.where(v, f0, torch.zeros_like(f0)).double()
        va, vb = v[f], v[fb]
        f0n = torch.where(va & vb, (1 - u) * f64[f] + u * f64[fb], torch.where(va, f64[f], torch.where(vb, f64[fb], 0.0)))
        inc = torch.where(f0n < SR / 2.0, turns(f0n), torch.zeros_like(n))
        phase = (torch.cumsum(inc, 0) - inc) & 0xFFFFFFFF
        hs = torch.arange(1, H + 1, device="cuda")
        y = torch.empty(n_samples, device="cuda")
        A = amp * v[:, None]
        for c0 in range(0, n_samples, a.sample_chunk):
            c = slice(c0, min(c0 + a.sample_chunk, n_samples))
            uf = u[c].float()[:, None]
            ah = (1 - uf) * A[f[c]] + uf * A[fb[c]]
            keep = hs[None, :].double() * f0n[c, None] < SR / 2.0
            y[c] = (ah * torch.sin(angle(phase[c, None] * hs[None, :])) * keep).sum(1)
        return y

    def torch_compare(amp_a, amp_r, f0, voiced, cutoff, floor):
        cell = ((voiced != 0) & (f0 > 0))[:, None] & (amp_r > floor)
        e = 20.0 * torch.log10((amp_a.double() + floor) / (amp_r.double() + floor))
        hf = torch.arange(1, H + 1, device="cuda", dtype=torch.float64)[None, :] * f0[:, None].double()
        out = []
        for band in (cell & (hf < cutoff), cell & ~(hf < cutoff)):
            eb = torch.where(band, e, torch.zeros_like(e))
            out += [band.sum().double(), eb.sum(), (eb * eb).sum(), eb.abs().sum()]
        return torch.stack(out)

    for seconds in a.seconds:
        n = int(seconds * SR)
        frames = 1 + n // HOP
        t = torch.arange(frames, device="cuda", dtype=torch.float32)
        f0 = 180.0 + 60.0 * torch.sin(t / 37.0)
        voiced = ((t.long() // 50) % 5 != 4).to(torch.uint8)                       # every fifth stretch of 50 frames is unvoiced
        amp0 = (0.4 / torch.arange(1, H + 1, device="cuda")).repeat(frames, 1).contiguous()
        gt = HM.synthesize(f0, voiced, amp0, n)
        scale = torch.where(torch.arange(1, H + 1, device="cuda")[None, :] * f0[:, None] >= 8000.0, 0.5, 1.0)
        pred = HM.synthesize(f0, voiced, (amp0 * scale).contiguous(), n) + 1e-3 * torch.randn(n, device="cuda")

        def torch_metrics():
            tf0, tv, _ = pitch.yin(gt)
            tv = tv.view(torch.uint8)
            ap_, _ = torch_analyze(pred, tf0, tv)
            ag, _ = torch_analyze(gt, tf0, tv)
            return torch_compare(ap_, ag, tf0, tv, 8000.0, HM.DEFAULT_FLOOR).cpu()

        fns = {"analyze": lambda: HM.analyze(gt, f0, voiced, n_harmonics=H),
               "torch analyze": lambda: torch_analyze(gt, f0, voiced),
               "synthesize": lambda: HM.synthesize(f0, voiced, amp0, n),
               "torch synthesize": lambda: torch_synth(f0, voiced, amp0, n),
               "harmonic_metrics": lambda: HM.harmonic_metrics(pred, gt, cutoff_hz=8000.0, n_harmonics=H),
               "torch harmonic_metrics": torch_metrics,
               "yin alone": lambda: pitch.yin(gt)}
        amp_l, en_l = HM.analyze(gt, f0, voiced, n_harmonics=H)
        amp_t, en_t = torch_analyze(gt, f0, voiced)
        d_amp = float((amp_l - amp_t).abs().max())
        d_y = float((HM.synthesize(f0, voiced, amp0, n) - torch_synth(f0, voiced, amp0, n)).abs().max())
        live = int((amp_l != 0).sum())
        if not (d_amp <= AGREE and d_y <= AGREE):
            raise SystemExit(f"the torch composition is not the library's algorithm: max |analyze - torch| {d_amp:.2e}, "
                             f"max |synthesize - torch| {d_y:.2e} (accepted: {AGREE:.0e})")
        temp = {k: peak_temp_bytes(f) for k, f in fns.items()}
        for f in fns.values():
            f()
        torch.cuda.synchronize()
        tm = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, f in fns.items():
                tm[k].append(timed(f, a.reps))
        m = {k: statistics.median(v) for k, v in tm.items()}
        print(f"{seconds} s = {n} samples, {frames} frames, H = {H}: {live} live cells; max |analyze - torch| {d_amp:.2e}, "
              f"max |synthesize - torch| {d_y:.2e}")
        for k in fns:
            print(f"  {k:26s} {m[k]:11.1f} us [{min(tm[k]):.1f}..{max(tm[k]):.1f}] | allocator peak over one call "
                  f"{temp[k] / 2 ** 20:8.1f} MiB", flush=True)
        terms = live * N
        print(f"  analyze: {terms / 1e9:.2f} G terms (sincosf + 2 fma each), {terms / (m['analyze'] * 1e-6) / 1e12:.3f} T terms/s, "
              f"{4 * terms / (m['analyze'] * 1e-6) / 1e12:.2f} TFLOP/s counting the fmas alone")
        print(f"  torch / library: analyze x{m['torch analyze'] / m['analyze']:.1f}, synthesize "
              f"x{m['torch synthesize'] / m['synthesize']:.1f}, harmonic_metrics "
              f"x{m['torch harmonic_metrics'] / m['harmonic_metrics']:.1f}", flush=True)


if __name__ == "__main__":
    main()
