#!/usr/bin/env python3
"""Time the voicing-aware index rates (csrc/retrieval_rate.hip) with HIP events on one stream after warm-up:
    python tools/retrieval_rate_bench.py [--keys 100000] [--frames 1378 4096] [--reps 20] [--rounds 11]
at C = 1024, B = 1:
(a) LatentBank.retrieve with a per-frame track against the same call with a scalar rate, k = 1 and k = 8: the difference is the
    cost of the feature (the range check of the track on the host, one more pass over [C, T] and its launch);
(b) mix_rates alone (the unchecked launch and the checked Python call) against its byte bound, 3 C T 4 bytes at the copy rate
    this process measures with a device-to-device copy of the same size, and against torch.lerp(x, v, rates[:, None, :]);
(c) f0_classes + rate_track for 47.6 s of audio (4101 frames) beside the yin call that feeds them.
The variants alternate in rounds within one process; the median round counts and the range of the rounds is printed.  The
existing path does not pay by construction: the sha256 of the four retrieval kernel sources is printed for comparison with the
parent commit's."""
import argparse
import hashlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from retrieval_bench import timed  # noqa: E402


def sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=100_000)
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--frames", type=int, nargs="+", default=[1378, 4096])
    ap.add_argument("--seconds", type=float, default=47.6)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--rate", type=float, default=0.4)
    a = ap.parse_args()
    import torch
    from jatsr_amd import _lib, pitch
    from jatsr_amd import retrieval as RT
    _lib.require_gpu()
    print(f"library {os.path.basename(_lib.LIB_PATH)} sha256 {sha(_lib.LIB_PATH)[:16]}")
    csrc = os.path.join(ROOT, "jatsr-just-audio-transformer-super-solution_amd", "csrc")
    for name in ("retrieval.hip", "retrieval_ms.hip", "retrieval_km.hip", "retrieval_ivf.hip"):
        print(f"  {name:18s} sha256 {sha(os.path.join(csrc, name))}")
    N, C = a.keys, a.channels
    g = torch.Generator(device="cuda").manual_seed(0)
    mean = torch.randn(C, device="cuda", generator=g) * 0.2
    std = torch.rand(C, device="cuda", generator=g) + 0.5
    stats = {"hr_mean": mean, "hr_std": std, "lr_mean": mean, "lr_std": std}
    bank = RT.LatentBank(C, N)
    bank._set_stats(stats)
    bank.load_rows(torch.randn(N, C, device="cuda", generator=g).half())
    print(f"bank: {N} x {C} fp16 = {N * C * 2 / 2 ** 20:.0f} MiB")

    def measure(fns):
        for f in fns.values():
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        t = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, f in fns.items():
                t[k].append(timed(f, a.reps))
        m = {k: statistics.median(v) for k, v in t.items()}
        for k in fns:
            print(f"  {k:40s} {m[k]:10.1f} us [{min(t[k]):.1f}..{max(t[k]):.1f}]", flush=True)
        return m

    for T in a.frames:
        x = (torch.randn(1, C, T, device="cuda", generator=g) * std[None, :, None] + mean[None, :, None]).contiguous()
        cls = (torch.arange(T, device="cuda") // 40 % 3).to(torch.uint8)           # stretches of 40 frames of each class
        rates = RT.rate_track(cls, T, a.rate, protect=0.33, unstable=0.7, smooth=2)[None].contiguous()
        v = bank.retrieve(x, 1.0)
        y, copy_dst = torch.empty_like(x), torch.empty(3 * x.numel() // 2, device="cuda")
        copy_src = torch.randn(3 * x.numel() // 2, device="cuda", generator=g)      # a copy moving 3 C T 4 bytes: read half, write half
        print(f"T = {T}:")
        m = measure({"retrieve scalar k=1": lambda: bank.retrieve(x, a.rate),
                     "retrieve track  k=1": lambda: bank.retrieve(x, rates),
                     "retrieve scalar k=8": lambda: bank.retrieve(x, a.rate, k=8),
                     "retrieve track  k=8": lambda: bank.retrieve(x, rates, k=8),
                     "mix_rates (launch only)": lambda: RT._mix_rates(x, v, rates, y),
                     "mix_rates (with the host range check)": lambda: RT.mix_rates(x, v, rates, out=y),
                     "torch.lerp(x, v, rates[:, None, :])": lambda: torch.lerp(x, v, rates[:, None, :], out=y),
                     "device copy of 3 C T 4 bytes": lambda: copy_dst.copy_(copy_src)})
        nbytes = 3 * C * T * 4
        copy_rate = nbytes / (m["device copy of 3 C T 4 bytes"] * 1e-6) / 1e12
        mix = m["mix_rates (launch only)"]
        print(f"  cost of the track: k=1 {m['retrieve track  k=1'] - m['retrieve scalar k=1']:+.1f} us "
              f"(x{m['retrieve track  k=1'] / m['retrieve scalar k=1']:.3f}), k=8 "
              f"{m['retrieve track  k=8'] - m['retrieve scalar k=8']:+.1f} us (x{m['retrieve track  k=8'] / m['retrieve scalar k=8']:.3f})")
        print(f"  mix_rates: {nbytes / 1e6:.1f} MB in {mix:.1f} us = {nbytes / (mix * 1e-6) / 1e12:.2f} TB/s; the copy of as many bytes "
              f"runs at {copy_rate:.2f} TB/s: mix / byte bound x{mix / m['device copy of 3 C T 4 bytes']:.2f}; "
              f"torch.lerp / mix x{m['torch.lerp(x, v, rates[:, None, :])'] / mix:.2f} (launches included)", flush=True)
        assert torch.equal(RT._mix_rates(x, v, torch.full_like(rates, a.rate), torch.empty_like(x)), bank.retrieve(x, a.rate))
    L = int(a.seconds * 44100)
    t = torch.arange(L, device="cuda", dtype=torch.float32) / 44100
    audio = (0.5 * torch.sin(2 * torch.pi * (220.0 * t + 40.0 * t * t)) + 0.05 * torch.randn(L, device="cuda", generator=g)).contiguous()
    f0, voiced, _ = pitch.yin(audio)
    frames = f0.shape[0]
    cls, _ = RT.f0_classes(f0, voiced)
    print(f"{a.seconds} s of audio, {frames} pitch frames:")
    measure({"yin": lambda: pitch.yin(audio),
             "f0_classes": lambda: RT.f0_classes(f0, voiced),
             "rate_track": lambda: RT.rate_track(cls, frames, a.rate, protect=0.33, unstable=0.7, smooth=2),
             "f0_classes + rate_track": lambda: RT.rate_track(RT.f0_classes(f0, voiced)[0], frames, a.rate, protect=0.33,
                                                             unstable=0.7, smooth=2)})


if __name__ == "__main__":
    main()
