#!/usr/bin/env python3
"""Time the low-band splice (csrc/splice.hip) with HIP events on one stream after warm-up:
    python tools/splice_bench.py [--seconds 47.6 16] [--reps 50] [--rounds 7]
(a) jatsr_amd.splice.splice_lowband(generated, source, cutoff_hz=8000), B = 1: the transform kernel (two frames per
    complex transform, forward and inverse in LDS) and the overlap-add gather;
(b) the same algorithm as a user composes it from PyTorch on the same GPU: torch.stft (rocFFT) of the difference with the
    periodic Hann window and zero centre padding, a multiply by the gain, torch.istft, an add.
(a) and (b) alternate in rounds within one process; the median round counts and the spread of the rounds is printed, so
that a ratio inside it can be read as a tie.  The largest difference between the two results is printed too.
For a kernel table run it on its own under
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- python tools/splice_bench.py --reps 10 --rounds 1"""
import argparse
import hashlib
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3      # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, nargs="+", default=[4096 * 512 / 44100, 705536 / 44100])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    import numpy as np
    import torch
    from jatsr_amd import _lib
    from jatsr_amd.splice import band_gain, splice_lowband
    _lib.require_gpu()
    print(f"library {os.path.basename(_lib.LIB_PATH)} sha256 {hashlib.sha256(open(_lib.LIB_PATH, 'rb').read()).hexdigest()[:16]}")
    n_fft, hop, cutoff = 2048, 512, 8000.0
    win = torch.hann_window(n_fft, periodic=True, dtype=torch.float32, device="cuda")
    gain = band_gain(44100, n_fft, cutoff, 500.0).cuda()[:, None]
    for seconds in a.seconds:
        n = int(round(seconds * 44100))
        rng = np.random.default_rng(0)
        tt = np.arange(n) / 44100.0
        src_h = 0.3 * np.sin(2 * np.pi * 220 * tt) + 0.2 * np.sin(2 * np.pi * 3100 * tt + 0.3) + 0.02 * rng.standard_normal(n)
        src = torch.from_numpy(src_h.astype(np.float32)).cuda()
        gen = (0.9 * src + 0.05 * torch.from_numpy(rng.standard_normal(n).astype(np.float32)).cuda()).contiguous()

        def ours():
            return splice_lowband(gen, src, cutoff_hz=cutoff)[0]

        def torch_ops():
            D = torch.stft(src - gen, n_fft, hop, window=win, center=True, pad_mode="constant", return_complex=True)
            return gen + torch.istft(D * gain, n_fft, hop, window=win, center=True, length=n)

        diff = float((ours() - torch_ops()).abs().max())
        for fn in (ours, torch_ops):                      # warm-up: code objects, rocFFT plans
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        t = {"ours": [], "torch": []}
        for _ in range(a.rounds):
            t["ours"].append(timed(ours, a.reps))
            t["torch"].append(timed(torch_ops, a.reps))
        m = {k: statistics.median(v) for k, v in t.items()}
        print(f"{seconds:5.1f} s ({n} samples): splice_lowband {m['ours']:8.1f} us [{min(t['ours']):.1f}..{max(t['ours']):.1f}] | "
              f"torch composition {m['torch']:8.1f} us [{min(t['torch']):.1f}..{max(t['torch']):.1f}] | x{m['torch'] / m['ours']:.2f} | "
              f"max |ours - torch| {diff:.2e}", flush=True)


if __name__ == "__main__":
    main()
