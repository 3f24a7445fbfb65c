#!/usr/bin/env python3
"""Time the audio-quality metrics (csrc/metrics.hip) with HIP events on one stream after warm-up:
    python tools/metrics_bench.py [--seconds 47.6 16] [--reps 50] [--rounds 7]
(a) jatsr_amd.metrics.evaluate(pred, gt): three STFT-and-reduce passes (the 2048 / 512 one carries the LSD), B = 1,
    Python floats out (one synchronising copy);
(b) the same algorithm as a user composes it from PyTorch on the same GPU: torch.stft (rocFFT) with the periodic Hann
    window and zero centre padding, abs, the dense mel filterbank as a matmul, log10, amax, clamp, the means; the 2048 / 512
    spectrogram is shared by the LSD and the mel terms, and the results come back in one synchronising copy as well.
(a) and (b) alternate in rounds within one process; the median round counts and the spread of the rounds is printed, so
that a ratio inside it can be read as a tie.  The largest difference between the two results is printed too.
For a kernel table run it on its own under
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- python tools/metrics_bench.py --reps 10 --rounds 1"""
import argparse
import hashlib
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SCALES = ((512, 128, 40), (1024, 256, 64), (2048, 512, 80))


def timed(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3      # us


class TorchComposition:
    """calculate_metrics.py op by op in torch on the GPU"""

    def __init__(self, device, sr=44100):
        import torch
        from jatsr_amd.metrics import mel_filterbank
        self.t = torch
        self.win = {n: torch.hann_window(n, periodic=True, dtype=torch.float32, device=device) for n, _, _ in SCALES}
        self.fb = {n: mel_filterbank(sr, n, m).to(device) for n, _, m in SCALES}

    def db(self, S):
        t = self.t
        ls = 10.0 * t.log10(t.clamp(S, min=1e-10)) - 10.0 * t.log10(t.clamp(S.amax(), min=1e-10))
        return t.maximum(ls, ls.amax() - 80.0)

    def __call__(self, pred, gt):
        t = self.t
        n = min(pred.shape[-1], gt.shape[-1])
        pred, gt = pred[..., :n], gt[..., :n]
        out = []
        for n_fft, hop, _ in SCALES:
            P, G = (t.stft(x, n_fft, hop, window=self.win[n_fft], center=True, pad_mode="constant", return_complex=True).abs()
                    for x in (pred, gt))
            a, b = self.db(self.fb[n_fft] @ (P * P)), self.db(self.fb[n_fft] @ (G * G))
            d = a - b
            out += [d.abs().mean(), (d * d).mean().sqrt()]
            if n_fft == 2048:
                ld = t.log10(t.clamp(P, min=1e-8)) - t.log10(t.clamp(G, min=1e-8))
                out.append(20.0 * (ld * ld).mean(dim=0).sqrt().mean())
        v = t.stack(out).cpu().tolist()
        return {"lsd": v[6], "mel_l1": v[4], "mel_l2": v[5], "ms_l1": (v[0] + v[2] + v[4]) / 3, "ms_l2": (v[1] + v[3] + v[5]) / 3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, nargs="+", default=[4096 * 512 / 44100, 705536 / 44100])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    import numpy as np
    import torch
    from jatsr_amd import _lib
    from jatsr_amd.metrics import METRIC_KEYS, evaluate
    _lib.require_gpu()
    print(f"library {os.path.basename(_lib.LIB_PATH)} sha256 {hashlib.sha256(open(_lib.LIB_PATH, 'rb').read()).hexdigest()[:16]}")
    base = TorchComposition(torch.device("cuda"))
    for seconds in a.seconds:
        n = int(round(seconds * 44100))
        rng = np.random.default_rng(0)
        tt = np.arange(n) / 44100.0
        gt_h = (0.3 * np.sin(2 * np.pi * 220 * tt) + 0.2 * np.sin(2 * np.pi * 3100 * tt + 0.3) + 0.02 * rng.standard_normal(n))
        gt = torch.from_numpy(gt_h.astype(np.float32)).cuda()
        pred = (0.9 * gt + 0.01 * torch.from_numpy(rng.standard_normal(n).astype(np.float32)).cuda()).contiguous()

        def ours():
            return evaluate(pred, gt)["generated"]

        def torch_ops():
            return base(pred, gt)

        r_a, r_b = ours(), torch_ops()
        diff = max(abs(r_a[k] - r_b[k]) for k in METRIC_KEYS)
        for fn in (ours, torch_ops):                      # warm-up: code objects, rocFFT plans
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        t = {"ours": [], "torch": []}
        for _ in range(a.rounds):
            t["ours"].append(timed(ours, a.reps))
            t["torch"].append(timed(torch_ops, a.reps))
        m = {k: statistics.median(v) for k, v in t.items()}
        print(f"{seconds:5.1f} s ({n} samples): evaluate {m['ours']:8.1f} us [{min(t['ours']):.1f}..{max(t['ours']):.1f}] | "
              f"torch composition {m['torch']:8.1f} us [{min(t['torch']):.1f}..{max(t['torch']):.1f}] | x{m['torch'] / m['ours']:.2f} | "
              f"lsd {r_a['lsd']:.4f} mel_l1 {r_a['mel_l1']:.4f} ms_l2 {r_a['ms_l2']:.4f}, max |ours - torch| {diff:.2e}", flush=True)


if __name__ == "__main__":
    main()
