#!/usr/bin/env python3
"""Time the pitch tracker (csrc/pitch.hip) with HIP events on one stream after warm-up:
    python tools/pitch_bench.py [--seconds 16 47.6] [--reps 50] [--rounds 7]
(a) jatsr_amd.pitch.yin(x): one launch, B = 1, the three tracks stay on the device;
    jatsr_amd.pitch.f0_metrics(pred, gt): one yin launch over both signals, one comparison launch, Python numbers out (one
    synchronising copy);
(b) the same algorithm as a user composes it from PyTorch on the same GPU, in the textbook fast form: frames by unfold,
    the difference function as E(0) + E(tau) - 2 acf(tau) with the autocorrelation from torch.fft (rocFFT) and the energies
    from a cumsum, the cumulative mean by cumsum, the troughs and the threshold as masks, argmax / argmin, gathers for the
    parabola.  That form cancels in fp32 at a periodic signal's dip, which the kernel's direct sum does not; the share of
    frames on which the two decide differently is printed.
(a) and (b) alternate in rounds within one process; the median round counts and the spread of the rounds is printed, so
that a ratio inside it can be read as a tie.
For a kernel table run it on its own under
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- python tools/pitch_bench.py --reps 10 --rounds 1"""
import argparse
import hashlib
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SR, FL, HOP, THRESHOLD, GROSS = 44100, 2048, 512, 0.1, 50.0


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
    """YIN op by op in torch on the GPU, autocorrelation form"""

    def __init__(self, lo, hi, device="cuda"):
        import torch
        self.t, self.lo, self.hi, self.W = torch, lo, hi, FL // 2
        self.tau = torch.arange(1, hi + 1, dtype=torch.float32, device=device)
        self.tiny = float(torch.finfo(torch.float32).tiny)

    def yin(self, x):
        t, W, lo, hi = self.t, self.W, self.lo, self.hi
        fr = t.nn.functional.pad(x, (FL // 2, FL // 2)).unfold(-1, FL, HOP)                 # [..., F, FL]
        head = t.nn.functional.pad(fr[..., :W], (0, FL - W))
        acf = t.fft.irfft(t.fft.rfft(head).conj() * t.fft.rfft(fr), n=FL)[..., 1:hi + 1]
        cs = t.nn.functional.pad(t.cumsum(fr * fr, dim=-1), (1, 0))
        d = (cs[..., W:W + 1] + (cs[..., W + 1:W + hi + 1] - cs[..., 1:hi + 1]) - 2.0 * acf).clamp_(min=0.0)
        c = d / (t.cumsum(d, dim=-1) / self.tau + self.tiny)
        y = c[..., lo - 1:]
        trough = t.zeros_like(y, dtype=t.bool)
        trough[..., 1:-1] = (y[..., 1:-1] < y[..., :-2]) & (y[..., 1:-1] <= y[..., 2:])
        trough[..., 0] = y[..., 0] < y[..., 1]
        under = trough & (y < THRESHOLD)
        voiced = under.any(dim=-1)
        k = t.where(voiced, under.to(t.int8).argmax(dim=-1), y.argmin(dim=-1))
        ny = y.shape[-1]
        ym, y0, yp = (y.gather(-1, (k + o).clamp(0, ny - 1)[..., None])[..., 0] for o in (-1, 0, 1))
        a, b = yp + ym - 2.0 * y0, (yp - ym) * 0.5
        ok = (k > 0) & (k < ny - 1) & (b.abs() < a.abs())
        shift = t.where(ok, -b / t.where(ok, a, t.ones_like(a)), t.zeros_like(a))
        return SR / ((lo + k).float() + shift), voiced, y0, k

    def f0_metrics(self, pred, gt):
        t = self.t
        f0, v, _, _ = self.yin(t.stack([pred, gt]))
        both = v[0] & v[1]
        cents = (1200.0 * t.log2(f0[0].double() / f0[1].double())).abs()
        gross = both & ~(cents <= GROSS)
        out = t.stack([v[1].sum().double(), both.sum().double(), (v[0] != v[1]).sum().double(), gross.sum().double(),
                       (cents * both).sum(), (cents * (both & ~gross)).sum()])
        return out.cpu().tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, nargs="+", default=[16.0, 47.6])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    import numpy as np
    import torch
    from jatsr_amd import _lib
    from jatsr_amd.pitch import f0_metrics, periods, yin, yin_full
    _lib.require_gpu()
    print(f"library {os.path.basename(_lib.LIB_PATH)} sha256 {hashlib.sha256(open(_lib.LIB_PATH, 'rb').read()).hexdigest()[:16]}")
    lo, hi = periods(SR, 50.0, 1000.0, FL)
    base = TorchComposition(lo, hi)
    for seconds in a.seconds:
        n = int(round(seconds * SR))
        rng = np.random.default_rng(0)
        tt = np.arange(n) / SR
        f_inst = 110.0 * 4.0 ** (0.5 - 0.5 * np.cos(2 * np.pi * tt / 8.0)) * (1.0 + 0.01 * np.sin(2 * np.pi * 5.5 * tt))
        phase = 2 * np.pi * np.cumsum(f_inst) / SR
        gt_h = 0.2 * sum(0.6 ** k * np.sin((k + 1) * phase) for k in range(6)) * (np.sin(2 * np.pi * tt / 3.0) > -0.7)
        gt_h = gt_h + 0.01 * rng.standard_normal(n)
        gt = torch.from_numpy(gt_h.astype(np.float32)).cuda()
        pred = (0.9 * gt + 0.01 * torch.from_numpy(rng.standard_normal(n).astype(np.float32)).cuda()).contiguous()
        frames = 1 + n // HOP
        fns = {"yin": lambda: yin(gt), "torch yin": lambda: base.yin(gt),
               "f0_metrics": lambda: f0_metrics(pred, gt), "torch f0_metrics": lambda: base.f0_metrics(pred, gt)}
        ours = yin_full(gt, want=("index",))
        f0_t, v_t, _, k_t = base.yin(gt)
        same = (ours["index"] == k_t) & (ours["voiced"].bool() == v_t)
        sel = same & v_t
        cents = float((1200.0 * torch.log2(ours["f0"][sel].double() / f0_t[sel].double())).abs().max()) if bool(sel.any()) else 0.0
        for fn in fns.values():                           # warm-up: code objects, rocFFT plans
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                t[k].append(timed(fn, a.reps))
        m = {k: statistics.median(v) for k, v in t.items()}
        terms = frames * hi * (FL // 2)
        print(f"{seconds:5.1f} s ({n} samples, {frames} frames, {int(ours['voiced'].sum())} voiced): "
              + " | ".join(f"{k} {m[k]:8.1f} us [{min(t[k]):.1f}..{max(t[k]):.1f}]" for k in fns)
              + f" | yin x{m['torch yin'] / m['yin']:.2f}, f0_metrics x{m['torch f0_metrics'] / m['f0_metrics']:.2f} | "
              f"{3 * terms / m['yin'] / 1e6:.2f} TFLOP/s in the difference function | kernel and composition decide alike on "
              f"{int(same.sum())} of {frames} frames, max {cents:.2e} cents apart on the voiced ones of them", flush=True)


if __name__ == "__main__":
    main()
