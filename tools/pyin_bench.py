#!/usr/bin/env python3
"""Time the pYIN tracker (csrc/pyin.hip) with device events on one stream after warm-up:
    python tools/pyin_bench.py [--seconds 16 47.6] [--batch 1 8] [--reps 10] [--rounds 5] [--no-numpy]
(a) jatsr_amd.pitch.pyin(x) at the defaults, and its four launches apart (difference function, observation, Viterbi forward,
    back-trace) from the events the library records around them (`jat_pyin_set_profile`);
(b) jatsr_amd.pitch.yin(x), for scale;
(c) the same algorithm as a user composes it from PyTorch on the same GPU, fed with the library's own cmndf (so the leg is
    the probabilistic stage and the decoder alone, which favours it): troughs, threshold membership, Boltzmann weights and
    the scatter as tensor ops over [frames, candidates, thresholds] in slabs of frames, the Viterbi as a per-frame loop of
    unfold / max over both halves, the back-trace as a gather per frame on the device;
(d) the fp64 numpy statement (tests/pyin_ref.py) on the host, once, B = 1 only.
The legs alternate in rounds within one process; the median round counts and the spread of the rounds is printed, so that
a ratio inside it can be read as a tie.  The claim under test: the slowest pyin round is under the fastest round of (c)."""
import argparse
import ctypes as C
import hashlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SR, FL, HOP = 44100, 2048, 512


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
    """stages 2-6 of pYIN op by op in torch on the GPU, from a cmndf [B, frames, lags]"""

    def __init__(self, handle, T, device="cuda"):
        import torch
        t = self.t = torch
        tab = handle.tables()
        f32 = lambda a: t.tensor(a, dtype=t.float32, device=device)  # noqa: E731
        self.lo, self.hi, self.nb, self.H, self.N = T["lo"], T["hi"], T["n_bins"], T["H"], T["N"]
        self.theta, self.beta = f32(T["theta"]), f32(T["beta"])
        self.cum = f32(T["cum_beta"])
        self.A, self.invD = f32(T["A"]), f32(T["invD"])
        self.ntp = float(T["no_trough_prob"])
        self.logw_rev, self.logZ = f32(tab["logw"][::-1].copy()), f32(tab["logZ"])
        self.lk, self.ls, self.logpi = float(tab["lk"]), float(tab["ls"]), float(tab["logpi"])
        self.freqs = f32(tab["freqs"])
        self.lag = t.arange(self.lo, self.hi + 1, dtype=t.float64, device=device)
        self.scale, self.fmin = 12.0 * T["bps"], T["fmin"]
        self.tiny = float(t.finfo(t.float32).tiny)

    def observe(self, c, slab=64):
        t, nb = self.t, self.nb
        y = c[..., self.lo:self.hi + 1].reshape(-1, self.hi - self.lo + 1)
        F, ny = y.shape
        tr = t.zeros_like(y, dtype=t.bool)
        tr[:, 1:-1] = (y[:, 1:-1] < y[:, :-2]) & (y[:, 1:-1] <= y[:, 2:])
        tr[:, 0] = y[:, 0] < y[:, 1]
        yd = y.double()
        a, b = (yd[:, 2:] + yd[:, :-2]) - 2.0 * yd[:, 1:-1], (yd[:, 2:] - yd[:, :-2]) / 2.0
        ok = b.abs() < a.abs()
        shift = t.zeros_like(yd)
        shift[:, 1:-1] = t.where(ok, -b / t.where(ok, a, t.ones_like(a)), t.zeros_like(a))
        bins = t.clamp(t.round(self.scale * t.log2((SR / (self.lag[None, :] + shift)) / self.fmin)), 0, nb - 1).long()
        obs = t.zeros(F, nb, dtype=t.float32, device=y.device)
        idx = t.arange(ny, device=y.device)
        for f0 in range(0, F, slab):
            ys, ts = y[f0:f0 + slab], tr[f0:f0 + slab]
            under = ts[:, :, None] & (ys[:, :, None] < self.theta[None, None, :])          # [s, ny, N]
            n = under.sum(dim=1)                                                           # [s, N]
            p = under.cumsum(dim=1) - under.long()
            term = t.where(under, self.beta[None, None, :] * self.A[p.clamp(max=self.A.numel() - 1)] * self.invD[n][:, None, :],
                           t.zeros((), device=y.device))
            pr = term.sum(dim=2)                                                           # [s, ny]
            g = t.where(ts, ys, t.full_like(ys, float("inf"))).argmin(dim=1)
            nbelow = (~under[t.arange(ys.shape[0], device=y.device), g]).sum(dim=1)
            pr[t.arange(ys.shape[0], device=y.device), g] += t.where(ts.any(dim=1), self.ntp * self.cum[nbelow], t.zeros_like(self.cum[nbelow]))
            # the largest lag wins a shared bin: the winning candidate index per bin by an integer scatter-max
            win = t.full((ys.shape[0], nb), -1, dtype=t.long, device=y.device)
            win.scatter_reduce_(1, bins[f0:f0 + slab], t.where(ts, idx[None, :], t.full_like(idx, -1)[None, :]), "amax")
            obs[f0:f0 + slab] = t.where(win >= 0, pr.gather(1, win.clamp(min=0)), t.zeros((), device=y.device))
        vp = obs.sum(dim=1).clamp(0, 1)
        lo = t.log(t.cat([obs + self.tiny, ((1 - vp) / nb + self.tiny)[:, None]], dim=1))
        return vp.reshape(c.shape[:-1]), lo.reshape(c.shape[:-1] + (nb + 1,))

    def viterbi(self, lo):
        """lo [B, frames, nb + 1] -> (f0, voiced) [B, frames]"""
        t, nb, H = self.t, self.nb, self.H
        B, F, _ = lo.shape
        V = t.stack([lo[:, 0, :nb], lo[:, 0, nb:].expand(B, nb)], dim=1) + self.logpi          # [B, 2, nb]
        back = t.empty(F, B, 2 * nb, dtype=t.long, device=lo.device)
        base = t.arange(nb, device=lo.device) - H
        for f in range(1, F):
            U = t.nn.functional.pad(V - self.logZ, (H, H), value=float("-inf"))
            M, j = (U.unfold(2, 2 * H + 1, 1) + self.logw_rev).max(dim=3)                      # [B, 2, nb]
            R = base + j
            same0, oth0, same1, oth1 = M[:, 0] + self.lk, M[:, 1] + self.ls, M[:, 1] + self.lk, M[:, 0] + self.ls
            k0, k1 = same0 >= oth0, same1 > oth1
            new = t.stack([lo[:, f, :nb] + t.where(k0, same0, oth0), lo[:, f, nb:] + t.where(k1, same1, oth1)], dim=1)
            back[f] = t.cat([t.where(k0, R[:, 0], nb + R[:, 1]), t.where(k1, nb + R[:, 1], R[:, 0])], dim=1)
            V = new - new.amax(dim=(1, 2), keepdim=True)
        state = t.empty(B, F, dtype=t.long, device=lo.device)
        cur = V.reshape(B, -1).argmax(dim=1)
        state[:, F - 1] = cur
        for f in range(F - 1, 0, -1):
            cur = back[f].gather(1, cur[:, None])[:, 0]
            state[:, f - 1] = cur
        voiced = state < nb
        return t.where(voiced, self.freqs[state.clamp(max=nb - 1)], t.zeros((), device=lo.device)), voiced, state

    def pyin(self, c):
        vp, lo = self.observe(c)
        f0, voiced, state = self.viterbi(lo)
        return f0, voiced, vp, state


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, nargs="+", default=[16.0, 47.6])
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--torch-reps", type=int, default=1)
    ap.add_argument("--no-numpy", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    import pitch_ref as P
    import pyin_ref as Y
    from jatsr_amd import _lib
    from jatsr_amd.pitch import pyin, pyin_full, pyin_handle, yin
    _lib.require_gpu()
    print(f"library {os.path.basename(_lib.LIB_PATH)} sha256 {hashlib.sha256(open(_lib.LIB_PATH, 'rb').read()).hexdigest()[:16]}")
    h, T = pyin_handle(device="cuda"), Y.tables()
    base = TorchComposition(h, T)
    for seconds in a.seconds:
        n = int(round(seconds * SR))
        rng = np.random.default_rng(0)
        tt = np.arange(n) / SR
        f_inst = 110.0 * 4.0 ** (0.5 - 0.5 * np.cos(2 * np.pi * tt / 8.0)) * (1.0 + 0.01 * np.sin(2 * np.pi * 5.5 * tt))
        phase = 2 * np.pi * np.cumsum(f_inst) / SR
        sig = 0.2 * sum(0.6 ** k * np.sin((k + 1) * phase) for k in range(6)) * (np.sin(2 * np.pi * tt / 3.0) > -0.7)
        sig = (sig + 0.01 * rng.standard_normal(n)).astype(np.float32)
        frames = 1 + n // HOP
        for B in a.batch:
            x = torch.from_numpy(np.stack([np.roll(sig, 1000 * b) for b in range(B)])).cuda()
            full = pyin_full(x, want=("cmndf", "state"))
            c = full["cmndf"]
            fns = {"pyin": lambda: pyin(x), "yin": lambda: yin(x)}
            if not a.no_torch:
                fns["torch pyin (from cmndf)"] = lambda: base.pyin(c)
                f0_t, v_t, vp_t, st_t = base.pyin(c)
                mine = (full["state"] < h.n_bins, full["state"].long())
                differ = int(((mine[0] != v_t) | (mine[0] & v_t & (mine[1] != st_t))).sum())
            else:
                differ = -1
            for k, fn in fns.items():                     # warm-up
                for _ in range(1 if k.startswith("torch") else 3):
                    fn()
            torch.cuda.synchronize()
            t = {k: [] for k in fns}
            parts = []
            for _ in range(a.rounds):
                for k, fn in fns.items():
                    t[k].append(timed(fn, a.torch_reps if k.startswith("torch") else a.reps))
                _lib.lib().jat_pyin_set_profile(h.h, 1)
                pyin(x)
                us = (C.c_float * 4)()
                _lib.check(_lib.lib().jat_pyin_profile(h.h, us))
                _lib.lib().jat_pyin_set_profile(h.h, 0)
                parts.append(list(us))
            med = {k: statistics.median(v) for k, v in t.items()}
            pm = [statistics.median(p[i] for p in parts) for i in range(4)]
            line = (f"{seconds:5.1f} s B={B} ({frames} frames, {int(full['voiced'].sum())} voiced): "
                    + " | ".join(f"{k} {med[k]:9.1f} us [{min(t[k]):.1f}..{max(t[k]):.1f}]" for k in fns)
                    + f" | pyin launches: difference {pm[0]:.1f}, observe {pm[1]:.1f}, viterbi {pm[2]:.1f} ({pm[2] / (frames - 1):.3f} us a frame), "
                      f"trace {pm[3]:.1f} ({pm[3] / (frames - 1):.3f} us a frame)")
            if not a.no_torch:
                k = "torch pyin (from cmndf)"
                line += (f" | x{med[k] / med['pyin']:.1f}; slowest pyin round {max(t['pyin']):.1f} "
                         f"{'<' if max(t['pyin']) < min(t[k]) else '>='} fastest composition round {min(t[k]):.1f}"
                         f" | kernel and composition decode alike on {B * frames - differ} of {B * frames} frames")
            print(line, flush=True)
        if not a.no_numpy:
            t0 = time.perf_counter()
            r = P.yin(sig, dtype=np.float64)
            t1 = time.perf_counter()
            Y.decode(r["cmndf"], T, np.float64)
            t2 = time.perf_counter()
            print(f"{seconds:5.1f} s numpy fp64 statement on the host: difference function {t1 - t0:.1f} s, stages 2-6 {t2 - t1:.1f} s", flush=True)


if __name__ == "__main__":
    main()
