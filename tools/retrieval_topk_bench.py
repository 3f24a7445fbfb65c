#!/usr/bin/env python3
"""Time top-k latent retrieval (csrc/retrieval.hip) with HIP events on one stream after warm-up:
    python tools/retrieval_topk_bench.py [--keys 100000] [--frames 1378 4096] [--reps 20] [--rounds 11]
at C = 1024, B = 1:
(a) LatentBank.search (k = 1) against LatentBank.search_topk at k = 2, 4, 8 (list lengths 2, 4, 8), queries normalised
    already: what the per-lane lists, the merge at the end of a slab and the k-way merge over slabs cost;
(b) LatentBank.retrieve at k = 1 and k = 8 (search with the normalisation in the loader + the de-normalising blend, index rate
    0.4) against the k = 8 algorithm as a user composes it from PyTorch on the same GPU, with the bank kept as an fp32 [N, C]
    tensor: the per-channel normalisation, G = q @ keys32.T, G * -2 + |k|^2 + |q|^2, topk(8, largest=False), the gather of
    the eight rows, the inverse-square weights in their ratio form, the weighted sum, values * std + mean, torch.lerp.
The variants alternate in rounds within one process; the median round counts and the range of the rounds is printed, so that
a ratio inside it reads as a tie.  How many of torch's index lists equal ours is printed too (fp32 GEMM rounding may move
near-ties)."""
import argparse
import hashlib
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from retrieval_bench import peak_temp_bytes, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=100_000)
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--frames", type=int, nargs="+", default=[1378, 4096])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--rate", type=float, default=0.4)
    ap.add_argument("--floor", type=float, default=1e-6)
    a = ap.parse_args()
    import torch
    from jatsr_amd import _lib
    from jatsr_amd.retrieval import LatentBank
    _lib.require_gpu()
    print(f"library {os.path.basename(_lib.LIB_PATH)} sha256 {hashlib.sha256(open(_lib.LIB_PATH, 'rb').read()).hexdigest()[:16]}")
    N, C = a.keys, a.channels
    g = torch.Generator(device="cuda").manual_seed(0)
    mean = torch.randn(C, device="cuda", generator=g) * 0.2
    std = torch.rand(C, device="cuda", generator=g) + 0.5
    stats = {"hr_mean": mean, "hr_std": std, "lr_mean": mean, "lr_std": std}
    bank = LatentBank(C, N)
    bank._set_stats(stats)
    bank.load_rows(torch.randn(N, C, device="cuda", generator=g).half())
    keys16, norms = bank.rows("keys")
    keys32 = keys16.float()
    print(f"bank: {N} x {C} fp16 = {N * C * 2 / 2 ** 20:.0f} MiB; torch's fp32 copy {N * C * 4 / 2 ** 20:.0f} MiB")
    for T in a.frames:
        xn = torch.randn(1, C, T, device="cuda", generator=g)                 # normalised queries
        x = (xn * std[None, :, None] + mean[None, :, None]).contiguous()      # de-normalised latent

        def torch_retrieve8():
            q = ((x[0] - mean[:, None]) / std[:, None]).T
            G = q @ keys32.T
            G.mul_(-2.0).add_(norms[None, :]).add_((q * q).sum(1)[:, None])
            d, idx = torch.topk(G, 8, dim=1, largest=False)
            d = d.clamp_min_(a.floor)
            u = (d[:, :1] / d).square_()
            w = u / u.sum(1, keepdim=True)
            v = (keys16[idx].float() * w[:, :, None]).sum(1) * std[None, :] + mean[None, :]
            return torch.lerp(x, v.T[None], a.rate), idx

        fns = {"search": lambda: bank.search(xn)}
        for k in (2, 4, 8):
            fns[f"search_topk k={k}"] = lambda k=k: bank.search_topk(xn, k)
        fns["retrieve k=1"] = lambda: bank.retrieve(x, a.rate)
        fns["retrieve k=8"] = lambda: bank.retrieve(x, a.rate, k=8)
        fns["torch retrieve k=8"] = torch_retrieve8

        y_ours, i_ours, _ = bank.retrieve(x, a.rate, k=8, neighbours=True)
        y_torch, i_torch = torch_retrieve8()
        agree = float((i_ours[0] == i_torch).all(1).float().mean())
        ydiff = float((y_ours - y_torch).abs().max())
        temp = {k: peak_temp_bytes(f) for k, f in fns.items()}
        for f in fns.values():                      # warm-up: code objects, the GEMM library's choices
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        t = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, f in fns.items():
                t[k].append(timed(f, a.reps))
        m = {k: statistics.median(v) for k, v in t.items()}
        print(f"T = {T}: index lists equal to torch's {agree * 100:.2f} %, max |retrieve k=8 - torch| {ydiff:.2e}; workspace "
              f"k=1 {bank.workspace_bytes(T) / 2 ** 20:.1f} MiB, k=8 {bank.topk_workspace_bytes(T, 8) / 2 ** 20:.1f} MiB")
        for k in fns:
            print(f"  {k:20s} {m[k]:10.1f} us [{min(t[k]):.1f}..{max(t[k]):.1f}] | allocator peak over one call "
                  f"{temp[k] / 2 ** 20:8.1f} MiB", flush=True)
        print("  " + ", ".join(f"search_topk k={k} / search x{m[f'search_topk k={k}'] / m['search']:.3f}" for k in (2, 4, 8)) +
              f"; retrieve k=8 / retrieve k=1 x{m['retrieve k=8'] / m['retrieve k=1']:.3f}; torch retrieve k=8 / retrieve k=8 "
              f"x{m['torch retrieve k=8'] / m['retrieve k=8']:.2f}", flush=True)


if __name__ == "__main__":
    main()
