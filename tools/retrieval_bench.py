#!/usr/bin/env python3
"""Time latent retrieval (csrc/retrieval.hip) with HIP events on one stream after warm-up:
    python tools/retrieval_bench.py [--keys 100000] [--frames 1378 4096] [--reps 20] [--rounds 11]
at C = 1024, B = 1:
(a) LatentBank.search (queries normalised already) and LatentBank.retrieve (search with the normalisation in the loader +
    the de-normalising blend, index rate 0.4);
(b) the same as a user composes it from PyTorch on the same GPU, with the bank kept as an fp32 [N, C] tensor:
    G = q @ keys32.T, G * -2 + |k|^2, argmin (+ |q|^2 for the distance); for retrieve also the per-channel normalisation
    ahead of it and values[idx] * std + mean, torch.lerp behind it;
(c) (b) with the bank kept in fp16 and converted per call (`keys.float()`), what a user short of memory would write.
The variants alternate in rounds within one process; the median round counts and the range of the rounds is printed, so that
a ratio inside it reads as a tie.  Temporary bytes: ours from the workspace query function plus the outputs, torch's from
the allocator's peak over one call.  How many indices agree is printed too (fp32 GEMM rounding may move near-ties).
For a kernel table run it on its own under
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- python tools/retrieval_bench.py --reps 5 --rounds 1"""
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


def peak_temp_bytes(fn):
    import torch
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=100_000)
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--frames", type=int, nargs="+", default=[1378, 4096])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--rate", type=float, default=0.4)
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
    print(f"bank: {N} x {C} fp16 = {N * C * 2 / 2 ** 20:.0f} MiB (+ {N * 4 / 2 ** 10:.0f} KiB norms); torch's fp32 copy {N * C * 4 / 2 ** 20:.0f} MiB")
    for T in a.frames:
        xn = torch.randn(1, C, T, device="cuda", generator=g)                 # normalised queries
        x = (xn * std[None, :, None] + mean[None, :, None]).contiguous()      # de-normalised latent

        def ours_search():
            return bank.search(xn)

        def ours_retrieve():
            return bank.retrieve(x, a.rate)

        def torch_search(q=None, resident=True):
            q = xn[0].T if q is None else q
            G = q @ (keys32 if resident else keys16.float()).T
            G.mul_(-2.0).add_(norms[None, :])
            d, idx = G.min(dim=1)
            return idx, (d + (q * q).sum(1)).clamp_min_(0.0)

        def torch_search_fp16_bank():
            return torch_search(resident=False)

        def torch_retrieve():
            q = ((x[0] - mean[:, None]) / std[:, None]).T
            idx, _ = torch_search(q)
            v = keys16[idx].float() * std[None, :] + mean[None, :]
            return torch.lerp(x, v.T[None], a.rate)

        i_ours, d_ours = ours_search()
        i_torch, d_torch = torch_search()
        agree = float((i_ours.view(-1) == i_torch.view(-1)).float().mean())
        ddiff = float((d_ours.view(-1) - d_torch).abs().max())
        ydiff = float((ours_retrieve() - torch_retrieve()).abs().max())
        fns = {"search": ours_search, "torch search": torch_search, "torch search, fp16 bank": torch_search_fp16_bank,
               "retrieve": ours_retrieve, "torch retrieve": torch_retrieve}
        temp = {k: peak_temp_bytes(f) for k, f in fns.items()}
        ours_bytes = bank.workspace_bytes(T) + 8 * T
        for f in fns.values():                      # warm-up: code objects, the GEMM library's choices
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        t = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, f in fns.items():
                t[k].append(timed(f, a.reps))
        m = {k: statistics.median(v) for k, v in t.items()}
        flop = 2.0 * T * N * C
        print(f"T = {T}: indices equal to torch's {agree * 100:.2f} %, max |dist2 - torch| {ddiff:.2e}, max |retrieve - torch| {ydiff:.2e}")
        for k in fns:
            extra = ""
            if k == "search":
                extra = (f" | {flop / m[k] * 1e-6:.0f} TFLOP/s of the contraction, {2 * flop / m[k] * 1e-6:.0f} TFLOP/s issued as fp16 "
                         f"MFMA (two passes) | workspace + outputs {ours_bytes / 2 ** 20:.1f} MiB")
            print(f"  {k:24s} {m[k]:10.1f} us [{min(t[k]):.1f}..{max(t[k]):.1f}] | allocator peak over one call "
                  f"{temp[k] / 2 ** 20:8.1f} MiB{extra}", flush=True)
        print(f"  torch search / search x{m['torch search'] / m['search']:.2f}, torch retrieve / retrieve "
              f"x{m['torch retrieve'] / m['retrieve']:.2f}", flush=True)


if __name__ == "__main__":
    main()
