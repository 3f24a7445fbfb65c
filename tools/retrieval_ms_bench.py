#!/usr/bin/env python3
"""Time multi-scale latent retrieval (csrc/retrieval_ms.hip) with HIP events on one stream after warm-up:
    python tools/retrieval_ms_bench.py [--keys 100000] [--frames 1378 4096] [--reps 20] [--rounds 11]
at C = 1024, B = 1, scales (1, 2, 4), `--keys` rows per scale:
(a) MultiScaleBank.retrieve at k = 1 and k = 8 against the single-scale LatentBank.retrieve and against the same algorithm as a
    user composes it from PyTorch on the same GPU around the library's own search: the per-channel normalisation,
    F.avg_pool1d, LatentBank.search / search_topk per scale, the gather of the value rows (for k = 8 with the inverse-square
    weights), values * std + mean, F.interpolate(mode="linear"), the weighted sum, torch.lerp.  The torch side runs at T
    rounded down to a multiple of 8, where its pooling and interpolation are the same functions as ours;
(b) the two new per-call kernels alone, as bytes moved over time: pool_frames (x read once, the three pooled tensors written)
    and mix_scales (x and the three tracks read, y written), against the measured HBM copy rate of the MI355X;
(c) what the estimates of the design said: the three searches against one (1 + 1/2 + 1/4 = 1.75 x estimated), and pooling plus
    mix (a few tens of microseconds estimated at T = 4096).
The variants alternate in rounds within one process; the median round counts and the range of the rounds is printed, so that
a ratio inside it reads as a tie.  Temporary bytes: the allocator's peak over one call."""
import argparse
import hashlib
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from retrieval_bench import peak_temp_bytes, timed  # noqa: E402

HBM_COPY_TBS = 6.29          # measured float4 copy rate of the MI355X (8.0 TB/s by specification)
SCALES = (1, 2, 4)


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
    import torch.nn.functional as F
    from jatsr_amd import _lib
    from jatsr_amd import retrieval as RT
    _lib.require_gpu()
    print(f"library {os.path.basename(_lib.LIB_PATH)} sha256 {hashlib.sha256(open(_lib.LIB_PATH, 'rb').read()).hexdigest()[:16]}")
    N, C = a.keys, a.channels
    g = torch.Generator(device="cuda").manual_seed(0)
    mean = torch.randn(C, device="cuda", generator=g) * 0.2
    std = torch.rand(C, device="cuda", generator=g) + 0.5
    stats = {"hr_mean": mean, "hr_std": std, "lr_mean": mean, "lr_std": std}
    bank = RT.MultiScaleBank(C, N, scales=SCALES)
    for s, b in zip(SCALES, bank.banks):
        b._set_stats(stats)
        b.load_rows((torch.randn(N, C, device="cuda", generator=g) / s ** 0.5).half())    # a mean of s frames: variance 1 / s
    single = bank.banks[0]
    rows16 = [b.rows("values")[0] for b in bank.banks]
    w = torch.tensor(bank.weights, device="cuda")
    print(f"banks: {len(SCALES)} x {N} x {C} fp16 = {len(SCALES) * N * C * 2 / 2 ** 20:.0f} MiB")
    for T in a.frames:
        T8 = T - T % 8
        xn = torch.randn(1, C, T, device="cuda", generator=g)
        x = (xn * std[None, :, None] + mean[None, :, None]).contiguous()
        x8 = x[:, :, :T8].contiguous()

        def torch_ms(k):
            q = (x8 - mean[None, :, None]) / std[None, :, None]
            m = None
            for i, (s, b) in enumerate(zip(SCALES, bank.banks)):
                qs = q if s == 1 else F.avg_pool1d(q, s)
                if k == 1:
                    idx, _ = b.search(qs)
                    v = rows16[i][idx[0].long()].float()                                  # [Ts, C]
                else:
                    idx, d = b.search_topk(qs, k)
                    d = d[0].clamp_min(1e-6)
                    u = (d[:, :1] / d).square_()
                    v = (rows16[i][idx[0].long()].float() * (u / u.sum(1, keepdim=True))[:, :, None]).sum(1)
                v = (v * std[None, :] + mean[None, :]).T[None]                            # [1, C, Ts]
                up = v if s == 1 else F.interpolate(v, scale_factor=s, mode="linear", align_corners=False)
                m = up * w[i] if m is None else m + up * w[i]
            return torch.lerp(x8, m, a.rate)

        pooled = RT.pool_frames(x, (2, 4), mean, std)
        tracks = [x.clone()] + [p.clone() for p in pooled]

        def searches():
            single.search(x, mean, std)
            for p, b in zip(pooled, bank.banks[1:]):
                b.search(p)

        fns = {"single retrieve k=1": lambda: single.retrieve(x, a.rate),
               "single retrieve k=8": lambda: single.retrieve(x, a.rate, k=8),
               "multi retrieve k=1": lambda: bank.retrieve(x, a.rate),
               "multi retrieve k=8": lambda: bank.retrieve(x, a.rate, k=8),
               f"multi retrieve k=1 T={T8}": lambda: bank.retrieve(x8, a.rate),
               f"multi retrieve k=8 T={T8}": lambda: bank.retrieve(x8, a.rate, k=8),
               f"torch composition k=1 T={T8}": lambda: torch_ms(1),
               f"torch composition k=8 T={T8}": lambda: torch_ms(8),
               "search at scale 1": lambda: single.search(x, mean, std),
               "searches at scales 1, 2, 4": searches,
               "pool_frames (2, 4)": lambda: RT.pool_frames(x, (2, 4), mean, std, outs=pooled),
               "mix_scales (1, 2, 4)": lambda: RT.mix_scales(x, SCALES, tracks, bank.weights, a.rate)}
        diff = {k: float((bank.retrieve(x8, a.rate, k=k) - torch_ms(k)).abs().max()) for k in (1, 8)}
        temp = {k: peak_temp_bytes(f) for k, f in fns.items()}
        for f in fns.values():
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        t = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, f in fns.items():
                t[k].append(timed(f, a.reps))
        m = {k: statistics.median(v) for k, v in t.items()}
        print(f"T = {T}: max |multi retrieve - torch composition| at T = {T8}: k=1 {diff[1]:.2e}, k=8 {diff[8]:.2e}")
        for k in fns:
            print(f"  {k:34s} {m[k]:10.1f} us [{min(t[k]):.1f}..{max(t[k]):.1f}] | allocator peak over one call "
                  f"{temp[k] / 2 ** 20:8.1f} MiB", flush=True)
        el = C * 4                                                                        # bytes per frame of one [C, T] fp32 tensor
        pool_bytes = el * (T + sum(RT.pooled_length(T, s) for s in (2, 4)))
        mix_bytes = el * (2 * T + sum(RT.pooled_length(T, s) for s in SCALES))
        for name, nbytes in (("pool_frames (2, 4)", pool_bytes), ("mix_scales (1, 2, 4)", mix_bytes)):
            rate = nbytes / (m[name] * 1e-6) / 1e12
            print(f"  {name}: {nbytes / 1e6:.1f} MB moved, {rate:.2f} TB/s = {100 * rate / HBM_COPY_TBS:.0f} % of the measured "
                  f"{HBM_COPY_TBS} TB/s copy rate (launch included)")
        print(f"  multi / single retrieve: k=1 x{m['multi retrieve k=1'] / m['single retrieve k=1']:.2f}, k=8 "
              f"x{m['multi retrieve k=8'] / m['single retrieve k=8']:.2f}; torch composition / multi retrieve at T = {T8}: k=1 "
              f"x{m[f'torch composition k=1 T={T8}'] / m[f'multi retrieve k=1 T={T8}']:.2f}, k=8 "
              f"x{m[f'torch composition k=8 T={T8}'] / m[f'multi retrieve k=8 T={T8}']:.2f}; three searches / one "
              f"x{m['searches at scales 1, 2, 4'] / m['search at scale 1']:.2f} (estimated 1.75); pool + mix "
              f"{m['pool_frames (2, 4)'] + m['mix_scales (1, 2, 4)']:.1f} us", flush=True)


if __name__ == "__main__":
    main()
