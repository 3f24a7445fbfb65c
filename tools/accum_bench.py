#!/usr/bin/env python3
"""What gradient accumulation costs per optimiser step at the workload's shape (v3mod2, B = 28, T = 1378, k = 4), four ways in one
process, all through the C ABI on one trainer:

    fused      k x jat_trainer_fwd_bwd_ex (overwrite, then JAT_FB_ACCUMULATE) + one jat_trainer_optim    (Trainer(grad_accum_steps=k))
    overwrite  the same k calls without the accumulate flag + one step: the same launches minus the read of the resident gradient
               (computes nothing useful; fused - overwrite is what the in-kernel adds cost)
    plain      k plain steps (jat_trainer_fwd_bwd + jat_trainer_optim each): the same samples without accumulation
    composed   the alternative from the outside: plain jat_trainer_fwd_bwd, a sixth flat torch buffer and one torch pass over it per
               micro-batch (copy_, add_, ..., and the last one added back into grads, the cheapest arrangement), then one step

The legs are interleaved round by round, in rotating order, and timed with device events around each leg on an idle device.
Prints the median and the 10 % / 90 % points of each, the paired differences, and the sha256 of the library.

    python tools/accum_bench.py --rounds 10
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="v3mod2")
    ap.add_argument("--batch", type=int, default=28)
    ap.add_argument("--frames", type=int, default=1378)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import numpy as np
    import torch

    import jatsr_amd
    import jatsr_amd._lib as L
    import jatsr_amd.recipe as recipe
    from jatsr_amd.train import Trainer

    L.require_gpu()
    cfg = recipe.CONFIGS[args.config]
    B, T, k, Cin = args.batch, args.frames, args.k, cfg["input_channels"]
    model = jatsr_amd.JaT_AudioSR_V3(**cfg, dropout=0.0, drop_path_rate=0.0).to("cuda")
    tr = Trainer(model, batch_size=B, frames=T, seed=1, use_grad_scaler=False)
    g = torch.Generator(device="cuda").manual_seed(1)
    z_t, cond, target = (torch.randn((B, Cin, T), device="cuda", generator=g) for _ in range(3))
    t = torch.rand(B, device="cuda", generator=g)
    sixth = torch.zeros_like(tr.grads)
    lib, s = L.lib(), L.stream_ptr()
    scale = 4096.0 if L.operand_dtype() == "fp16" else 1.0
    step = [0]

    def fb(flags):
        L.check(lib.jat_trainer_fwd_bwd_ex(tr.ptr, L.ptr(z_t), L.ptr(t), L.ptr(cond), L.ptr(target), None, scale, C.c_uint64(7),
                                           L.ptr(tr._scal), None, flags, s))

    def optim(div):
        step[0] += 1
        L.check(lib.jat_trainer_optim(tr.ptr, 1e-6, 0.9, 0.999, 1e-8, 0.1, 1.0, scale * div, step[0], None, s))

    def fused():
        for j in range(k):
            fb((L.FB_ACCUMULATE if j > 0 else 0) | (L.FB_NO_HOOK if j < k - 1 else 0))
        optim(k)

    def overwrite():
        for j in range(k):
            fb(L.FB_NO_HOOK if j < k - 1 else 0)
        optim(1)

    def plain():
        for _ in range(k):
            fb(0)
            optim(1)

    def composed():
        for j in range(k):
            fb(0)
            if j == 0:
                sixth.copy_(tr.grads)
            elif j < k - 1:
                sixth.add_(tr.grads)
            else:
                tr.grads.add_(sixth)
        optim(k)
    legs = {"fused": fused, "overwrite": overwrite, "plain": plain, "composed": composed}
    times = {name: [] for name in legs}
    names = list(legs)
    for r in range(args.warmup + args.rounds):
        for name in names[r % len(names):] + names[:r % len(names)]:      # every leg follows every other in turn
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()      # the re-pack's transposed copies run on the second stream, past the end event
            a.record()
            legs[name]()
            b.record()
            b.synchronize()
            if r >= args.warmup:
                times[name].append(a.elapsed_time(b))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(tr.params).all()) and bool(torch.isfinite(tr.grads).all())

    def summary(x):
        x = np.asarray(x)
        return dict(median_ms=round(float(np.median(x)), 3), p10_ms=round(float(np.percentile(x, 10)), 3),
                    p90_ms=round(float(np.percentile(x, 90)), 3))
    out = {name: summary(v) for name, v in times.items()}
    for name, (x, y) in {"fused_minus_composed": ("fused", "composed"), "fused_minus_plain": ("fused", "plain"),
                         "fused_minus_overwrite": ("fused", "overwrite")}.items():
        out[name] = summary(np.asarray(times[x]) - np.asarray(times[y]))      # paired by round
    out["accumulate_cost_per_micro_batch_ms"] = round(out["fused_minus_overwrite"]["median_ms"] / max(k - 1, 1), 3)
    with open(L.LIB_PATH, "rb") as f:
        sha = hashlib.sha256(f.read()).hexdigest()
    print(json.dumps(dict(config=args.config, batch=B, frames=T, k=k, flat_floats=tr.grads.numel(), rounds=args.rounds,
                          library=os.path.basename(L.LIB_PATH), sha256=sha, **out)))
    for name, v in out.items():
        if isinstance(v, dict):
            print(f"{name:>24}: median {v['median_ms']:9.3f} ms   (10 % {v['p10_ms']:.3f}, 90 % {v['p90_ms']:.3f})")


if __name__ == "__main__":
    main()
