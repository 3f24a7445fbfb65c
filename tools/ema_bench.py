#!/usr/bin/env python3
"""What the EMA of the weights costs per optimiser step, at the full parameter count, three ways in one process:

    (a) jat_trainer_optim without an average                         (what ships with ema_decay=None)
    (b) jat_trainer_optim with the average fused into the AdamW pass (Trainer(ema_decay=...))
    (c) (a) followed by ema.lerp_(params, 1 - d) in torch            (the way it is usually written)

The three are interleaved round by round, in rotating order, and timed with device events around each call on an idle device
(gradient norm + AdamW + the re-pack's casts on the step's stream; the re-pack is the same work in all three).  The kernel pair on its own (jat_k_adamw / jat_k_adamw_ema:
gradient norm + AdamW on the same buffers) is timed the same way.  Prints the median and the 10 % / 90 % points of each, the
paired differences, and the sha256 of the library.

    python tools/ema_bench.py --rounds 40
"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="v3mod2")
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--decay", type=float, default=0.9999)
    args = ap.parse_args()
    import numpy as np
    import torch

    import jatsr_amd
    import jatsr_amd._lib as L
    import jatsr_amd.recipe as recipe
    from jatsr_amd.train import Trainer

    L.require_gpu()
    cfg = recipe.CONFIGS[args.config]
    model = jatsr_amd.JaT_AudioSR_V3(**cfg, dropout=0.0, drop_path_rate=0.0).to("cuda")
    tr = Trainer(model, batch_size=2, frames=128, seed=1, use_grad_scaler=False, ema_decay=args.decay, ema_warmup=False)
    n = tr.params.numel()
    g = torch.Generator(device="cuda").manual_seed(1)
    tr.grads.normal_(0.0, 1e-3, generator=g)
    lib, s = L.lib(), L.stream_ptr()
    hyper = (5e-5, 0.9, 0.999, 1e-8, 0.1, 1.0, 1.0)
    wk = torch.empty(4104, dtype=torch.uint8, device="cuda")
    step = [0]

    def optim(ema):
        L.check(lib.jat_trainer_set_ema(tr.ptr, L.ptr(tr.ema) if ema else None, args.decay))
        step[0] += 1
        L.check(lib.jat_trainer_optim(tr.ptr, *hyper, step[0], None, s))

    def lerp():
        optim(False)
        tr.ema.lerp_(tr.params, 1.0 - args.decay)

    def kernel(ema):
        step[0] += 1
        if ema:
            L.check(lib.jat_k_adamw_ema(L.ptr(tr.params), L.ptr(tr.grads), L.ptr(tr.exp_avg), L.ptr(tr.exp_avg_sq), L.ptr(tr.ema), n,
                                        *hyper, args.decay, step[0], None, L.ptr(wk), wk.numel(), s))
        else:
            L.check(lib.jat_k_adamw(L.ptr(tr.params), L.ptr(tr.grads), L.ptr(tr.exp_avg), L.ptr(tr.exp_avg_sq), n, *hyper, step[0],
                                    None, L.ptr(wk), wk.numel(), s))
    legs = {"optim": lambda: optim(False), "optim_fused_ema": lambda: optim(True), "optim_then_lerp": lerp,
            "kernel_adamw": lambda: kernel(False), "kernel_adamw_ema": lambda: kernel(True)}
    times = {k: [] for k in legs}
    names = list(legs)
    for r in range(args.warmup + args.rounds):
        for name in names[r % len(names):] + names[:r % len(names)]:      # every leg follows every other in turn
            fn = legs[name]
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            # the re-pack rebuilds the transposed copies on the trainer's second stream, past the end event: without this wait
            # they would run under the NEXT leg and be charged to it
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            b.synchronize()
            if r >= args.warmup:
                times[name].append(a.elapsed_time(b))
    assert bool(torch.isfinite(tr.params).all()) and bool(torch.isfinite(tr.ema).all())

    def summary(x):
        x = np.asarray(x)
        return dict(median_ms=round(float(np.median(x)), 4), p10_ms=round(float(np.percentile(x, 10)), 4),
                    p90_ms=round(float(np.percentile(x, 90)), 4))
    out = {k: summary(v) for k, v in times.items()}
    for name, (x, y) in {"fused_minus_plain": ("optim_fused_ema", "optim"), "lerp_minus_plain": ("optim_then_lerp", "optim"),
                         "lerp_minus_fused": ("optim_then_lerp", "optim_fused_ema"),
                         "kernel_ema_minus_plain": ("kernel_adamw_ema", "kernel_adamw")}.items():
        out[name] = summary(np.asarray(times[x]) - np.asarray(times[y]))      # paired by round
    with open(L.LIB_PATH, "rb") as f:
        sha = hashlib.sha256(f.read()).hexdigest()
    print(json.dumps(dict(config=args.config, parameters=int(sum(p.numel() for p in model.parameters())), flat_floats=n,
                          rounds=args.rounds, decay=args.decay, library=os.path.basename(L.LIB_PATH), sha256=sha, **out)))
    for k, v in out.items():
        print(f"{k:>24}: median {v['median_ms']:8.3f} ms   (10 % {v['p10_ms']:.3f}, 90 % {v['p90_ms']:.3f})")


if __name__ == "__main__":
    main()
