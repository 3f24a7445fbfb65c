#!/usr/bin/env python3
"""What the V3-MOD3 loss (Charbonnier + latent perceptual loss, `Trainer(loss="charbonnier_latent")`) costs at the workload's shape
(v3mod2, LayerNorm model, B = 28, T = 1378), in one process:

  step legs, one trainer, the loss switched by jat_trainer_set_loss_ex between legs (jat_trainer_fwd_bwd + jat_trainer_optim each):
    mse_latent    recon_eps 0, weight 1: the v3mod2 loss on the kernels it always ran (the baseline)
    charb_latent  recon_eps 1e-6, weight 1: the general instances of the same kernels
  loss legs, on the step's own [B * C, T] tensors:
    fused         jat_k_latent_loss_ex: the Charbonnier term inside the loss kernels
    composed      the alternative from the outside: jat_k_latent_loss (MSE + latent), then torch takes the MSE gradient out of dpred
                  and puts the Charbonnier gradient in, and adds the two scalars on the device

The legs are interleaved round by round, in rotating order, timed with device events around each leg on an idle device.  Prints the
median and the 10 % / 90 % points of each, the paired differences, and the sha256 of the library.

    python tools/mod3_bench.py --rounds 10
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
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--eps", type=float, default=1e-6)
    ap.add_argument("--reconstruction-weight", type=float, default=1.0)
    args = ap.parse_args()
    import numpy as np
    import torch

    import jatsr_amd
    import jatsr_amd._lib as L
    import jatsr_amd.recipe as recipe
    from jatsr_amd.train import Trainer

    L.require_gpu()
    cfg = recipe.CONFIGS[args.config]
    B, T, Cin, eps, rw = args.batch, args.frames, cfg["input_channels"], args.eps, args.reconstruction_weight
    model = jatsr_amd.JaT_AudioSR_V2(**cfg, dropout=0.0, drop_path_rate=0.0).to("cuda")
    tr = Trainer(model, batch_size=B, frames=T, seed=1, use_grad_scaler=False, latent_loss_weight=0.3)
    g = torch.Generator(device="cuda").manual_seed(1)
    z_t, cond, target = (torch.randn((B, Cin, T), device="cuda", generator=g) for _ in range(3))
    t = torch.rand(B, device="cuda", generator=g)
    lib, s = L.lib(), L.stream_ptr()
    scale = 4096.0 if L.operand_dtype() == "fp16" else 1.0
    weights = tuple(tr.latent_loss.values())           # lw, fw, mw, cw, the three band ratios
    lw = weights[0]
    step = [0]

    def train_step(recon_eps, recon_weight):
        L.check(lib.jat_trainer_set_loss_ex(tr.ptr, recon_eps, recon_weight, *weights))
        L.check(lib.jat_trainer_fwd_bwd(tr.ptr, L.ptr(z_t), L.ptr(t), L.ptr(cond), L.ptr(target), L.ptr(cond), scale, C.c_uint64(7),
                                        L.ptr(tr._scal), None, s))
        step[0] += 1
        L.check(lib.jat_trainer_optim(tr.ptr, 1e-6, 0.9, 0.999, 1e-8, 0.1, 1.0, scale, step[0], None, s))

    # the loss legs: the prediction of one forward, so that the tensors are the step's own
    pred = torch.empty_like(z_t)
    L.check(lib.jat_trainer_fwd_bwd(tr.ptr, L.ptr(z_t), L.ptr(t), L.ptr(cond), L.ptr(target), L.ptr(cond), scale, C.c_uint64(7),
                                    L.ptr(tr._scal), L.ptr(pred), s))
    rows, n = B * Cin, B * Cin * T
    dpred_f, dpred_c = torch.empty_like(pred), torch.empty_like(pred)
    out_f, out_c = torch.zeros(6, device="cuda"), torch.zeros(6, device="cuda")
    total_c = torch.zeros((), device="cuda")
    work = torch.empty((T * 8 + 255) // 256 * 256 + rows * 32, dtype=torch.uint8, device="cuda")

    def fused():
        L.check(lib.jat_k_latent_loss_ex(L.ptr(pred), L.ptr(target), L.ptr(cond), L.ptr(dpred_f), L.ptr(out_f), rows, T, eps, rw,
                                         *weights, 1.0, L.ptr(work), work.numel(), s))

    def composed():
        L.check(lib.jat_k_latent_loss(L.ptr(pred), L.ptr(target), L.ptr(cond), L.ptr(dpred_c), L.ptr(out_c), rows, T, *weights, 1.0,
                                      L.ptr(work), work.numel(), s))
        e = pred - target
        r = torch.sqrt(e * e + eps)
        dpred_c.add_(e, alpha=-2.0 / n)                 # the MSE gradient out
        dpred_c.addcdiv_(e, r, value=rw / n)            # the Charbonnier gradient in
        total_c.copy_(rw * r.mean() + lw * out_c[5])

    legs = {"mse_latent": lambda: train_step(0.0, 1.0), "charb_latent": lambda: train_step(eps, rw), "fused": fused,
            "composed": composed}
    times = {name: [] for name in legs}
    names = list(legs)
    for r_ in range(args.warmup + args.rounds):
        for name in names[r_ % len(names):] + names[:r_ % len(names)]:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()      # the re-pack's transposed copies run on the second stream, past the end event
            a.record()
            legs[name]()
            b.record()
            b.synchronize()
            if r_ >= args.warmup:
                times[name].append(a.elapsed_time(b))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(tr.params).all()) and bool(torch.isfinite(tr.grads).all())
    # the two loss legs computed the same thing
    agree = dict(dpred_rel_l2=float((dpred_f.double() - dpred_c.double()).norm() / dpred_c.double().norm()),
                 total_fused=float(out_f[0]), total_composed=float(total_c))

    def summary(x):
        x = np.asarray(x)
        return dict(median_ms=round(float(np.median(x)), 3), p10_ms=round(float(np.percentile(x, 10)), 3),
                    p90_ms=round(float(np.percentile(x, 90)), 3))
    out = {name: summary(v) for name, v in times.items()}
    for name, (x, y) in {"charb_latent_minus_mse_latent": ("charb_latent", "mse_latent"), "fused_minus_composed": ("fused", "composed")}.items():
        out[name] = summary(np.asarray(times[x]) - np.asarray(times[y]))      # paired by round
    with open(L.LIB_PATH, "rb") as f:
        sha = hashlib.sha256(f.read()).hexdigest()
    print(json.dumps(dict(config=args.config, batch=B, frames=T, eps=eps, reconstruction_weight=rw, rounds=args.rounds,
                          library=os.path.basename(L.LIB_PATH), sha256=sha, agreement=agree, **out)))
    for name, v in out.items():
        print(f"{name:>30}: median {v['median_ms']:9.3f} ms   (10 % {v['p10_ms']:.3f}, 90 % {v['p90_ms']:.3f})")


if __name__ == "__main__":
    main()
