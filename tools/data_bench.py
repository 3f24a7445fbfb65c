#!/usr/bin/env python3
"""Time the training-data path (csrc/data.hip, jatsr_amd.data, jatsr_amd.fit) with HIP events after warm-up, at the
product shape B = 28, C = 1024, T = 1378 with odd crop starts and odd file lengths:
    python tools/data_bench.py [--runs 25] [--reps 10] [--skip-loop]
1. jat_latent_gather (one launch, tables prepared): us and GB/s over the 474.1 MB it has to move, against
   (A) the composed device path: torch.stack of the fp16 slices -> .float() -> jat_channel_affine, for HR and LR;
   (B) the reference's path: the fp32 crops in pinned host memory -> device copy -> (x - mean) / std in torch, twice.
2. jat_train_monitor against the same five figures from torch reductions on the same tensors (no host read in either).
3. The step time of fit's inner loop (`fit.loop_step`: gather + prefetch + Trainer.step_normalised) on a resident synthetic
   data set at full v3mod2 size, plain steps and logging steps apart, against Trainer.step_normalised on two fixed
   tensors; host clock around steps that end in the step's own synchronising read, blocks of steps alternating.
Every figure is the median of `--runs` windows with their minimum and maximum; the methods alternate window by window."""
import argparse
import hashlib
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, C, T = 28, 1024, 1378
GATHER_BYTES = 2 * B * C * T * (2 + 4)          # fp16 in, fp32 out, both tensors: 474.1 MB


def window(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3      # us


def compare(fns, runs, reps, warm=3):
    for fn in fns.values():
        for _ in range(warm):
            fn()
    t = {k: [] for k in fns}
    for _ in range(runs):
        for k, fn in fns.items():
            t[k].append(window(fn, reps))
    return t


def show(name, v, extra=""):
    print(f"  {name:34s} {statistics.median(v):10.1f} us  [{min(v):.1f} .. {max(v):.1f}]{extra}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--steps", type=int, default=10, help="steps per block of the loop measurement")
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--skip-loop", action="store_true")
    a = ap.parse_args()
    import torch
    from jatsr_amd import _lib as L
    from jatsr_amd import fit as F
    from jatsr_amd import io as jio
    from jatsr_amd.data import LatentStore, train_batch_plan
    from jatsr_amd.sampler import channel_affine
    from jatsr_amd.train import train_monitor
    L.require_gpu()
    print(f"library {os.path.basename(L.LIB_PATH)} sha256 {hashlib.sha256(open(L.LIB_PATH, 'rb').read()).hexdigest()[:16]}")
    dev = torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(0)
    lengths = [2001 + 2 * (7 * i % 50) for i in range(B)]                      # odd
    starts = [1 + 2 * (((n - T - 1) // 2) * (i % 5) // 4) for i, n in enumerate(lengths)]   # odd, from 1 to len - T
    assert all(s % 2 == 1 and s + T <= n for s, n in zip(starts, lengths))
    hr_src = [torch.randn(C, n, device=dev, generator=g).half() for n in lengths]
    lr_src = [torch.randn(C, n, device=dev, generator=g).half() for n in lengths]
    stats = {k: (torch.rand(C, device=dev, generator=g) + 0.5) for k in ("hr_mean", "hr_std", "lr_mean", "lr_std")}
    table = torch.tensor([[x.data_ptr() for x in hr_src], [x.data_ptr() for x in lr_src], lengths, starts], dtype=torch.int64).cuda()
    out = (torch.empty(B, C, T, device=dev), torch.empty(B, C, T, device=dev))
    pinned = [torch.stack([x[:, s:s + T] for x, s in zip(src, starts)]).float().cpu().pin_memory() for src in (hr_src, lr_src)]
    bc = {k: v.view(1, -1, 1) for k, v in stats.items()}

    def kernel():
        L.check(L.lib().jat_latent_gather(L.ptr(table[0]), L.ptr(table[1]), L.ptr(table[2]), L.ptr(table[3]), L.ptr(stats["hr_mean"]),
                                          L.ptr(stats["hr_std"]), L.ptr(stats["lr_mean"]), L.ptr(stats["lr_std"]), L.ptr(out[0]),
                                          L.ptr(out[1]), B, C, T, L.stream_ptr()))

    def composed():
        h = channel_affine(torch.stack([x[:, s:s + T] for x, s in zip(hr_src, starts)]).float(), stats["hr_mean"], stats["hr_std"])
        l = channel_affine(torch.stack([x[:, s:s + T] for x, s in zip(lr_src, starts)]).float(), stats["lr_mean"], stats["lr_std"])
        return h, l

    def reference():
        h = (pinned[0].to(dev, non_blocking=True) - bc["hr_mean"]) / bc["hr_std"]
        l = (pinned[1].to(dev, non_blocking=True) - bc["lr_mean"]) / bc["lr_std"]
        return h, l

    kernel()
    same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(out, composed()))
    print(f"1. batch assembly, B {B} C {C} T {T}, odd starts (kernel == composed path bit for bit: {same})")
    t = compare({"kernel": kernel, "composed": composed, "reference": reference}, a.runs, a.reps)
    mk = statistics.median(t["kernel"])
    show("jat_latent_gather", t["kernel"], f"  {GATHER_BYTES / mk / 1e3:.0f} GB/s over {GATHER_BYTES / 1e6:.1f} MB")
    show("(A) stack + float + 2 affine", t["composed"], f"  x{statistics.median(t['composed']) / mk:.2f}")
    show("(B) pinned fp32 copy + 2 normalise", t["reference"], f"  x{statistics.median(t['reference']) / mk:.2f}")

    pred = out[0] + 0.3 * torch.randn(B, C, T, device=dev, generator=g)
    target, cond = out

    def monitor():
        return train_monitor(pred, target, cond)

    def torch_reductions():
        snr = 10 * torch.log10((target ** 2).mean() / (((pred - target) ** 2).mean() + 1e-8))
        return pred.mean(), pred.std(), snr, cond.std().clamp(0.5, 2.0)

    print("2. step monitor, three [28, 1024, 1378] fp32 tensors")
    t = compare({"kernel": monitor, "torch": torch_reductions}, a.runs, a.reps)
    mk = statistics.median(t["kernel"])
    show("jat_train_monitor", t["kernel"], f"  {3 * B * C * T * 4 / mk / 1e3:.0f} GB/s")
    show("torch reductions", t["torch"], f"  x{statistics.median(t['torch']) / mk:.2f}")
    if a.skip_loop:
        return
    del pinned, hr_src, lr_src
    with tempfile.TemporaryDirectory() as d:
        os.makedirs(os.path.join(d, "train"))
        cpu_g = torch.Generator().manual_seed(1)
        for i in range(32):
            n = 1500 + 37 * i
            jio.save_latent_file(os.path.join(d, "train", f"clip_{i:03d}.pt"), hr_latent=torch.randn(C, n, generator=cpu_g),
                                 lr_latent=torch.randn(C, n, generator=cpu_g))
        store = LatentStore(d, "train", T, dev)
    args = F.build_parser().parse_args([])
    trainer = F.build_trainer(args, F.build_model(args, dev), 10 ** 6)
    stats = {k: v.contiguous() for k, v in stats.items()}
    n_plans = a.steps * a.blocks * 2 + 8
    plans = [train_batch_plan(store.lengths, T, [(j * B + k) % (32 * 6) for k in range(B)], 42, 0) for j in range(n_plans)]
    fixed = store.batch(*plans[0], stats)
    pos = [0]

    def loop(monitor):
        t0 = time.perf_counter()
        F.loop_step(trainer, store, plans, pos[0] % (n_plans - 1), stats, 1e-5, monitor)
        pos[0] += 1
        return (time.perf_counter() - t0) * 1e3

    def bare(_):
        t0 = time.perf_counter()
        trainer.step_normalised(fixed[0], fixed[1], monitor=False, lr=1e-5)
        return (time.perf_counter() - t0) * 1e3

    for fn in (bare, loop):
        for _ in range(3):
            fn(False)
    loop(True)
    t = {"bare": [], "loop": [], "log": []}
    for _ in range(a.blocks):
        t["bare"] += [bare(False) for _ in range(a.steps)]
        t["loop"] += [loop(False) for _ in range(a.steps)]
        t["log"] += [loop(True) for _ in range(max(a.steps // 2, 1))]
    print(f"3. training step at full v3mod2 size ({trainer.workspace_bytes() / 2**30:.1f} GiB workspace), ms per step")
    for name, k in (("step_normalised, fixed tensors", "bare"), ("fit loop step", "loop"), ("fit loop step, logging", "log")):
        v = t[k]
        print(f"  {name:34s} {statistics.median(v):10.3f} ms  [{min(v):.3f} .. {max(v):.3f}]  ({len(v)} steps)")
    mb, ml = statistics.median(t["bare"]), statistics.median(t["loop"])
    print(f"  loop - bare = {ml - mb:+.3f} ms ({100 * (ml - mb) / mb:+.2f} %); inside the bare step's min..max: {min(t['bare']) <= ml <= max(t['bare'])}")


if __name__ == "__main__":
    main()
