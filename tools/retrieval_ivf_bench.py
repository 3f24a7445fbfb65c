#!/usr/bin/env python3
"""Time the IVF index over a retrieval bank (csrc/retrieval_ivf.hip) with HIP events on one stream after warm-up:
    python tools/retrieval_ivf_bench.py [--rows 1000000] [--channels 1024] [--frames 1378 4096] [--reps 3] [--rounds 5]
on synthetic rows only (the uneven Gaussian mixture of tools/retrieval_km_bench.py; no audio, no trained weights):
(a) the build: k-means with RVC's default number of lists, one `assign`, one `group_rows`, each on its own;
(b) `IVFBank.search_topk` at nprobe in {1, 8} and k in {1, 8} against `LatentBank.search_topk` (the flat kernel of
    csrc/retrieval.hip, unchanged) on the same grouped bank in the same process; the coarse stage is timed on its own
    (`centroids.search_topk`, the very call stage 1 makes) and the rest (query planes + list scan) is the difference of the
    medians; the scan is set against its byte bound, probed rows x 2 C bytes at the measured copy rate;
(c) recall on held-out queries of the same mixture: the share whose flat nearest row is returned at nprobe in {1, 2, 4, 8}, and
    the mean overlap of the k = 8 lists.  Recall is reported, not gated.
The variants alternate in rounds within one process; the median round counts and the range of the rounds is printed."""
import argparse
import hashlib
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from retrieval_bench import timed  # noqa: E402

HBM_COPY_TBS = 6.29          # measured float4 copy rate of the MI355X


def sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()[:16]


def ivf_group_bytes(bank, nlist):
    import ctypes
    from jatsr_amd import _lib
    n = ctypes.c_size_t()
    _lib.check(_lib.lib().jat_bank_group_workspace_bytes(bank._h, nlist, ctypes.byref(n)))
    return n.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--frames", type=int, nargs="+", default=[1378, 4096])
    ap.add_argument("--held-out", type=int, default=20_000)
    ap.add_argument("--lists", type=int, default=None, help="default: min(int(16 sqrt(rows)), rows // 39)")
    ap.add_argument("--kmeans-iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import torch
    from jatsr_amd import _lib
    from jatsr_amd import retrieval as RT
    _lib.require_gpu()
    csrc = os.path.join(os.path.dirname(_lib.LIB_PATH))
    print(f"library {os.path.basename(_lib.LIB_PATH)} sha256 {sha(_lib.LIB_PATH)}; retrieval.hip sha256 "
          f"{sha(os.path.join(csrc, 'retrieval.hip'))} (untouched: the flat search is the one measured before)")
    N, C, held = a.rows, a.channels, a.held_out
    g = torch.Generator(device="cuda").manual_seed(0)
    centres = 2000
    mu = torch.randn(centres, C, device="cuda", generator=g) * 1.5
    w = torch.rand(centres, device="cuda", generator=g) ** 4             # a few heavy components, many light ones
    pick = torch.multinomial(w, N + held, replacement=True, generator=g)
    bank = RT.LatentBank(C, N)
    for lo in range(0, N, 1 << 18):
        n = min(1 << 18, N - lo)
        bank.load_rows((mu[pick[lo:lo + n]] + torch.randn(n, C, device="cuda", generator=g) * 0.5).half())
    q = (mu[pick[N:]] + torch.randn(held, C, device="cuda", generator=g) * 0.5).half().float()   # held out, fp16 values like rows
    nlist = a.lists or RT.default_nlist(N)
    print(f"bank {N} x {C} fp16 = {N * C * 2 / 2 ** 20:.0f} MiB of {centres} uneven components, {nlist} lists requested")

    # (a) the build
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cent, report = RT.kmeans(bank, nlist, iters=a.kmeans_iters, drop_empty=True)
    torch.cuda.synchronize()
    t_km = time.perf_counter() - t0
    idx, _ = cent.assign(bank)
    t_assign = statistics.median(timed(lambda: cent.assign(bank, idx=idx), 1) for _ in range(3))
    grouped, offsets, order = RT.group_rows(bank, idx, len(cent))
    gwork = torch.empty(ivf_group_bytes(bank, len(cent)), dtype=torch.uint8, device="cuda")

    def regroup():                                                     # into the same bank again: no allocation in the timing
        grouped.clear()
        _lib.check(_lib.lib().jat_bank_group(bank._h, _lib.ptr(idx), len(cent), grouped._h, _lib.ptr(offsets), _lib.ptr(order),
                                             _lib.ptr(gwork), gwork.numel(), _lib.stream_ptr()))
    t_group = statistics.median(timed(regroup, 1) for _ in range(3))
    ivf = RT.IVFBank(grouped, cent, offsets, order, 1)
    sizes = sorted(ivf.list_sizes().tolist())
    print(f"build: k-means {report['iterations']} iterations {t_km:.2f} s (wall, waits for the device every iteration), kept "
          f"{report['kept']} of {nlist} lists; assign {t_assign / 1e3:.2f} ms; group {t_group / 1e3:.2f} ms "
          f"(reading and writing the rows once at {HBM_COPY_TBS} TB/s: {2 * N * C * 2 / (HBM_COPY_TBS * 1e12) * 1e3:.2f} ms); "
          f"lists of {sizes[0]} / {sizes[len(sizes) // 2]} / {sizes[-1]} rows (min / median / max)", flush=True)
    del bank
    torch.cuda.empty_cache()
    lsize = ivf.list_sizes().cuda()

    # (b) speed
    for nq in a.frames:
        x = q[:nq].t()[None].contiguous()
        fns = {"flat k=1": (lambda: grouped.search_topk(x, 1)), "flat k=8": (lambda: grouped.search_topk(x, 8))}
        for nprobe in (1, 8):
            fns[f"coarse nprobe={nprobe}"] = (lambda p=nprobe: cent.search_topk(x, p))
            for k in (1, 8):
                fns[f"ivf nprobe={nprobe} k={k}"] = (lambda p=nprobe, kk=k: ivf.search_topk(x, kk, nprobe=p))
        for f in fns.values():
            f()
        torch.cuda.synchronize()
        t = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, f in fns.items():
                t[k].append(timed(f, a.reps))
        m = {k: statistics.median(v) for k, v in t.items()}
        print(f"{nq} queries:")
        for k in fns:
            print(f"  {k:22s} {m[k] / 1e3:9.3f} ms [{min(t[k]) / 1e3:.3f}..{max(t[k]) / 1e3:.3f}]", flush=True)
        for nprobe in (1, 8):
            pr = ivf.search_topk(x, 1, nprobe=nprobe, probes=True)[2].long().clamp_min(0)
            rows = int(lsize[pr.flatten()].sum())
            bound = rows * C * 2 / (HBM_COPY_TBS * 1e12) * 1e6
            for k in (1, 8):
                scan = m[f"ivf nprobe={nprobe} k={k}"] - m[f"coarse nprobe={nprobe}"]
                print(f"  nprobe={nprobe} k={k}: planes + scan {scan / 1e3:.3f} ms (total - coarse) for {rows} probed rows = "
                      f"{rows * C * 2 / 2 ** 20:.0f} MiB, byte bound {bound / 1e3:.3f} ms (x{scan / bound:.1f}); flat / ivf x"
                      f"{m[f'flat k={k}'] / m[f'ivf nprobe={nprobe} k={k}']:.1f}", flush=True)

    # (c) recall
    x = q.t()[None].contiguous()
    f1, _ = grouped.search_topk(x, 1)
    f8, _ = grouped.search_topk(x, 8)
    for nprobe in (1, 2, 4, 8):
        i1, _ = ivf.search_topk(x, 1, nprobe=nprobe)
        i8, _ = ivf.search_topk(x, 8, nprobe=nprobe)
        hit = float((i1 == f1).float().mean())
        overlap = float((i8[0, :, :, None] == f8[0, :, None, :]).any(-1).float().mean())
        print(f"recall, {held} held-out queries, nprobe={nprobe}: flat nearest row returned for {100 * hit:.2f} %, mean overlap of "
              f"the k = 8 lists {100 * overlap:.2f} %", flush=True)


if __name__ == "__main__":
    main()
