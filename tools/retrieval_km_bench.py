#!/usr/bin/env python3
"""Time k-means compaction of a retrieval bank (csrc/retrieval_km.hip) with HIP events on one stream after warm-up:
    python tools/retrieval_km_bench.py [--pool 1000000 200000] [--clusters 10000] [--channels 1024] [--reps 2] [--rounds 5]
per pool size, K centroids seeded from pool rows i N // K:
(a) one `assign`, one `cluster_update`, and one full iteration (assign, inertia, update; nothing waits for the device);
(b) the same iteration composed from what existed before on the same GPU: the pool rows to fp32 [1, C, n] by torch in chunks,
    `LatentBank.search` per chunk, `index_add_` of the rows into fp32 sums, a divide, the rows loaded into a bank;
(c) what the design expected: the assignment at about half the search's time per (row, centroid) pair (one MFMA pass instead of
    two), the update near the time to read the pool once at the measured copy rate;
(d) on synthetic latents only (an uneven mixture: dense and sparse regions), the mean dist2 from a held-out row to its nearest
    bank row for a clustered bank against a strided bank of the same size.  No audio, no trained weights.
The variants alternate in rounds within one process; the median round counts and the range of the rounds is printed.  Temporary
bytes: the allocator's peak over one call."""
import argparse
import hashlib
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from retrieval_bench import peak_temp_bytes, timed  # noqa: E402

HBM_COPY_TBS = 6.29          # measured float4 copy rate of the MI355X (8.0 TB/s by specification)
CHUNK = 65536                # pool rows per search of the composed iteration


def sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pool", type=int, nargs="+", default=[1_000_000, 200_000])
    ap.add_argument("--clusters", type=int, default=10_000)
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quality-pool", type=int, default=200_000, help="pool rows of the synthetic-latent figure (0: skip)")
    a = ap.parse_args()
    import torch
    from jatsr_amd import _lib
    from jatsr_amd import retrieval as RT
    _lib.require_gpu()
    csrc = os.path.join(os.path.dirname(_lib.LIB_PATH))
    print(f"library {os.path.basename(_lib.LIB_PATH)} sha256 {sha(_lib.LIB_PATH)}; retrieval.hip sha256 "
          f"{sha(os.path.join(csrc, 'retrieval.hip'))} (untouched: the search is the one measured before)")
    K, C = a.clusters, a.channels
    g = torch.Generator(device="cuda").manual_seed(0)
    for N in a.pool:
        pool = RT.LatentBank(C, N)
        for lo in range(0, N, 1 << 18):
            pool.load_rows(torch.randn(min(1 << 18, N - lo), C, device="cuda", generator=g).half())
        rows16 = pool.rows("keys")[0]
        seeds = torch.tensor(RT.seed_positions(N, K), device="cuda")
        cent, other = RT.LatentBank(C, K), RT.LatentBank(C, K)
        cent.load_rows(rows16[seeds])
        idx = torch.full((N,), -1, dtype=torch.int32, device="cuda")
        changed = torch.zeros(1, dtype=torch.int32, device="cuda")
        cent.assign(pool, idx=idx)
        print(f"pool {N} x {C} fp16 = {N * C * 2 / 2 ** 20:.0f} MiB, {K} centroids = {K * C * 2 / 2 ** 20:.0f} MiB")

        def ours_iter():
            _, d = cent.assign(pool, idx=idx, changed=changed)
            RT.sum_dist2(d)
            return cent.cluster_update(pool, idx, check=False)

        def torch_iter():
            sums = torch.zeros(K, C, device="cuda")
            cnt = torch.zeros(K, device="cuda")
            for lo in range(0, N, CHUNK):
                rows = rows16[lo:lo + CHUNK]
                f = rows.float()
                i, _ = cent.search(f.T.contiguous()[None])
                i = i[0].long()
                sums.index_add_(0, i, f)
                cnt.index_add_(0, i, torch.ones_like(i, dtype=torch.float32))
            new = torch.where(cnt[:, None] > 0, sums / cnt.clamp_min(1)[:, None], cent.rows("keys")[0].float()).half()
            other.clear()
            other.load_rows(new)
            return new

        def search_only():
            for lo in range(0, N, CHUNK):
                cent.search(rows16[lo:lo + CHUNK].float().T.contiguous()[None])

        fns = {"assign": lambda: cent.assign(pool, idx=idx, changed=changed),
               "cluster_update": lambda: cent.cluster_update(pool, idx, check=False),
               "iteration (assign, inertia, update)": ours_iter,
               "composed: convert + search": search_only,
               "composed iteration (torch + search + index_add_)": torch_iter}
        temp = {k: peak_temp_bytes(f) for k, f in fns.items()}
        cent.clear()
        cent.load_rows(rows16[seeds])                                   # every variant times the same first iterations
        for f in fns.values():
            f()
        torch.cuda.synchronize()
        t = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, f in fns.items():
                t[k].append(timed(f, a.reps))
        m = {k: statistics.median(v) for k, v in t.items()}
        for k in fns:
            print(f"  {k:50s} {m[k] / 1e3:10.2f} ms [{min(t[k]) / 1e3:.2f}..{max(t[k]) / 1e3:.2f}] | allocator peak over one call "
                  f"{temp[k] / 2 ** 20:8.1f} MiB", flush=True)
        pairs = N * K
        read_ms = N * C * 2 / (HBM_COPY_TBS * 1e12) * 1e3
        print(f"  assign: {m['assign'] * 1e6 / pairs:.2f} ps per (row, centroid) pair, {2 * pairs * C / (m['assign'] * 1e-6) / 1e12:.0f} "
              f"TFLOP/s; convert + search: {m['composed: convert + search'] * 1e6 / pairs:.2f} ps per pair; ratio "
              f"{m['assign'] / m['composed: convert + search']:.2f} (expected about 0.5)")
        print(f"  cluster_update: {m['cluster_update'] / 1e3:.2f} ms against {read_ms:.2f} ms to read the pool once at {HBM_COPY_TBS} TB/s "
              f"(x{m['cluster_update'] / 1e3 / read_ms:.1f}); composed / ours per iteration x"
              f"{m['composed iteration (torch + search + index_add_)'] / m['iteration (assign, inertia, update)']:.2f}", flush=True)
        del pool, cent, other, rows16, idx
        torch.cuda.empty_cache()
    if a.quality_pool:
        N, held, centres = a.quality_pool, 20_000, 2000
        mu = torch.randn(centres, C, device="cuda", generator=g) * 1.5
        w = torch.rand(centres, device="cuda", generator=g) ** 4         # a few heavy components, many light ones
        pick = torch.multinomial(w, N + held, replacement=True, generator=g)
        data = (mu[pick] + torch.randn(N + held, C, device="cuda", generator=g) * 0.5).half()
        pool, test = RT.LatentBank(C, N), RT.LatentBank(C, held)
        pool.load_rows(data[:N])
        test.load_rows(data[N:])
        Kq = min(K, held)
        km, report = RT.kmeans(pool, Kq, iters=10)
        strided = RT.LatentBank(C, len(km))
        strided.load_rows(data[:N][torch.tensor(RT.seed_positions(N, len(km)), device="cuda")])
        dk = float(RT.sum_dist2(km.assign(test)[1])) / held
        ds = float(RT.sum_dist2(strided.assign(test)[1])) / held
        print(f"synthetic latents ({centres} uneven components, {N} pool rows, {held} held out, C = {C}): mean dist2 to the nearest "
              f"of {len(km)} rows: clustered {dk:.2f}, strided {ds:.2f} (x{ds / dk:.2f}); k-means ran {report['iterations']} "
              f"iterations, inertia {report['inertia'][0]:.4g} -> {report['inertia'][-1]:.4g}, kept {report['kept']} of {Kq}, "
              f"sizes {report['size_min']} / {report['size_median']} / {report['size_max']}")


if __name__ == "__main__":
    main()
