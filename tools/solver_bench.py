#!/usr/bin/env python3
"""Euler-50 against midpoint-25 at the flagship shape, in one process:
    python tools/solver_bench.py [--B 28] [--T 512] [--repeats 7] [--runs 3] [--warmup 2]

Both make 50 model evaluations (CFG double batch each).  The two captured samplers live side by side on one model and are timed
the way bench.py times the sampler (graph replays between two synchronisations, wall clock), `--runs` replays per figure,
interleaved: euler, midpoint, euler, midpoint, ... so that clock and temperature drift reaches both alike.  Prints one JSON line:
the medians over `--repeats`, the max - min spread of the Euler figures, and whether
    median(midpoint-25) <= median(euler-50) * 1.005 + spread(euler-50)
holds: the stages read or write one more fp32 plane per evaluation than the Euler tail, nothing else differs.
It times the integration rule's cost, not its quality.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="v3mod2")
    ap.add_argument("--B", type=int, default=28)
    ap.add_argument("--T", type=int, default=512)
    ap.add_argument("--cfg-scale", type=float, default=3.0)
    ap.add_argument("--euler-steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--runs", type=int, default=3, help="graph replays per timed figure")
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if a.euler_steps % 2:
        ap.error("--euler-steps must be even: midpoint takes half as many steps")
    import torch
    import jatsr_amd
    import jatsr_amd.recipe as recipe
    cfg = recipe.CONFIGS[a.config]
    C = cfg["input_channels"]
    model = jatsr_amd.JaT_AudioSR_V3(**cfg)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in recipe.make_state_dict(cfg).items()}, strict=False)
    model = model.cuda().eval()
    lr = torch.from_numpy(recipe.gaussian("lr_latent", (a.B, C, a.T), 1234)).cuda()
    z0 = torch.from_numpy(recipe.gaussian("z0", (a.B, C, a.T), 1235)).cuda()
    samplers = {"euler": jatsr_amd.Sampler(model, a.B, a.T, a.euler_steps, a.cfg_scale),
                "midpoint": jatsr_amd.Sampler(model, a.B, a.T, a.euler_steps // 2, a.cfg_scale, solver="midpoint")}
    evals = {k: s.evaluations() for k, s in samplers.items()}
    assert evals["euler"] == evals["midpoint"] == a.euler_steps, evals
    for s in samplers.values():
        for _ in range(a.warmup):
            out = s.run(lr, z0)
    torch.cuda.synchronize()
    ms = {k: [] for k in samplers}
    for _ in range(a.repeats):
        for k, s in samplers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.runs):
                out = s.run(lr, z0)
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) / a.runs * 1e3)
            assert bool(torch.isfinite(out).all())
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = max(ms["euler"]) - min(ms["euler"])
    limit = med["euler"] * 1.005 + spread
    print(json.dumps({"workload": f"{a.config} B={a.B} T={a.T} CFG={a.cfg_scale}, {a.euler_steps} evaluations per run",
                      "euler_ms": med["euler"], "midpoint_ms": med["midpoint"], "euler_spread_ms": spread,
                      "midpoint_spread_ms": max(ms["midpoint"]) - min(ms["midpoint"]), "ratio": med["midpoint"] / med["euler"],
                      "limit_ms": limit, "within_limit": med["midpoint"] <= limit, "repeats": a.repeats, "runs": a.runs,
                      "info": {k: s.info() | {"tail_fused": s.tail_fused()} for k, s in samplers.items()},
                      "euler_all_ms": ms["euler"], "midpoint_all_ms": ms["midpoint"]}))


if __name__ == "__main__":
    main()
