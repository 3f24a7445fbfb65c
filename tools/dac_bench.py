#!/usr/bin/env python3
"""Time jat_dac_decode (DAC 44.1 kHz decoder, csrc/dac.hip) with HIP events after warm-up, recipe weights:
    python tools/dac_bench.py [--T 1378 4096] [--B 1] [--reps 5] [--precision bf16x3 bf16]
Prints ms, TFLOP/s (1.608 GFLOP x T x passes: bf16x3 runs three MFMA passes) and the fraction of 2.5 PFLOP/s."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, nargs="+", default=[1378, 4096])
    ap.add_argument("--B", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--precision", nargs="+", default=["bf16x3", "bf16"])
    a = ap.parse_args()
    import torch
    import jatsr_amd.dac as D
    import jatsr_amd.recipe as recipe
    m = D.DacDecoder(max_B=a.B, max_T=max(a.T))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in recipe.make_dac_state_dict().items()})
    m = m.cuda()
    for T in a.T:
        z = torch.from_numpy(recipe.gaussian("dac_bench", (a.B, 1024, T), 5)).cuda()
        for prec in a.precision:
            m(z, precision=prec)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                m(z, precision=prec)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / a.reps
            passes = 3 if prec == "bf16x3" else 1
            tf = recipe.dac_flops(T, a.B) * passes / (ms * 1e-3) / 1e12
            print(f"B={a.B} T={T} ({T * 512 / 44100:.1f} s audio) {prec:6s}: {ms:8.2f} ms  {tf:6.1f} TFLOP/s "
                  f"({passes} pass{'es' if passes > 1 else ''})  {tf / 2500:.1%} of 2.5 PF", flush=True)


if __name__ == "__main__":
    main()
