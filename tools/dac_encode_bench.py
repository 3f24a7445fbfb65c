#!/usr/bin/env python3
"""Time jat_dac_encode (DAC 44.1 kHz encoder + quantizer, csrc/dac.hip + csrc/dac_enc.hip) with HIP events after warm-up,
recipe weights and recipe audio:
    python tools/dac_encode_bench.py [--T 1378 4096] [--B 1] [--reps 5] [--precision bf16x3 bf16]
Prints ms (mean of --reps encodes), algorithmic TFLOP/s (recipe.dac_encoder_flops: 0.711 GFLOP x T) and the MFMA rate
(x 3 passes for bf16x3).  For the per-stage table run it on its own under
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- python tools/dac_encode_bench.py --T 4096 --precision bf16x3"""
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
    m = D.DacEncoder(max_B=a.B, max_T=max(a.T))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in recipe.make_dac_encoder_state_dict().items()})
    m = m.cuda()
    for T in a.T:
        audio = torch.from_numpy(recipe.make_dac_audio(a.B, T * 512, 5)).cuda()
        for prec in a.precision:
            m(audio, precision=prec)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                m(audio, precision=prec)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / a.reps
            passes = 3 if prec == "bf16x3" else 1
            tf = recipe.dac_encoder_flops(T, a.B) / (ms * 1e-3) / 1e12
            print(f"B={a.B} T={T} ({T * 512 / 44100:.1f} s audio) {prec:6s}: {ms:8.2f} ms  {tf:6.1f} TFLOP/s algorithmic "
                  f"({tf * passes:6.1f} x {passes} pass{'es' if passes > 1 else ''})", flush=True)


if __name__ == "__main__":
    main()
