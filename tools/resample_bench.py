#!/usr/bin/env python3
"""Time the sample-rate converter (csrc/resample.hip) with HIP events on one stream after warm-up:
    python tools/resample_bench.py [--seconds 47.6 16] [--reps 200] [--prepare 60]
(a) jat_resample for 16k -> 44.1k, 44.1k -> 48k, 48k -> 16k, 16k -> 48k and 48k -> 44.1k (width 24, rolloff 0.945);
(b) the same algorithm as torchaudio runs it on a GPU: zero-pad, one torch.nn.functional.conv1d with the same table and
    stride, transpose to sample order (`conv1d` alone is printed too); (a) and (b) alternate in rounds, the median round counts;
(c) with --prepare S: jatsr_amd.prepare.prepare_audio of an S-second 44.1 kHz file with recipe DAC weights, split into
    resample / encode / statistics time.
Prints the worst |a - b| of each conversion as well.  For a kernel table run it on its own under
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- python tools/resample_bench.py --reps 20"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONVERSIONS = [(16000, 44100, 6, 0.99), (44100, 48000, 6, 0.99), (48000, 16000, 6, 0.99), (16000, 48000, 6, 0.99),
               (48000, 44100, 24, 0.945)]


def timed(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3      # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, nargs="+", default=[4096 * 512 / 44100, 16.0])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--prepare", type=float, default=0.0, help="also time prepare_audio of a file of this many seconds")
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from jatsr_amd import _lib
    from jatsr_amd.resample import resample, sinc_table
    _lib.require_gpu()
    import hashlib
    print(f"library {os.path.basename(_lib.LIB_PATH)} sha256 {hashlib.sha256(open(_lib.LIB_PATH, 'rb').read()).hexdigest()[:16]}")
    g = torch.Generator().manual_seed(0)
    for seconds in a.seconds:
        for orig, new, lpw, roll in CONVERSIONS:
            n_in = int(round(seconds * orig))
            x = (0.1 * torch.randn(1, n_in, generator=g)).cuda()
            h, o, n, width, K = sinc_table(orig, new, lpw, roll)
            w = torch.from_numpy(h).cuda()[:, None, :]
            n_out = -(-n * n_in // o)

            def ours():
                return resample(x, orig, new, lpw, roll)

            def conv_only(xp=F.pad(x, (width, width + o))[:, None]):
                return F.conv1d(xp, w, stride=o)

            def as_torchaudio():
                y = F.conv1d(F.pad(x, (width, width + o))[:, None], w, stride=o)
                return y.transpose(1, 2).reshape(1, -1)[..., :n_out].contiguous()

            err = float((ours() - as_torchaudio()).abs().max())
            for fn in (ours, conv_only, as_torchaudio):          # warm-up: code objects, algorithm search
                for _ in range(5):
                    fn()
            torch.cuda.synchronize()
            t = {"ours": [], "conv": [], "ta": []}
            for _ in range(a.rounds):
                t["ours"].append(timed(ours, a.reps))
                t["conv"].append(timed(conv_only, a.reps))
                t["ta"].append(timed(as_torchaudio, a.reps))
            m = {k: statistics.median(v) for k, v in t.items()}
            gflop = 2.0 * n_out * K / 1e9
            print(f"{seconds:5.1f} s {orig:6d} -> {new:6d} (o {o:3d} n {n:3d} K {K:3d}): jat_resample {m['ours']:8.1f} us "
                  f"[{min(t['ours']):.1f}..{max(t['ours']):.1f}] ({gflop / m['ours'] * 1e3:6.2f} TFLOP/s) | conv1d alone "
                  f"{m['conv']:8.1f} us | pad + conv1d + transpose {m['ta']:8.1f} us | x{m['conv'] / m['ours']:.2f} / "
                  f"x{m['ta'] / m['ours']:.2f} | max |diff| {err:.2e}", flush=True)
    if a.prepare > 0:
        prepare_split(a.prepare, a.reps)


def prepare_split(seconds, reps):
    import numpy as np
    import torch
    import jatsr_amd.dac as D
    import jatsr_amd.prepare as P
    import jatsr_amd.recipe as recipe
    enc = D.DacEncoder()
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in recipe.make_dac_encoder_state_dict().items()})
    codec = D.DacCodec(D.DacDecoder(), enc.cuda())
    rng = np.random.default_rng(0)
    audio = torch.from_numpy((0.1 * rng.standard_normal(int(seconds * 44100))).astype(np.float32)).cuda()
    P.prepare_audio(audio, 44100, codec)
    torch.cuda.synchronize()
    times = {}
    for _ in range(3):
        out = P.prepare_audio(audio, 44100, codec, timings=times)
    n = 3
    total = sum(times.values())
    print(f"prepare_audio of {seconds:.0f} s at 44.1 kHz -> {out['hr_latent'].shape[-1]} frames: "
          + ", ".join(f"{k} {v / n:.2f} ms ({100 * v / total:.1f} %)" for k, v in times.items())
          + f", sum {total / n:.2f} ms", flush=True)


if __name__ == "__main__":
    main()
