#!/usr/bin/env python3
"""Time the IIR low-pass (csrc/iir.hip) with HIP events on one stream after warm-up:
    python tools/lowpass_bench.py [--kind cheby1] [--order 10] [--cutoff-hz 4000] [--reps 20] [--rounds 11]
`sosfiltfilt` at 8 x 384 000 samples (the batch `prepare` filters) and 1 x 2 285 568 (a 47.6 s recording), against
(a) its byte bound: the six launches read the row four times and write it twice (forward A: x; forward C: x -> the filtered
    extension; backward A: the extension; backward C: the extension -> y), 6 B n 4 bytes plus 66 samples of extension per pass and
    160 bytes of tile states per tile and direction, at the 6.29 TB/s copy rate DESIGN uses, and at the rate a device-to-device
    copy of as many bytes reaches in this process;
(b) scipy.signal.sosfiltfilt on the host in fp64, both copies included, where scipy imports;
(c) a torch composition on the same GPU, rfft -> multiply by |H|^2 -> irfft: circular edges in the place of the odd extension, a
    timing comparator only.
With --prepare S also prepare_audio of an S-second 44.1 kHz file (recipe DAC weights), the default round trip and --lr-filter
alternating, host clock around a device synchronise.
The variants alternate in rounds within one process; the median round counts and the range of the rounds is printed."""
import argparse
import hashlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from retrieval_bench import timed  # noqa: E402

COPY_RATE = 6.29e12       # bytes / s, DESIGN's device-copy rate


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", default="cheby1")
    ap.add_argument("--order", type=int, default=10)
    ap.add_argument("--cutoff-hz", type=float, default=4000.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--host-rounds", type=int, default=3)
    ap.add_argument("--prepare", type=float, default=0.0, help="also time prepare_audio of a file of this many seconds")
    a = ap.parse_args()
    import numpy as np
    import torch
    from jatsr_amd import _lib
    from jatsr_amd import lowpass as LP
    _lib.require_gpu()
    print(f"library {os.path.basename(_lib.LIB_PATH)} sha256 {hashlib.sha256(open(_lib.LIB_PATH, 'rb').read()).hexdigest()[:16]}")
    sos = LP.design_sos(a.kind, a.order, a.cutoff_hz, 48000)
    bank = LP.LowpassBank([sos])
    try:
        import scipy.signal as ss
    except Exception:
        ss = None
        print("scipy does not import here: no host comparison")
    g = torch.Generator(device="cuda").manual_seed(0)
    for B, n in ((8, 384_000), (1, 2_285_568)):
        x = torch.randn(B, n, device="cuda", generator=g)
        y = torch.empty_like(x)
        rows = bank.rows(None, B)
        nbytes = LP.workspace_bytes(B, n)
        work = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        fn, stream = _lib.lib().jat_iir_sosfiltfilt, _lib.stream_ptr()
        w = np.fft.rfftfreq(n) * 2 * np.pi
        z = np.exp(-1j * w)
        H = np.prod([(s[0] + s[1] * z + s[2] * z * z) / (1 + s[4] * z + s[5] * z * z) for s in sos], axis=0)
        H2 = torch.from_numpy((np.abs(H) ** 2).astype(np.float32)).cuda()
        tiles = -(-(n + 66) // LP.TILE)
        moved = B * (4 * (4 * (n + 66) + 2 * n) + 2 * 160 * tiles)
        src, dst = torch.empty(moved // 8, device="cuda"), torch.empty(moved // 8, device="cuda")   # a copy moving as many bytes
        fns = {"sosfiltfilt (launches only)": lambda: fn(bank.ptr, _lib.ptr(rows), _lib.ptr(x), _lib.ptr(y), B, n, _lib.ptr(work), nbytes, stream),
               "sosfiltfilt (Python call)": lambda: LP.sosfiltfilt(x, bank, out=y),
               "sosfilt (one direction, launches only)": lambda: _lib.lib().jat_iir_sosfilt(bank.ptr, _lib.ptr(rows), _lib.ptr(x), _lib.ptr(y),
                                                                                         B, n, _lib.ptr(work), nbytes, stream),
               "rfft * |H|^2 irfft (torch)": lambda: torch.fft.irfft(torch.fft.rfft(x) * H2, n=n),
               "device copy of as many bytes": lambda: dst.copy_(src)}
        for f in fns.values():
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        t = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, f in fns.items():
                t[k].append(timed(f, a.reps))
        m = {k: statistics.median(v) for k, v in t.items()}
        print(f"{B} x {n} samples, {a.kind} order {a.order} at {a.cutoff_hz:g} Hz, {tiles} tiles a row:")
        for k in fns:
            print(f"  {k:40s} {m[k]:10.1f} us [{min(t[k]):.1f}..{max(t[k]):.1f}]", flush=True)
        ff = m["sosfiltfilt (launches only)"]
        print(f"  bytes moved by the six launches: {moved / 1e6:.1f} MB = {moved / COPY_RATE * 1e6:.1f} us at 6.29 TB/s: sosfiltfilt / byte "
              f"bound x{ff / (moved / COPY_RATE * 1e6):.2f}; / the measured copy x{ff / m['device copy of as many bytes']:.2f}; "
              f"torch fft / sosfiltfilt x{m['rfft * |H|^2 irfft (torch)'] / ff:.2f}")
        if ss is not None:
            host = []
            for _ in range(a.host_rounds):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = torch.from_numpy(ss.sosfiltfilt(sos, x.cpu().numpy().astype(np.float64), axis=-1).astype(np.float32)).cuda()
                torch.cuda.synchronize()
                host.append((time.perf_counter() - t0) * 1e6)
            err = float((out - LP.sosfiltfilt(x, bank)).norm() / out.norm())
            print(f"  scipy.signal.sosfiltfilt on the host (fp64, both copies): {statistics.median(host) / 1e3:.1f} ms "
                  f"[{min(host) / 1e3:.1f}..{max(host) / 1e3:.1f}] = x{statistics.median(host) / ff:.0f}; GPU against it rel-L2 {err:.2e}",
                  flush=True)
    if a.prepare > 0:
        prepare_both(a.prepare, {"kind": a.kind, "order": a.order, "cutoff_hz": a.cutoff_hz}, a.rounds)


def prepare_both(seconds, filt, rounds):
    import numpy as np
    import torch
    import jatsr_amd.dac as D
    import jatsr_amd.prepare as P
    import jatsr_amd.recipe as recipe
    enc = D.DacEncoder()
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in recipe.make_dac_encoder_state_dict().items()})
    codec = D.DacCodec(D.DacDecoder(), enc.cuda())
    audio = torch.from_numpy((0.1 * np.random.default_rng(0).standard_normal(int(seconds * 44100))).astype(np.float32)).cuda()
    kws = {"default (sinc round trip)": {}, f"lr_filter {filt['kind']} {filt['order']}": {"lr_filter": filt}}
    t = {k: [] for k in kws}
    split = {k: {} for k in kws}
    for k, kw in kws.items():
        P.prepare_audio(audio, 44100, codec, **kw)
    for _ in range(rounds):
        for k, kw in kws.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = P.prepare_audio(audio, 44100, codec, timings=split[k], **kw)
            torch.cuda.synchronize()
            t[k].append((time.perf_counter() - t0) * 1e3)
    for k in kws:
        print(f"prepare_audio of {seconds:.0f} s at 44.1 kHz -> {out['hr_latent'].shape[-1]} frames, {k}: {statistics.median(t[k]):.2f} ms "
              f"[{min(t[k]):.2f}..{max(t[k]):.2f}]; stages " + ", ".join(f"{s} {v / rounds:.2f} ms" for s, v in split[k].items()), flush=True)


if __name__ == "__main__":
    main()
