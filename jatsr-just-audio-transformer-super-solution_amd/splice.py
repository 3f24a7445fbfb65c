"""Inverse STFT and low-band splice on the GPU — the closing stage of audio super-resolution: keep the input's own low
band, take only the new high band from the generator, with a raised-cosine crossfade in frequency below the input's band
limit.  Computed by csrc/splice.hip behind `jat_istft`, `jat_ltas` and `jat_band_splice`; the definitions are in
include/jat_hip.h.  The conventions are those of `jatsr_amd.metrics.stft` (periodic Hann, center=True).

    y = istft(X, length)                                   # complex64 CUDA [bins, frames] or [B, bins, frames] -> fp32 [.., length]
    P = ltas(x)                                            # long-term average power spectrum, fp64 [..., bins]
    hz = detect_cutoff(x)                                  # 1 + the last bin within 60 dB of the loudest, in Hz
    a = band_gain(44100, 2048, cutoff_hz, 500.0)           # fp32 [bins] on the host: 1 = take the source
    out, hz = splice_lowband(generated, source)            # generated + iSTFT(a STFT(source - generated))

    python -m jatsr_amd.splice --generated X_generated.wav --source low.wav --out X_lf.wav [--cutoff-hz HZ] [--transition-hz HZ]

The splice is built as a correction of `generated`, so it leaves `generated` untouched wherever the gain is zero, and the
samples past the shorter of the two signals are `generated` unchanged.  hop must divide n_fft with 4 <= n_fft / hop <= 64.

There is no CPU path: a CPU tensor raises.
"""
from __future__ import annotations

import argparse
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from .metrics import _check_args, _handle, _shape, _signal
from .resample import _on


def _rows(name, x):
    x = _signal(name, x)
    if x.shape[-1] < 1 or x.numel() < 1:
        raise ValueError(f"splice: {name} must hold at least one sample")
    return x.reshape(-1, x.shape[-1]).contiguous(), x.dim() == 2


def _work(h, nbytes):
    if h.work is None or h.work.numel() < nbytes:
        h.work = torch.empty(nbytes, dtype=torch.uint8, device=h.device)
    return h.work


@torch.no_grad()
def istft(X: torch.Tensor, length: int, n_fft: int = 2048, hop_length: int = 512) -> torch.Tensor:
    """`torch.istft(X, n_fft, hop_length, window=hann, center=True, length=length)`: complex64 CUDA [bins, frames] or
    [B, bins, frames] with frames = 1 + length // hop_length -> fp32 [..., length]."""
    if not isinstance(X, torch.Tensor) or X.dim() not in (2, 3):
        raise L.JatError("istft: X must be a tensor [bins, frames] or [B, bins, frames]")
    if not X.is_cuda:
        raise L.JatError("istft: X must be a CUDA tensor (there is no CPU path)")
    if X.dtype != torch.complex64:
        raise L.JatError(f"istft: X must be complex64, got {X.dtype}")
    _check_args(44100, n_fft, hop_length, 0)
    length, n_fft, hop = int(length), int(n_fft), int(hop_length)
    batched = X.dim() == 3
    Xs = X.detach().reshape(-1, X.shape[-2], X.shape[-1]).contiguous()
    B = Xs.shape[0]
    need = C.c_size_t()
    L.check(L.lib().jat_istft_workspace_bytes(n_fft, hop, B, length, C.byref(need)))          # the argument checks
    if tuple(Xs.shape[1:]) != (1 + n_fft // 2, 1 + length // hop):
        raise ValueError(f"istft: X {tuple(X.shape)} does not hold {1 + n_fft // 2} bins x {1 + length // hop} frames")
    h = _handle(44100, n_fft, hop, 0, X.device)
    with _on(X.device):
        work = _work(h, need.value)
        y = torch.empty(B, length, dtype=torch.float32, device=X.device)
        L.check(L.lib().jat_istft(h.ptr, L.ptr(Xs), B, length, L.ptr(y), L.ptr(work), work.numel(), L.stream_ptr()))
    return _shape(y, batched)


@torch.no_grad()
def ltas(x: torch.Tensor, n_fft: int = 2048, hop_length: int = 512) -> torch.Tensor:
    """Long-term average power spectrum P[k] = mean_f |STFT(x)[k, f]|^2: fp32 CUDA [L] or [B, L] -> fp64 [..., bins]."""
    xs, batched = _rows("x", x)
    B, n = xs.shape
    h = _handle(44100, n_fft, hop_length, 0, x.device)
    with _on(x.device):
        work = _work(h, B * L.LTAS_SLICES * h.bins * 8)
        P = torch.empty(B, h.bins, dtype=torch.float64, device=x.device)
        L.check(L.lib().jat_ltas(h.ptr, L.ptr(xs), B, n, L.ptr(P), L.ptr(work), work.numel(), L.stream_ptr()))
    return _shape(P, batched)


def cutoff_bin(P, threshold_db: float = 60.0) -> int:
    """P fp64 [bins] on the host -> 1 + the last bin at or above max(P) 10^(-threshold_db / 10); 0 for silence"""
    P = np.asarray(P, np.float64)
    top = P.max()
    if not top > 0:
        return 0
    return 1 + int(np.nonzero(P >= top * 10.0 ** (-float(threshold_db) / 10.0))[0].max())


@torch.no_grad()
def detect_cutoff(x: torch.Tensor, sr: int = 44100, threshold_db: float = 60.0, n_fft: int = 2048, hop_length: int = 512):
    """The band limit of x in Hz: (1 + the last bin whose long-term power is within `threshold_db` of the loudest bin)
    sr / n_fft; 0.0 for silence.  A float, or a list of floats for [B, L]."""
    P = ltas(x, n_fft, hop_length).cpu().numpy()
    hz = [cutoff_bin(p, threshold_db) * float(sr) / int(n_fft) for p in P.reshape(-1, P.shape[-1])]
    return hz if x.dim() == 2 else hz[0]


def band_gain(sr: int, n_fft: int, cutoff_hz: float, transition_hz: float) -> torch.Tensor:
    """The splice's gain per bin, fp32 [1 + n_fft / 2] on the host (no GPU): 1 up to cutoff_hz - transition_hz, a raised
    cosine down to 0 at cutoff_hz, 0 above."""
    _check_args(sr, n_fft, 1, 0)
    a = np.zeros(1 + max(int(n_fft), 0) // 2, np.float32)
    L.check(L.lib().jat_band_gain(int(sr), int(n_fft), float(cutoff_hz), float(transition_hz), a.ctypes.data))
    return torch.from_numpy(a)


@torch.no_grad()
def splice_gain(generated: torch.Tensor, source: torch.Tensor, gain: torch.Tensor, n_fft: int = 2048,
                hop_length: int = 512) -> torch.Tensor:
    """generated + iSTFT(gain STFT(source - generated)) on the common length, `generated` beyond it; gain fp32 [bins]
    (host or device).  fp32 CUDA [L] or [B, L]; the two signals may differ in length."""
    g, batched = _rows("generated", generated)
    s, sb = _rows("source", source)
    if sb != batched or s.shape[0] != g.shape[0] or s.device != g.device:
        raise L.JatError(f"splice: generated {tuple(generated.shape)} and source {tuple(source.shape)} must agree but "
                         "for their length")
    _check_args(44100, n_fft, hop_length, 0)
    n_fft, hop = int(n_fft), int(hop_length)
    B = g.shape[0]
    need = C.c_size_t()
    L.check(L.lib().jat_band_splice_workspace_bytes(n_fft, hop, B, g.shape[1], s.shape[1], C.byref(need)))
    if not isinstance(gain, torch.Tensor) or gain.dtype != torch.float32 or tuple(gain.shape) != (1 + n_fft // 2,):
        raise L.JatError(f"splice: gain must be a float32 tensor [{1 + n_fft // 2}]")
    h = _handle(44100, n_fft, hop, 0, g.device)
    with _on(g.device):
        a = gain.to(g.device).contiguous()
        work = _work(h, need.value)
        out = torch.empty_like(g)
        L.check(L.lib().jat_band_splice(h.ptr, L.ptr(g), L.ptr(s), B, g.shape[1], s.shape[1], L.ptr(a), L.ptr(out),
                                        L.ptr(work), work.numel(), L.stream_ptr()))
    return _shape(out, batched)


@torch.no_grad()
def splice_lowband(generated: torch.Tensor, source: torch.Tensor, cutoff_hz: float | None = None,
                   transition_hz: float = 500.0, sr: int = 44100, n_fft: int = 2048, hop_length: int = 512):
    """Replace the band of `generated` below `cutoff_hz` by that of `source` -> (out, cutoff_hz).  With cutoff_hz=None the
    cutoff is `detect_cutoff(source)`; for a batch the rows then share the lowest detected cutoff."""
    if cutoff_hz is None:
        hz = detect_cutoff(source, sr=sr, n_fft=n_fft, hop_length=hop_length)
        cutoff_hz = min(hz) if isinstance(hz, list) else hz
    cutoff_hz = float(cutoff_hz)
    return splice_gain(generated, source, band_gain(sr, n_fft, cutoff_hz, transition_hz), n_fft, hop_length), cutoff_hz


def build_parser():
    p = argparse.ArgumentParser(prog="python -m jatsr_amd.splice",
                                description="Replace the low band of a generated WAV by that of its source, on MI355X")
    p.add_argument("--generated", type=str, required=True, help="generated WAV (44.1 kHz)")
    p.add_argument("--source", type=str, required=True, help="source (input) WAV; resampled to the generated rate when needed")
    p.add_argument("--out", type=str, required=True, help="output WAV (float32)")
    p.add_argument("--cutoff-hz", type=float, default=None, help="band limit of the source; default: detected")
    p.add_argument("--transition-hz", type=float, default=500.0, help="width of the crossfade below the cutoff")
    p.add_argument("--device", type=str, default="cuda", help="Device (an AMD GPU; there is no CPU path)")
    return p


def main(argv=None):
    from . import io as jio
    from .metrics import load_audio
    args = build_parser().parse_args(argv)
    L.require_gpu()
    x, sr = jio.read_wav(args.generated)
    gen = torch.from_numpy(np.ascontiguousarray(x)).to(args.device)
    src, _ = load_audio(args.source, sr, args.device)
    out, hz = splice_lowband(gen, src, args.cutoff_hz, args.transition_hz, sr=sr)
    jio.write_wav_float32(args.out, out, sr)
    print(f"low band below {hz:.1f} Hz ({'given' if args.cutoff_hz is not None else 'detected'}) taken from "
          f"{args.source}: {min(gen.shape[-1], src.shape[-1])} of {gen.shape[-1]} samples -> {args.out}")
    return hz


if __name__ == "__main__":
    main()
