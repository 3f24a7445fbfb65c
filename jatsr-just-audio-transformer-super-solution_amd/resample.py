"""Sample-rate conversion on the GPU — `torchaudio.functional.resample` (`sinc_interp_hann`), which the reference's data
preparation calls (`AF.resample`, prepare_dataset_v5.py:198,203), computed by csrc/resample.hip behind `jat_resample`;
and the per-channel fp64 sums of fp16-rounded latents (prepare_dataset_v5.py:251-253) behind `jat_channel_stats`.

    y = jatsr_amd.resample(x, 16000, 44100)          # x fp32 [..., L] on the GPU -> [..., ceil(441 L / 160)]
    lr = jatsr_amd.simulate_lr(hr)                   # 48 -> 16 -> 48 kHz, padded back to hr's length

There is no CPU path: a CPU tensor raises.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L

# the 48 -> 44.1 kHz step before the DAC encode: the reference goes through audiotools' AudioSignal.resample (julius,
# zeros = 24, rolloff = 0.945); here the same windowed-sinc kernel with those two parameters
CODEC_LOWPASS_WIDTH, CODEC_ROLLOFF = 24, 0.945

STATS_SLICES = 16     # JAT_STATS_SLICES of include/jat_hip.h

_handles: dict = {}


class _Resampler:
    def __init__(self, orig, new, lpw, rolloff, device):
        self.ptr = C.c_void_p()
        self.device = device
        with torch.cuda.device(device):
            L.check(L.lib().jat_resampler_create(orig, new, lpw, rolloff, L.stream_ptr(), C.byref(self.ptr)))
        g = math.gcd(orig, new)
        self.o, self.n = orig // g, new // g

    def __del__(self):
        try:
            if self.ptr:
                L.lib().jat_resampler_destroy(self.ptr)
        except Exception:
            pass

    def out_length(self, n: int) -> int:
        if n < (1 << 30) // max(1, self.n // self.o + 1):          # far from the 31-bit limits: no call needed
            return -(-n * self.n // self.o)
        out = C.c_int64()
        L.check(L.lib().jat_resample_out_length(self.ptr, n, C.byref(out)))
        return out.value


def _check_args(orig_freq, new_freq, lowpass_filter_width, rolloff):
    for name, v in (("orig_freq", orig_freq), ("new_freq", new_freq)):
        if int(v) != v or v <= 0:
            raise ValueError(f"resample: {name} must be a positive integer, got {v!r}")
    if int(lowpass_filter_width) != lowpass_filter_width or lowpass_filter_width < 1:
        raise ValueError(f"resample: lowpass_filter_width must be an integer >= 1, got {lowpass_filter_width!r}")
    if not 0.0 < rolloff <= 1.0:
        raise ValueError(f"resample: rolloff must be in (0, 1], got {rolloff!r}")


def sinc_table(orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99):
    """-> (h fp32 numpy [n, K], o, n, width, K): the tap table `jat_resample_table` computes in fp64 on the host (no GPU)."""
    _check_args(orig_freq, new_freq, lowpass_filter_width, rolloff)
    dims = [C.c_int32() for _ in range(4)]
    args = (int(orig_freq), int(new_freq), int(lowpass_filter_width), float(rolloff))
    L.check(L.lib().jat_resample_table(*args, None, *(C.byref(d) for d in dims)))
    o, n, width, K = (d.value for d in dims)
    h = np.empty((n, K), np.float32)
    L.check(L.lib().jat_resample_table(*args, h.ctypes.data, *(C.byref(d) for d in dims)))
    return h, o, n, width, K


def _handle(orig, new, lpw, rolloff, device) -> _Resampler:
    key = (orig, new, lpw, rolloff, device)
    h = _handles.get(key)
    if h is None:
        h = _handles[key] = _Resampler(orig, new, lpw, rolloff, device)
    return h


@torch.no_grad()
def resample(waveform: torch.Tensor, orig_freq: int, new_freq: int, lowpass_filter_width: int = 6,
             rolloff: float = 0.99) -> torch.Tensor:
    """torchaudio's `functional.resample(waveform, orig_freq, new_freq, lowpass_filter_width, rolloff)` with the Hann
    window: fp32 CUDA [..., L] -> [..., ceil(new L / orig)].  `orig_freq == new_freq` returns a copy."""
    _check_args(orig_freq, new_freq, lowpass_filter_width, rolloff)
    if not isinstance(waveform, torch.Tensor) or waveform.dim() < 1:
        raise L.JatError("resample: the waveform must be a tensor [..., L]")
    if not waveform.is_cuda:
        raise L.JatError("resample: the waveform must be a CUDA tensor (there is no CPU path)")
    if waveform.dtype != torch.float32:
        raise L.JatError(f"resample: the waveform must be float32, got {waveform.dtype}")
    x = waveform.detach().contiguous()
    n = x.shape[-1]
    B = x.numel() // n if n else 0
    h = _handle(int(orig_freq), int(new_freq), int(lowpass_filter_width), float(rolloff), x.device)
    n_out = h.out_length(n)
    y = torch.empty(x.shape[:-1] + (n_out,), dtype=torch.float32, device=x.device)
    fn, yp, xp = L.lib().jat_resample, y.data_ptr(), x.data_ptr()
    with _on(x.device):
        stream = L.stream_ptr()
        for b0 in range(0, B, 65535):          # rows per launch: one grid dimension
            L.check(fn(h.ptr, C.c_void_p(xp + 4 * b0 * n), C.c_void_p(yp + 4 * b0 * n_out), min(B - b0, 65535), n, stream))
    return y


_HERE = contextlib.nullcontext()


def _on(device):
    """the device guard, skipped when `device` is the current one already (the common case; the guard costs microseconds)"""
    return _HERE if device.index == torch.cuda.current_device() else torch.cuda.device(device)


def simulate_lr(hr: torch.Tensor, high_sr: int = 48000, low_sr: int = 16000) -> torch.Tensor:
    """The reference's low-resolution simulation (prepare_dataset_v5.py:203-205): down to `low_sr` and back, then brought
    to the input's length on the right — zero-padded where the round trip came out shorter, cut where it came out longer
    (the reference's `F.pad` with a negative amount cuts)."""
    lr = resample(resample(hr, high_sr, low_sr), low_sr, high_sr)
    n = hr.shape[-1]
    if lr.shape[-1] < n:
        lr = torch.nn.functional.pad(lr, (0, n - lr.shape[-1]))
    elif lr.shape[-1] > n:
        lr = lr[..., :n].contiguous()
    return lr


@torch.no_grad()
def channel_stats(z: torch.Tensor, sum: torch.Tensor | None = None, sq_sum: torch.Tensor | None = None):
    """Per-channel sum and sum of squares of `z` rounded to fp16, in fp64 (`jat_channel_stats`): z fp32 CUDA [B, C, T] or
    [C, T] -> (sum [C], sq_sum [C]) fp64 on the device.  Given `sum` / `sq_sum` are added to in place (running totals)."""
    if z.dim() == 2:
        z = z[None]
    if z.dim() != 3 or not z.is_cuda or z.dtype != torch.float32:
        raise L.JatError(f"channel_stats: z must be a float32 CUDA tensor [B, C, T], got {z.dtype} {tuple(z.shape)}")
    B, Cc, T = z.shape
    if min(B, Cc, T) < 1:
        raise L.JatError(f"channel_stats: empty tensor {tuple(z.shape)}")
    z = z.detach().contiguous()
    if sum is None:
        sum = torch.zeros(Cc, dtype=torch.float64, device=z.device)
    if sq_sum is None:
        sq_sum = torch.zeros(Cc, dtype=torch.float64, device=z.device)
    for name, t in (("sum", sum), ("sq_sum", sq_sum)):
        if t.dtype != torch.float64 or t.device != z.device or t.shape != (Cc,) or not t.is_contiguous():
            raise L.JatError(f"channel_stats: {name} must be a contiguous float64 [{Cc}] tensor on {z.device}")
    work = torch.empty(Cc * STATS_SLICES * 2, dtype=torch.float64, device=z.device)
    with torch.cuda.device(z.device):
        L.check(L.lib().jat_channel_stats(L.ptr(z), B, Cc, T, L.ptr(sum), L.ptr(sq_sum), L.ptr(work), work.numel() * 8,
                                          L.stream_ptr()))
    return sum, sq_sum


def out_length(n: int, orig_freq: int, new_freq: int) -> int:
    """ceil(new n / orig) with the rates reduced by their gcd."""
    g = math.gcd(int(orig_freq), int(new_freq))
    return -(-n * (int(new_freq) // g) // (int(orig_freq) // g))


class _CallableModule(type(math)):
    """`jatsr_amd.resample` names both this module and its function (torchaudio's spelling): once the module is imported
    the package attribute is the module, so calling the module resamples."""

    def __call__(self, *args, **kwargs):
        return resample(*args, **kwargs)


import sys as _sys  # noqa: E402

_sys.modules[__name__].__class__ = _CallableModule
