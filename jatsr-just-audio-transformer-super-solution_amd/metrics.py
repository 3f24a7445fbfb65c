"""Audio-quality metrics on the GPU — what the reference's `calculate_metrics.py` computes with librosa >= 0.10: the
log-spectral distance, the mel-spectrogram L1 / L2 losses in dB (single- and multi-scale), computed by csrc/metrics.hip
behind `jat_audio_metrics_run`; the definitions are in include/jat_hip.h.

    lsd_db, lsd_frames = calculate_lsd(pred, gt)                      # fp32 CUDA [L] or [B, L]; cut to the shorter
    l1, l2, pred_db, gt_db = calculate_mel_loss(pred, gt)
    avg_l1, avg_l2, detail = calculate_multi_scale_mel_loss(pred, gt)
    report = evaluate(generated, hr_gt, lr=lr_input)                  # everything, three transforms per pair

    python -m jatsr_amd.metrics --pred X_generated.wav --gt X_hr_gt.wav --lr X_lr_input.wav --json out.json

pred and gt of a frame share one complex transform, so a bin is accurate to about 1e-7 of the frame's energy in both
signals together: a signal that is non-zero but more than about 120 dB below its partner reads as the partner's rounding
noise, and its LSD is then not what the formula gives (a frame of exact zeros is kept exact).  Decoded audio is far from that.

There is no CPU path: a CPU tensor raises.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json

import numpy as np
import torch

from . import _lib as L
from .resample import _on

SCALES = ((512, 128, 40), (1024, 256, 64), (2048, 512, 80))     # calculate_metrics.py:108-110
METRIC_KEYS = ("lsd", "mel_l1", "mel_l2", "ms_l1", "ms_l2")

_handles: dict = {}


class _Metrics:
    def __init__(self, sr, n_fft, hop, n_mels, device):
        self.ptr = C.c_void_p()
        self.device = device
        self.n_fft, self.hop, self.n_mels, self.bins = n_fft, hop, n_mels, 1 + n_fft // 2
        self.work = None
        with torch.cuda.device(device):
            L.check(L.lib().jat_audio_metrics_create(sr, n_fft, hop, n_mels, L.stream_ptr(), C.byref(self.ptr)))

    def __del__(self):
        try:
            if self.ptr:
                L.lib().jat_audio_metrics_destroy(self.ptr)
        except Exception:
            pass

    def workspace(self, B, n):
        need = C.c_size_t()
        L.check(L.lib().jat_audio_metrics_workspace_bytes(self.ptr, B, n, C.byref(need)))
        if self.work is None or self.work.numel() < need.value:
            self.work = torch.empty(need.value, dtype=torch.uint8, device=self.device)
        return self.work


def _check_args(sr, n_fft, hop, n_mels):
    for name, v in (("sr", sr), ("n_fft", n_fft), ("hop_length", hop), ("n_mels", n_mels)):
        if int(v) != v:
            raise ValueError(f"metrics: {name} must be an integer, got {v!r}")


def _handle(sr, n_fft, hop, n_mels, device) -> _Metrics:
    key = (sr, n_fft, hop, n_mels, device)
    h = _handles.get(key)
    if h is None:
        _check_args(sr, n_fft, hop, n_mels)
        h = _handles[key] = _Metrics(int(sr), int(n_fft), int(hop), int(n_mels), device)
    return h


def _signal(name, x):
    if not isinstance(x, torch.Tensor) or x.dim() not in (1, 2):
        raise L.JatError(f"metrics: {name} must be a tensor [L] or [B, L]")
    if not x.is_cuda:
        raise L.JatError(f"metrics: {name} must be a CUDA tensor (there is no CPU path)")
    if x.dtype != torch.float32:
        raise L.JatError(f"metrics: {name} must be float32, got {x.dtype}")
    return x.detach()


def _pair(pred, gt):
    """-> (pred [B, L], gt [B, L], batched): both cut to the shorter (calculate_metrics.py:39-41)"""
    pred, gt = _signal("pred", pred), _signal("gt", gt)
    if pred.dim() != gt.dim() or pred.shape[:-1] != gt.shape[:-1] or pred.device != gt.device:
        raise L.JatError(f"metrics: pred {tuple(pred.shape)} and gt {tuple(gt.shape)} must agree but for their length")
    n = min(pred.shape[-1], gt.shape[-1])
    if n < 1:
        raise ValueError("metrics: the signals must hold at least one sample")
    batched = pred.dim() == 2
    pred, gt = (v[..., :n].reshape(-1, n).contiguous() for v in (pred, gt))
    if pred.shape[0] < 1:
        raise L.JatError("metrics: empty batch")
    return pred, gt, batched


def frames_for(n: int, hop_length: int = 512) -> int:
    out = C.c_int64()
    L.check(L.lib().jat_stft_frames(int(n), int(hop_length), C.byref(out)))
    return out.value


def _run(pred, gt, sr, n_fft, hop, n_mels, want_lsd, want_db=False, out=None):
    """One STFT-and-reduce pass over rows [B, L] -> (out fp64 [B, 3] on the device, lsd_frames, pred_db, gt_db)"""
    h = _handle(sr, n_fft, hop, n_mels, pred.device)
    B, n = pred.shape
    with _on(pred.device):
        work = h.workspace(B, n)
        frames = 1 + n // h.hop
        if out is None:
            out = torch.empty(B, 3, dtype=torch.float64, device=pred.device)
        lsd_frames = torch.empty(B, frames, dtype=torch.float32, device=pred.device) if want_lsd else None
        pdb = gdb = None
        if want_db:
            pdb, gdb = (torch.empty(B, h.n_mels, frames, dtype=torch.float32, device=pred.device) for _ in range(2))
        L.check(L.lib().jat_audio_metrics_run(h.ptr, L.ptr(pred), L.ptr(gt), B, n, int(bool(want_lsd)), L.ptr(out),
                                              L.ptr(lsd_frames), L.ptr(pdb), L.ptr(gdb), L.ptr(work), work.numel(),
                                              L.stream_ptr()))
    return out, lsd_frames, pdb, gdb


def _shape(t, batched):
    return t if batched else t[0]


@torch.no_grad()
def stft(x: torch.Tensor, n_fft: int = 2048, hop_length: int = 512, y: torch.Tensor | None = None):
    """`librosa.stft(x, n_fft=n_fft, hop_length=hop_length)` (0.10 defaults): fp32 CUDA [L] or [B, L] -> complex64
    [..., 1 + n_fft / 2, 1 + L // hop].  With `y` (same shape) both signals share one complex transform per frame, as the
    metrics do, and the pair (X, Y) is returned."""
    x = _signal("x", x)
    if x.shape[-1] < 1 or x.numel() < 1:
        raise ValueError("stft: the signal must hold at least one sample")
    batched = x.dim() == 2
    xs = x.reshape(-1, x.shape[-1]).contiguous()
    ys = None
    if y is not None:
        y = _signal("y", y)
        if y.shape != x.shape or y.device != x.device:
            raise L.JatError("stft: x and y must have the same shape")
        ys = y.reshape(-1, y.shape[-1]).contiguous()
    B, n = xs.shape
    h = _handle(44100, n_fft, hop_length, 0, x.device)
    with _on(x.device):
        need = C.c_size_t()
        L.check(L.lib().jat_audio_metrics_workspace_bytes(h.ptr, B, n, C.byref(need)))      # the shape checks
        frames = 1 + n // h.hop
        X = torch.empty(B, h.bins, frames, dtype=torch.complex64, device=x.device)
        Y = torch.empty_like(X) if ys is not None else None
        L.check(L.lib().jat_stft(h.ptr, L.ptr(xs), L.ptr(ys), B, n, L.ptr(X), L.ptr(Y), L.stream_ptr()))
    return _shape(X, batched) if Y is None else (_shape(X, batched), _shape(Y, batched))


def mel_filterbank(sr: int, n_fft: int, n_mels: int) -> torch.Tensor:
    """`librosa.filters.mel(sr=sr, n_fft=n_fft, n_mels=n_mels)` -> fp32 [n_mels, 1 + n_fft / 2] on the host (no GPU)."""
    _check_args(sr, n_fft, 1, n_mels)
    L.check(L.lib().jat_mel_filterbank(int(sr), int(n_fft), int(n_mels), None))
    w = np.zeros((int(n_mels), 1 + int(n_fft) // 2), np.float32)
    L.check(L.lib().jat_mel_filterbank(int(sr), int(n_fft), int(n_mels), w.ctypes.data))
    return torch.from_numpy(w)


@torch.no_grad()
def calculate_lsd(pred, gt, n_fft: int = 2048, hop_length: int = 512):
    """-> (lsd_db fp64 [] or [B], lsd_frames fp32 [frames] or [B, frames]), on the device"""
    pred, gt, batched = _pair(pred, gt)
    out, frames, _, _ = _run(pred, gt, 44100, n_fft, hop_length, 0, True)
    return _shape(out[:, 0], batched), _shape(frames, batched)


@torch.no_grad()
def calculate_mel_loss(pred, gt, sr: int = 44100, n_mels: int = 80, n_fft: int = 2048, hop_length: int = 512):
    """-> (mel_l1, mel_l2 fp64 [] or [B], pred_mel_db, gt_mel_db fp32 [..., n_mels, frames]), on the device"""
    if n_mels < 1:
        raise ValueError(f"metrics: n_mels must be at least 1, got {n_mels!r}")
    pred, gt, batched = _pair(pred, gt)
    out, _, pdb, gdb = _run(pred, gt, sr, n_fft, hop_length, n_mels, False, want_db=True)
    return _shape(out[:, 1], batched), _shape(out[:, 2], batched), _shape(pdb, batched), _shape(gdb, batched)


def _scale_mean(v):
    """the reference's running total over the scales divided by their number (calculate_metrics.py:121-128), the same
    IEEE operations on a tensor or a numpy array"""
    total = v[0]
    for i in range(1, len(SCALES)):
        total = total + v[i]
    return total / len(SCALES)


def _three_scales(pred, gt, sr, want_lsd):
    """the three multi-scale passes -> fp64 [3 scales, B, 3]; the 2048 / 512 pass also carries the LSD when asked"""
    out = torch.empty(len(SCALES), pred.shape[0], 3, dtype=torch.float64, device=pred.device)
    for i, (n_fft, hop, n_mels) in enumerate(SCALES):
        _run(pred, gt, sr, n_fft, hop, n_mels, want_lsd and n_fft == 2048, out=out[i])
    return out


@torch.no_grad()
def calculate_multi_scale_mel_loss(pred, gt, sr: int = 44100):
    """-> (avg_l1, avg_l2, {"fft512": {"l1", "l2"}, "fft1024": ..., "fft2048": ...}), fp64 [] or [B] on the device"""
    pred, gt, batched = _pair(pred, gt)
    out = _three_scales(pred, gt, sr, False)
    results = {f"fft{s[0]}": {"l1": _shape(out[i, :, 1], batched), "l2": _shape(out[i, :, 2], batched)}
               for i, s in enumerate(SCALES)}
    return _shape(_scale_mean(out[:, :, 1]), batched), _shape(_scale_mean(out[:, :, 2]), batched), results


def lsd_grade(lsd: float) -> str:
    """calculate_metrics.py:231-240"""
    for bound, name in ((1.0, "Excellent"), (1.5, "Very Good"), (2.0, "Good"), (2.5, "Fair")):
        if lsd < bound:
            return name
    return "Poor"


def mel_grade(mel_l1: float) -> str:
    """calculate_metrics.py:245-252"""
    for bound, name in ((3.0, "Excellent"), (5.0, "Very Good"), (7.0, "Good")):
        if mel_l1 < bound:
            return name
    return "Fair"


def _report(o, batched):
    """o: fp64 numpy [3 scales, B, 3] -> the per-pair dict (floats, or lists of floats for a batch)"""
    def val(a):
        return [float(v) for v in a] if batched else float(a[0])
    last = len(SCALES) - 1
    return {"lsd": val(o[last, :, 0]), "mel_l1": val(o[last, :, 1]), "mel_l2": val(o[last, :, 2]),
            "ms_l1": val(_scale_mean(o[:, :, 1])), "ms_l2": val(_scale_mean(o[:, :, 2])),
            "ms_detail": {f"fft{s[0]}": {"l1": val(o[i, :, 1]), "l2": val(o[i, :, 2])} for i, s in enumerate(SCALES)}}


@torch.no_grad()
def evaluate(pred, gt, lr=None, sr: int = 44100) -> dict:
    """Everything `calculate_metrics.py:main` reports, as Python floats (lists of floats for [B, L] input):
    {"generated": {lsd, mel_l1, mel_l2, ms_l1, ms_l2, ms_detail}, "lsd_grade", "mel_grade"} and, with `lr`,
    {"lr_input": {...}, "improvement": {key: {"abs": lr - generated, "rel": 1 - generated / lr}}}.
    Three transforms per pair: the 2048 / 512 pass serves the LSD, the single-scale mel loss and the third scale."""
    p, g, batched = _pair(pred, gt)
    outs = [_three_scales(p, g, sr, True)]
    if lr is not None:
        pl, gl, bl = _pair(lr, gt)
        if bl != batched or pl.shape[0] != p.shape[0]:
            raise L.JatError("metrics: lr must have the batch shape of pred")
        outs.append(_three_scales(pl, gl, sr, True))
    o = torch.stack(outs).cpu().numpy()                      # the one synchronisation
    rep = {"generated": _report(o[0], batched)}
    gen = rep["generated"]
    if lr is not None:
        rep["lr_input"] = low = _report(o[1], batched)

        def imp(a, b):
            return {"abs": b - a, "rel": 1.0 - a / b if b != 0 else 0.0}
        rep["improvement"] = {k: ([imp(a, b) for a, b in zip(gen[k], low[k])] if batched else imp(gen[k], low[k]))
                              for k in METRIC_KEYS}
    rep["lsd_grade"] = [lsd_grade(v) for v in gen["lsd"]] if batched else lsd_grade(gen["lsd"])
    rep["mel_grade"] = [mel_grade(v) for v in gen["mel_l1"]] if batched else mel_grade(gen["mel_l1"])
    return rep


def load_audio(path, target_sr: int = 44100, device="cuda"):
    """calculate_metrics.py:11-21: read, resample every channel to `target_sr` on the GPU, then average the channels.
    -> (fp32 CUDA [L], target_sr)"""
    from . import io as jio
    from .resample import resample
    x, sr = jio.read_wav(path, mono=False)
    w = torch.from_numpy(np.ascontiguousarray(x)).to(device)
    if sr != target_sr:
        w = resample(w, sr, target_sr)
    return (w.mean(dim=0) if w.shape[0] > 1 else w[0]).contiguous(), target_sr


def format_report(rep: dict) -> str:
    """the summary table of calculate_metrics.py:214-255, plain ASCII"""
    names = {"lsd": "LSD (dB)", "mel_l1": "Mel L1 (dB)", "mel_l2": "Mel L2 (dB)", "ms_l1": "Multi-Scale L1 (dB)",
             "ms_l2": "Multi-Scale L2 (dB)"}
    gen, low, imp = rep["generated"], rep.get("lr_input"), rep.get("improvement")
    lines = ["=" * 80]
    if low is None:
        lines += [f"{'Metric':<22}{'Generated vs GT':>15}", "-" * 80]
        lines += [f"{names[k]:<22}{gen[k]:>15.3f}" for k in METRIC_KEYS]
    else:
        lines += [f"{'Metric':<22}{'Generated vs GT':>15}   {'LR vs GT':>12}    Improvement", "-" * 80]
        lines += [f"{names[k]:<22}{gen[k]:>15.3f}   {low[k]:>12.3f}    {imp[k]['abs']:6.3f} ({imp[k]['rel'] * 100:4.1f}%)"
                  for k in METRIC_KEYS]
    lines += ["-" * 80]
    lines += [f"  {k}: L1={v['l1']:.3f}, L2={v['l2']:.3f}" for k, v in gen["ms_detail"].items()]
    lines += ["=" * 80, f"LSD Grade: {rep['lsd_grade']}", f"Mel Loss Grade: {rep['mel_grade']}", "=" * 80]
    return "\n".join(lines)


def build_parser():
    p = argparse.ArgumentParser(prog="python -m jatsr_amd.metrics",
                                description="LSD and mel-spectrogram losses of a generated WAV against its ground truth, on MI355X")
    p.add_argument("--pred", type=str, required=True, help="generated WAV (any sample rate; resampled to --sr)")
    p.add_argument("--gt", type=str, required=True, help="ground-truth WAV")
    p.add_argument("--lr", type=str, default=None, help="low-resolution input WAV: adds LR vs GT and the improvement")
    p.add_argument("--sr", type=int, default=44100, help="sample rate the metrics are taken at")
    p.add_argument("--json", type=str, default=None, help="write the report as JSON")
    p.add_argument("--device", type=str, default="cuda", help="Device (an AMD GPU; there is no CPU path)")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    L.require_gpu()
    sig = {k: load_audio(getattr(args, k), args.sr, args.device)[0] for k in ("pred", "gt", "lr") if getattr(args, k)}
    for k, v in sig.items():
        print(f"{k:>5}: {v.shape[-1] / args.sr:.2f} s")
    rep = evaluate(sig["pred"], sig["gt"], sig.get("lr"), sr=args.sr)
    print(format_report(rep))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rep, f, indent=2)
    return rep


if __name__ == "__main__":
    main()
