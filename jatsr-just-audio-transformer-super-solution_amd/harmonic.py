"""F0-guided harmonic structure on the GPU: the amplitude of every harmonic of a pitch track in every frame of a recording
(`analyze`), the additive harmonic template of a track (`synthesize`, `generate_harmonics`), and how far the harmonics of a
super-resolved recording agree with the ground truth's below and above the input's band limit (`compare`,
`harmonic_metrics`).  csrc/harmonic.hip behind `jat_harmonic_analyze`, `jat_harmonic_synth` and `jat_harmonic_compare`; the
definitions are in include/jat_hip_harm.h, the fp64 statement in tests/harmonic_ref.py.  With hop_length = 512 at 44.1 kHz a
table has one row per DAC latent frame, as the tracks of jatsr_amd.pitch have.

    amp, energy = analyze(x, f0, voiced, n_harmonics=32)              # fp32 CUDA [frames, H], [frames] (or batched)
    y = synthesize(f0, voiced, amp, length)                           # the oscillator bank; amp may be one [H] vector
    y = generate_harmonics(f0, num_harmonics=5)                       # the roadmap's harmonic template, equal amplitudes
    h = harmonicity(amp, energy)                                      # share of a frame's windowed energy on the harmonics
    report = harmonic_metrics(generated, hr_gt, lr=lr_input)          # dB errors of the kept and the regenerated band

    python -m jatsr_amd.harmonic --pred X_generated.wav --gt X_hr_gt.wav --lr X_lr_input.wav --json out.json
    python -m jatsr_amd.harmonic --pred ... --gt ... --template gt_harmonics.wav --n-harmonics 5

Limits.  A harmonic is read through the Hann window's main lobe, four bins wide: harmonics closer than that leak into each
other, so f0 should be at least 4 sr / frame_length (86 Hz at the defaults; at 55 Hz the round trip of a flat template is off by
up to 4.5 %, at 110 Hz by 0.14 %).  An error of the track is multiplied by h, and so is the real inharmonicity of strings: at h f0 = 8.8 kHz five cents are
25 Hz, more than a bin.  pYIN's f0 is quantised to 10-cent bins, so method="pyin" takes pYIN's voicing and refines the f0 on
the host side of the launch: YIN's f0 of the same frame where it lies within 50 cents of pYIN's bin, pYIN's value elsewhere.
No trained weights and no recordings were involved; whether these figures track perceived quality is not established.
There is no CPU path: a CPU tensor raises.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math

import torch

from . import _lib as L
from .pitch import PYIN_DEFAULTS, _int, _signal, _track, pyin_full, yin_full
from .resample import _on

METHODS = ("yin", "pyin")      # the trackers of reference_track
BAND_KEYS = ("n_cells", "bias_db", "rms_db", "mean_abs_db")
DEFAULT_FLOOR = 1e-5      # amplitude: a reference harmonic under -100 dBFS is not compared


def _table(name, amp, rows=None):
    if not isinstance(amp, torch.Tensor) or not amp.is_cuda:
        raise L.JatError(f"harmonic: {name} must be a CUDA tensor (there is no CPU path)")
    if amp.dtype != torch.float32 or amp.dim() not in (2, 3):
        raise L.JatError(f"harmonic: {name} must be float32 [frames, H] or [B, frames, H]")
    a = amp.detach().reshape((-1,) + tuple(amp.shape[-2:])).contiguous()
    if rows is not None and tuple(a.shape[:2]) != tuple(rows):
        raise L.JatError(f"harmonic: {name} {tuple(amp.shape)} does not match the track {tuple(rows)}")
    return a


@torch.no_grad()
def analyze(x, f0, voiced, n_harmonics: int = 32, sr: int = 44100, frame_length: int = 2048, hop_length: int = 512):
    """x fp32 CUDA [L] or [B, L], the track f0 fp32 / voiced bool or uint8 [frames] or [B, frames], frames = 1 + L // hop_length
    -> (amp fp32 [.., frames, H], energy fp32 [.., frames]).  amp[f, h - 1] is the amplitude of the sinusoid at h f0[f] in the
    Hann-windowed frame centred on sample f hop_length; 0 where the frame is unvoiced or h f0 is within two bins of Nyquist."""
    x = _signal("x", x)
    batched = x.dim() == 2
    if x.numel() < 1:
        raise ValueError("harmonic: the signal must hold at least one sample")
    xs = x.reshape(-1, x.shape[-1]).contiguous()
    B, n = xs.shape
    f, v = _track("the track", f0, voiced)
    H, hop = _int("n_harmonics", n_harmonics), _int("hop_length", hop_length)
    if f.shape[0] != B or f.device != xs.device or (f0.dim() == 2) != batched:
        raise L.JatError(f"harmonic: the track {tuple(f0.shape)} must have the batch shape of x {tuple(x.shape)}")
    frames = f.shape[1]
    dev = xs.device
    with _on(dev):
        amp = torch.empty(B, frames, max(H, 0), dtype=torch.float32, device=dev)
        energy = torch.empty(B, frames, dtype=torch.float32, device=dev)
        L.check(L.lib().jat_harmonic_analyze(L.ptr(xs), B, n, L.ptr(f), L.ptr(v), frames, H, _int("sr", sr),
                                             _int("frame_length", frame_length), hop, L.ptr(amp), L.ptr(energy), L.stream_ptr()))
    return (amp, energy) if batched else (amp[0], energy[0])


@torch.no_grad()
def synthesize(f0, voiced, amp, length: int, sr: int = 44100, hop_length: int = 512, want_phase: bool = False):
    """The track [frames] or [B, frames] with frames = 1 + length // hop_length and amp fp32 [.., frames, H] (or one [H] vector
    used in every frame) -> y fp32 [length] or [B, length]: harmonic h is a sinusoid at h times the linearly interpolated f0
    with linearly interpolated amplitude and one continuous phase per row; it fades over one hop next to an unvoiced frame
    and is absent where h f0 reaches Nyquist.  want_phase: -> (y, phase int32 view of uint32 [.., length]), a test output."""
    f, v = _track("the track", f0, voiced)
    B, frames = f.shape
    if not isinstance(amp, torch.Tensor) or not amp.is_cuda or amp.dtype != torch.float32:
        raise L.JatError("harmonic: amp must be a float32 CUDA tensor (there is no CPU path)")
    if amp.dim() == 1:
        amp = amp.detach().reshape(1, 1, -1).expand(B, frames, -1)
    a = _table("amp", amp, (B, frames))
    n, hop = _int("length", length), _int("hop_length", hop_length)
    if a.device != f.device:
        raise L.JatError("harmonic: amp and the track must be on one device")
    dev = f.device
    need = C.c_size_t()
    L.check(L.lib().jat_harmonic_synth_workspace_bytes(B, n, hop, C.byref(need)))
    with _on(dev):
        y = torch.empty(B, max(n, 0), dtype=torch.float32, device=dev)
        ph = torch.empty(B, max(n, 0), dtype=torch.int32, device=dev) if want_phase else None
        work = torch.empty(need.value, dtype=torch.uint8, device=dev)
        L.check(L.lib().jat_harmonic_synth(L.ptr(f), L.ptr(v), L.ptr(a), B, frames, a.shape[2], n, _int("sr", sr), hop, L.ptr(y),
                                           L.ptr(ph), L.ptr(work), work.numel(), L.stream_ptr()))
    batched = f0.dim() == 2
    y = y if batched else y[0]
    return (y, ph if batched else ph[0]) if want_phase else y


def generate_harmonics(f0_curve, num_harmonics: int = 5, voiced=None, length: int | None = None, sr: int = 44100,
                       hop_length: int = 512):
    """The harmonic template of a track: `num_harmonics` harmonics of equal amplitude 1 / num_harmonics (|y| <= 1).
    voiced None: every frame with a positive finite f0; length None: (frames - 1) hop_length samples."""
    if not isinstance(f0_curve, torch.Tensor) or not f0_curve.is_cuda:
        raise L.JatError("harmonic: f0_curve must be a CUDA tensor (there is no CPU path)")
    H = _int("num_harmonics", num_harmonics)
    if voiced is None:
        voiced = torch.ones_like(f0_curve, dtype=torch.uint8)
    if length is None:
        length = max((f0_curve.shape[-1] - 1) * int(hop_length), 1)
    amp = torch.full((max(H, 0),), 1.0 / max(H, 1), dtype=torch.float32, device=f0_curve.device)
    return synthesize(f0_curve, voiced, amp, length, sr=sr, hop_length=hop_length)


def harmonicity(amp, energy, frame_length: int = 2048):
    """sum_h amp^2 / 2 * sum_n w[n]^2 / energy per frame (sum w^2 = 3 N / 8 for the periodic Hann window): the share of the
    windowed frame's energy that lies on the harmonics; 1 for a harmonic signal, 0 where the energy is 0."""
    num = amp.double().square().sum(-1) * (0.5 * 0.375 * int(frame_length))
    e = energy.double()
    return torch.where(e > 0, num / e.clamp_min(1e-300), torch.zeros_like(e))


def _sums(amp_a, amp_ref, f0_ref, voiced_ref, cutoff_hz, floor, out=None):
    """-> fp64 [B, 8] on the device (jat_harmonic_compare)"""
    f, v = _track("the reference track", f0_ref, voiced_ref)
    r = _table("amp_ref", amp_ref, f.shape)
    a = _table("amp_a", amp_a, f.shape)
    if a.shape != r.shape or a.device != r.device or f.device != r.device:
        raise L.JatError(f"harmonic: the tables {tuple(a.shape)} and {tuple(r.shape)} must have one shape and device")
    B, frames, H = r.shape
    with _on(r.device):
        if out is None:
            out = torch.empty(B, 8, dtype=torch.float64, device=r.device)
        L.check(L.lib().jat_harmonic_compare(L.ptr(a), L.ptr(r), L.ptr(f), L.ptr(v), B, frames, H,
                                             math.inf if cutoff_hz is None else float(cutoff_hz), float(floor), L.ptr(out),
                                             L.stream_ptr()))
    return out


def band_from_sums(s) -> dict:
    """{n, sum e, sum e^2, sum |e|} -> cell count, mean error in dB (bias), RMS dB (a harmonic LSD) and mean |dB|; zeros for
    an empty band"""
    n, s1, s2, sa = (float(v) for v in s)
    if n <= 0:
        return {"n_cells": 0, "bias_db": 0.0, "rms_db": 0.0, "mean_abs_db": 0.0}
    return {"n_cells": int(n), "bias_db": s1 / n, "rms_db": math.sqrt(max(s2 / n, 0.0)), "mean_abs_db": sa / n}


def report_from_sums(row, banded: bool) -> dict:
    """one row of jat_harmonic_compare -> {"all": band} and, when a cutoff split the cells, {"kept", "regenerated"} too"""
    row = [float(v) for v in row]
    rep = {"all": band_from_sums([row[i] + row[4 + i] for i in range(4)])}
    if banded:
        rep["kept"], rep["regenerated"] = band_from_sums(row[:4]), band_from_sums(row[4:])
    return rep


@torch.no_grad()
def compare(amp_a, amp_ref, f0_ref, voiced_ref, cutoff_hz: float | None = None, floor: float = DEFAULT_FLOOR):
    """Two tables [frames, H] or [B, frames, H], the second the reference with its track -> report_from_sums of each row (a
    list for a batch).  A cell counts where the reference frame is voiced and amp_ref > floor; its error is
    20 log10((amp_a + floor) / (amp_ref + floor)); cells with h f0_ref < cutoff_hz are the kept band."""
    o = _sums(amp_a, amp_ref, f0_ref, voiced_ref, cutoff_hz, floor).cpu().numpy()
    reps = [report_from_sums(r, cutoff_hz is not None) for r in o]
    return reps if amp_ref.dim() == 3 else reps[0]


def refine_f0(f0_bins, voiced, f0_yin):
    """pYIN's f0 (bin centres, 0 where unvoiced) with YIN's f0 of the same frames -> YIN's value where the frame is voiced and
    it lies within 50 cents of the bin, pYIN's elsewhere.  A torch.where, no kernel."""
    near = (voiced != 0) & (f0_yin > 0) & (f0_bins > 0)
    near = near & ((1200.0 * torch.log2(f0_yin.clamp_min(1e-30) / f0_bins.clamp_min(1e-30))).abs() <= 50.0)
    return torch.where(near, f0_yin, f0_bins)


def reference_track(gt, method: str = "yin", sr: int = 44100, frame_length: int = 2048, hop_length: int = 512, **pitch_kw):
    """gt fp32 CUDA [B, L] -> (f0 fp32, voiced uint8) [B, frames] for the analysis.  "yin": YIN's track.  "pyin": pYIN's
    voicing, and YIN's f0 where it lies within 50 cents of pYIN's 10-cent bin, pYIN's elsewhere."""
    if method not in METHODS:
        raise ValueError(f"harmonic: method must be one of {METHODS}, got {method!r}")
    prior = {k: pitch_kw.pop(k) for k in list(pitch_kw) if k in PYIN_DEFAULTS}
    if prior and method == "yin":
        raise TypeError(f"harmonic: {sorted(prior)} are arguments of method='pyin'")
    unknown = set(pitch_kw) - {"fmin", "fmax", "trough_threshold"}
    if unknown:
        raise TypeError(f"harmonic: unknown pitch argument {sorted(unknown)}")
    kw = dict(sr=sr, frame_length=frame_length, hop_length=hop_length)
    ry = yin_full(gt, **kw, **pitch_kw)
    if method == "yin":
        return ry["f0"], ry["voiced"]
    pitch_kw.pop("trough_threshold", None)
    rp = pyin_full(gt, **kw, **pitch_kw, **prior)
    return refine_f0(rp["f0"], rp["voiced"], ry["f0"]), rp["voiced"]


@torch.no_grad()
def harmonic_metrics(pred, gt, lr=None, cutoff_hz: float | None = None, n_harmonics: int = 64, method: str = "yin",
                     sr: int = 44100, frame_length: int = 2048, hop_length: int = 512, floor: float = DEFAULT_FLOOR,
                     tables: dict | None = None, **pitch_kw) -> dict:
    """Harmonic preservation of `pred` (and of `lr`) against the reference recording `gt`: fp32 CUDA [L] or [B, L], all cut to
    the shortest.  The track is taken from `gt` (reference_track) and all signals are analysed at that one track.
    cutoff_hz None: splice.detect_cutoff(lr) when lr is given (its own host copy), no band split otherwise.
    -> {"generated": {"all": band, ["kept": band, "regenerated": band]}, ["lr_input": ...], "harmonicity": {"generated",
    "gt", ["lr_input"]} (mean over the frames voiced in gt), "cutoff_hz", "n_harmonics", "n_voiced", "n_frames"}, with
    band = BAND_KEYS; Python numbers (lists for a batch) after one device-to-host copy.  `tables`, when a dict, receives the
    device tensors {"f0", "voiced", "pred": (amp, energy), "gt": ..., "lr": ...} and the common "length".  See the module docstring for the limits."""
    sig = [_signal("pred", pred), _signal("gt", gt)] + ([_signal("lr", lr)] if lr is not None else [])
    if any(s.dim() != sig[0].dim() or s.shape[:-1] != sig[0].shape[:-1] or s.device != sig[0].device for s in sig):
        raise L.JatError("harmonic: pred, gt and lr must agree but for their length")
    n = min(s.shape[-1] for s in sig)
    if n < 1:
        raise ValueError("harmonic: the signals must hold at least one sample")
    batched = sig[0].dim() == 2
    rows = [s[..., :n].reshape(-1, n) for s in sig]
    B, S = rows[0].shape[0], len(rows)
    if cutoff_hz is None and lr is not None:
        from .splice import detect_cutoff
        cut = detect_cutoff(rows[2].contiguous(), sr=sr)
        if len(set(cut)) > 1:
            raise ValueError(f"harmonic: the rows of lr have different band limits {cut}; pass cutoff_hz")
        cutoff_hz = cut[0]
    kw = dict(sr=sr, frame_length=frame_length, hop_length=hop_length)
    f0, voiced = reference_track(rows[1].contiguous(), method, **kw, **pitch_kw)
    amp, energy = analyze(torch.cat(rows), f0.repeat(S, 1), voiced.repeat(S, 1), n_harmonics=n_harmonics, **kw)
    amp, energy = amp.reshape(S, B, *amp.shape[1:]), energy.reshape(S, B, -1)
    out = torch.empty(S - 1, B, 8, dtype=torch.float64, device=amp.device)
    _sums(amp[0], amp[1], f0, voiced, cutoff_hz, floor, out=out[0])
    if lr is not None:
        _sums(amp[2], amp[1], f0, voiced, cutoff_hz, floor, out=out[1])
    vm = ((voiced != 0) & (f0 > 0) & torch.isfinite(f0)).double()                       # [B, frames]
    hm = (harmonicity(amp, energy, frame_length) * vm).sum(-1)                          # [S, B]
    host = torch.cat([out.reshape(-1), hm.reshape(-1), vm.sum(-1)]).cpu().numpy()       # the one synchronisation
    o, hm, nv = host[:out.numel()].reshape(S - 1, B, 8), host[out.numel():out.numel() + S * B].reshape(S, B), host[-B:]
    if tables is not None:
        tables.update(f0=f0, voiced=voiced, length=n, pred=(amp[0], energy[0]), gt=(amp[1], energy[1]))
        if lr is not None:
            tables.update(lr=(amp[2], energy[2]))

    def shape(v):
        return list(v) if batched else v[0]
    banded = cutoff_hz is not None
    rep = {"generated": shape([report_from_sums(r, banded) for r in o[0]])}
    if lr is not None:
        rep["lr_input"] = shape([report_from_sums(r, banded) for r in o[1]])
    mean = [[float(hm[s, b] / nv[b]) if nv[b] > 0 else 0.0 for b in range(B)] for s in range(S)]
    rep["harmonicity"] = {k: shape(mean[i]) for i, k in enumerate(("generated", "gt", "lr_input")[:S])}
    rep.update(cutoff_hz=None if cutoff_hz is None else float(cutoff_hz), n_harmonics=int(n_harmonics),
               n_voiced=shape([int(v) for v in nv]), n_frames=int(f0.shape[-1]))
    return rep


def format_report(rep: dict) -> str:
    """a few plain ASCII lines for one (unbatched) report of harmonic_metrics"""
    low = rep.get("lr_input")
    cut = rep["cutoff_hz"]
    lines = [f"{'Harmonics vs GT (dB)':<30}{'Generated':>12}" + (f"{'LR':>12}" if low else "")]
    for band in ("kept", "regenerated", "all"):
        if band not in rep["generated"]:
            continue
        for k in BAND_KEYS[1:]:
            lines.append(f"{band + ' ' + k:<30}{rep['generated'][band][k]:>12.3f}" + (f"{low[band][k]:>12.3f}" if low else ""))
        lines.append(f"{band + ' cells':<30}{rep['generated'][band]['n_cells']:>12d}" + (f"{low[band]['n_cells']:>12d}" if low else ""))
    h = rep["harmonicity"]
    lines.append(f"{'harmonicity (GT ' + format(h['gt'], '.3f') + ')':<30}{h['generated']:>12.3f}" + (f"{h['lr_input']:>12.3f}" if low else ""))
    lines.append(f"band limit {'none' if cut is None else format(cut, '.1f') + ' Hz'}, {rep['n_harmonics']} harmonics, "
                 f"{rep['n_voiced']}/{rep['n_frames']} frames voiced in GT")
    return "\n".join(lines)


def build_parser():
    p = argparse.ArgumentParser(prog="python -m jatsr_amd.harmonic",
                                description="Harmonic amplitudes of a generated WAV and its ground truth at the ground truth's "
                                            "pitch track, below and above the input's band limit, on MI355X")
    p.add_argument("--pred", type=str, required=True, help="generated WAV (any sample rate; resampled to --sr)")
    p.add_argument("--gt", type=str, required=True, help="ground-truth WAV: the track and the reference amplitudes")
    p.add_argument("--lr", type=str, default=None, help="low-resolution input WAV: adds LR vs GT and the detected band limit")
    p.add_argument("--sr", type=int, default=44100, help="sample rate of the analysis")
    p.add_argument("--cutoff-hz", type=float, default=None, help="band limit between kept and regenerated harmonics (default: detected from --lr)")
    p.add_argument("--n-harmonics", type=int, default=64, help="harmonics per frame (1..128)")
    p.add_argument("--method", choices=METHODS, default="yin", help="the tracker of the ground truth's pitch")
    p.add_argument("--frame-length", type=int, default=2048, help="samples per analysis frame (even, 16..8192)")
    p.add_argument("--hop-length", type=int, default=512, help="samples between frames (512: one row per DAC latent frame)")
    p.add_argument("--json", type=str, default=None, help="write the report as JSON")
    p.add_argument("--template", type=str, default=None,
                   help="write the ground truth's harmonic template as WAV: its first --n-harmonics harmonics at the analysed amplitudes")
    p.add_argument("--device", type=str, default="cuda", help="Device (an AMD GPU; there is no CPU path)")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    L.require_gpu()
    from .metrics import load_audio
    sig = {k: load_audio(getattr(args, k), args.sr, args.device)[0] for k in ("pred", "gt", "lr") if getattr(args, k)}
    for k, v in sig.items():
        print(f"{k:>5}: {v.shape[-1] / args.sr:.2f} s")
    tables: dict = {}
    rep = harmonic_metrics(sig["pred"], sig["gt"], sig.get("lr"), cutoff_hz=args.cutoff_hz, n_harmonics=args.n_harmonics,
                           method=args.method, sr=args.sr, frame_length=args.frame_length, hop_length=args.hop_length,
                           tables=tables)
    print(format_report(rep))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rep, f, indent=2)
    if args.template:
        from . import io as jio
        f0, voiced = tables["f0"][0], tables["voiced"][0]
        y = synthesize(f0, voiced, tables["gt"][0][0], tables["length"], sr=args.sr, hop_length=args.hop_length)
        jio.write_wav_float32(args.template, y, args.sr)
        print(f"harmonic template of the ground truth -> {args.template}")
    return rep


if __name__ == "__main__":
    main()
