"""Pitch tracking on the GPU and F0-preservation figures between two recordings.  YIN (de Cheveigne & Kawahara 2002, steps
1-5, arranged as librosa.yin arranges them): csrc/pitch.hip behind `jat_yin` and `jat_f0_compare`.  pYIN (Mauch & Dixon 2014,
arranged as librosa.pyin arranges it): YIN's normalised difference, every trough spread over a prior of thresholds, and the
track decoded by a Viterbi pass over pitch bins, csrc/pyin.hip behind `jat_pyin_track`.  The definitions are in
include/jat_hip.h, the fp64 statements in tests/pitch_ref.py and tests/pyin_ref.py.  With hop_length = 512 at 44.1 kHz a
track has one value per DAC latent frame.

    f0, voiced, aperiodicity = yin(x)                                  # fp32 CUDA [L] or [B, L] -> [frames] or [B, frames]
    f0, voiced, voiced_prob = pyin(x)                                  # f0 quantised to 100 * resolution cents, 0 where unvoiced
    counts = compare_f0(f0_a, voiced_a, f0_ref, voiced_ref)            # rates and mean |cents|, the reference track second
    report = f0_metrics(generated, hr_gt, lr=lr_input)                 # {"generated": ..., "lr_input": ...}, one host copy
    report = f0_metrics(generated, hr_gt, method="pyin")               # the same figures from pYIN tracks

    python -m jatsr_amd.pitch --pred X_generated.wav --gt X_hr_gt.wav --lr X_lr_input.wav --json out.json --track out.npy
    python -m jatsr_amd.pitch --method pyin --pred ... --gt ...

`yin` decides every frame alone; `pyin` adds the probabilistic smoothing of Mauch & Dixon.  Neither is a learned tracker,
neither was compared with librosa or CREPE, and octave errors on real music were not studied.
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

COUNT_KEYS = ("n_frames", "n_ref_voiced", "n_both_voiced", "n_voicing_errors", "n_gross")
RATE_KEYS = ("voicing_error_rate", "gross_error_rate", "raw_pitch_accuracy", "mean_abs_cents", "fine_mean_abs_cents")
DEFAULTS = dict(sr=44100, fmin=50.0, fmax=1000.0, frame_length=2048, hop_length=512, trough_threshold=0.1)


def periods(sr: int = 44100, fmin: float = 50.0, fmax: float = 1000.0, frame_length: int = 2048):
    """-> (min_period, max_period) in samples, as the kernel uses them (host arithmetic of the library; no GPU needed)"""
    lo, hi = C.c_int32(), C.c_int32()
    L.check(L.lib().jat_yin_periods(_int("sr", sr), float(fmin), float(fmax), _int("frame_length", frame_length),
                                    C.byref(lo), C.byref(hi)))
    return lo.value, hi.value


def _int(name, v):
    if int(v) != v:
        raise ValueError(f"pitch: {name} must be an integer, got {v!r}")
    return int(v)


def _signal(name, x):
    if not isinstance(x, torch.Tensor) or x.dim() not in (1, 2):
        raise L.JatError(f"pitch: {name} must be a tensor [L] or [B, L]")
    if not x.is_cuda:
        raise L.JatError(f"pitch: {name} must be a CUDA tensor (there is no CPU path)")
    if x.dtype != torch.float32:
        raise L.JatError(f"pitch: {name} must be float32, got {x.dtype}")
    return x.detach()


@torch.no_grad()
def yin_full(x, sr=44100, fmin=50.0, fmax=1000.0, frame_length=2048, hop_length=512, trough_threshold=0.1, want=()):
    """`yin` with the unit-test outputs named in `want` ("index", "d", "cmndf") -> dict of device tensors"""
    x = _signal("x", x)
    batched = x.dim() == 2
    if x.numel() < 1:
        raise ValueError("pitch: the signal must hold at least one sample")
    xs = x.reshape(-1, x.shape[-1]).contiguous()
    B, n = xs.shape
    par = L.JatYinParams(float(fmin), float(fmax), _int("sr", sr), _int("frame_length", frame_length),
                         _int("hop_length", hop_length), float(trough_threshold))
    lo, hi = periods(par.sr, par.fmin, par.fmax, par.frame_length)
    if par.hop_length < 1:
        raise ValueError(f"pitch: hop_length {par.hop_length} must be at least 1")
    frames = 1 + n // par.hop_length
    dev = xs.device
    with _on(dev):
        out = {"f0": torch.empty(B, frames, dtype=torch.float32, device=dev),
               "aperiodicity": torch.empty(B, frames, dtype=torch.float32, device=dev),
               "voiced": torch.empty(B, frames, dtype=torch.uint8, device=dev)}
        if frames * (hi + 1) < 2 ** 31:          # beyond it the library refuses below, before anything is read
            if "index" in want:
                out["index"] = torch.empty(B, frames, dtype=torch.int32, device=dev)
            for k in ("d", "cmndf"):
                if k in want:
                    out[k] = torch.empty(B, frames, hi + 1, dtype=torch.float32, device=dev)
        L.check(L.lib().jat_yin(C.byref(par), L.ptr(xs), B, n, L.ptr(out["f0"]), L.ptr(out["aperiodicity"]),
                                L.ptr(out["voiced"]), L.ptr(out.get("index")), L.ptr(out.get("d")), L.ptr(out.get("cmndf")),
                                L.stream_ptr()))
    return {k: (v if batched else v[0]) for k, v in out.items()}


def yin(x, sr: int = 44100, fmin: float = 50.0, fmax: float = 1000.0, frame_length: int = 2048, hop_length: int = 512,
        trough_threshold: float = 0.1):
    """fp32 CUDA [L] or [B, L] -> (f0 fp32, voiced bool, aperiodicity fp32), each [frames] or [B, frames] with
    frames = 1 + L // hop_length, on the device.  f0 is reported for every frame; `voiced` says where a trough of the
    normalised difference lies under the threshold."""
    r = yin_full(x, sr, fmin, fmax, frame_length, hop_length, trough_threshold)
    return r["f0"], r["voiced"].view(torch.bool), r["aperiodicity"]


PYIN_DEFAULTS = dict(n_thresholds=100, beta_parameters=(2.0, 18.0), boltzmann_parameter=2.0, resolution=0.1,
                     max_transition_rate=35.92, switch_prob=0.01, no_trough_prob=0.01)
PYIN_WANT = ("cmndf", "prob", "bin", "obs", "log_obs", "state")
_pyin_handles: dict = {}


class PyinHandle:
    """one `jat_pyin` of the library: a parameter set with its host-made tables"""

    def __init__(self, par):
        self.h = C.c_void_p()
        L.check(L.lib().jat_pyin_create(C.byref(par), C.byref(self.h)))
        v = [C.c_int32() for _ in range(4)]
        L.check(L.lib().jat_pyin_shape(self.h, *(C.byref(q) for q in v)))
        self.n_bins, self.H, self.min_period, self.max_period = (q.value for q in v)
        self.n_thresholds, self.hop_length = par.n_thresholds, par.hop_length

    def tables(self) -> dict:
        """host copies: beta fp64 [n_thresholds], logw fp32 [2 H + 1], logZ and freqs fp32 [n_bins], lk, ls, logpi"""
        t = {"beta": np.zeros(self.n_thresholds, np.float64), "logw": np.zeros(2 * self.H + 1, np.float32),
             "logZ": np.zeros(self.n_bins, np.float32), "freqs": np.zeros(self.n_bins, np.float32), "scalars": np.zeros(3, np.float32)}
        L.check(L.lib().jat_pyin_tables(self.h, *(C.c_void_p(t[k].ctypes.data) for k in ("beta", "logw", "logZ", "freqs", "scalars"))))
        lk, ls, logpi = (np.float32(v) for v in t.pop("scalars"))
        return dict(t, lk=lk, ls=ls, logpi=logpi)

    def workspace_bytes(self, B, n) -> int:
        sz = C.c_size_t()
        L.check(L.lib().jat_pyin_workspace_bytes(self.h, B, n, C.byref(sz)))
        return sz.value

    def __del__(self):
        if getattr(self, "h", None) and L._lib is not None:
            L._lib.jat_pyin_destroy(self.h)
            self.h = None


def pyin_handle(sr=44100, fmin=50.0, fmax=1000.0, frame_length=2048, hop_length=512, n_thresholds=100,
                beta_parameters=(2.0, 18.0), boltzmann_parameter=2.0, resolution=0.1, max_transition_rate=35.92,
                switch_prob=0.01, no_trough_prob=0.01, device=None) -> PyinHandle:
    """the handle of a parameter set on a device, made once per process (creating one needs no GPU).  The library binds a
    handle's tables to the device of its first track, so the cache holds one handle per (parameters, device index);
    device None: a handle for host use (shape, tables) that is never given a track."""
    a, b = beta_parameters
    key = (_int("sr", sr), float(fmin), float(fmax), _int("frame_length", frame_length), _int("hop_length", hop_length),
           _int("n_thresholds", n_thresholds), float(a), float(b), float(boltzmann_parameter), float(resolution),
           float(max_transition_rate), float(switch_prob), float(no_trough_prob))
    key = key + (None if device is None else torch.device(device).index if torch.device(device).index is not None
                 else torch.cuda.current_device(),)
    if key not in _pyin_handles:
        _pyin_handles[key] = PyinHandle(L.JatPyinParams(key[1], key[2], key[0], *key[3:-1]))
    return _pyin_handles[key]


@torch.no_grad()
def pyin_full(x, sr=44100, fmin=50.0, fmax=1000.0, frame_length=2048, hop_length=512, want=(), **prior):
    """`pyin` with the unit-test outputs named in `want` (PYIN_WANT) -> dict of device tensors; `prior`: PYIN_DEFAULTS' keys"""
    x = _signal("x", x)
    batched = x.dim() == 2
    if x.numel() < 1:
        raise ValueError("pitch: the signal must hold at least one sample")
    unknown = set(prior) - set(PYIN_DEFAULTS)
    if unknown or set(want) - set(PYIN_WANT):
        raise TypeError(f"pitch: unknown pyin argument {sorted(unknown) or sorted(set(want) - set(PYIN_WANT))}")
    h = pyin_handle(sr, fmin, fmax, frame_length, hop_length, device=x.device, **prior)
    xs = x.reshape(-1, x.shape[-1]).contiguous()
    B, n = xs.shape
    frames = 1 + n // h.hop_length
    ny = h.max_period - h.min_period + 1
    dev = xs.device
    with _on(dev):
        work = torch.empty(h.workspace_bytes(B, n), dtype=torch.uint8, device=dev)      # refuses sizes beyond 31 bits
        out = {"f0": torch.empty(B, frames, dtype=torch.float32, device=dev),
               "voiced": torch.empty(B, frames, dtype=torch.uint8, device=dev),
               "voiced_prob": torch.empty(B, frames, dtype=torch.float32, device=dev)}
        shapes = {"cmndf": ((h.max_period + 1,), torch.float32), "prob": ((ny,), torch.float32), "bin": ((ny,), torch.int32),
                  "obs": ((h.n_bins,), torch.float32), "log_obs": ((h.n_bins + 1,), torch.float32), "state": ((), torch.int32)}
        for k in PYIN_WANT:
            if k in want:
                out[k] = torch.empty((B, frames) + shapes[k][0], dtype=shapes[k][1], device=dev)
        L.check(L.lib().jat_pyin_track(h.h, L.ptr(xs), B, n, L.ptr(out["f0"]), L.ptr(out["voiced"]), L.ptr(out["voiced_prob"]),
                                       *(L.ptr(out.get(k)) for k in PYIN_WANT), L.ptr(work), work.numel(), L.stream_ptr()))
    return {k: (v if batched else v[0]) for k, v in out.items()}


@torch.no_grad()
def pyin_decode(log_obs, sr=44100, fmin=50.0, fmax=1000.0, frame_length=2048, hop_length=512, **prior):
    """The Viterbi stage alone (`jat_pyin_decode`): log_obs fp32 CUDA [frames, n_bins + 1] or [B, frames, n_bins + 1], the last
    entry of a frame being every unvoiced state's -> dict(state int32, f0, voiced uint8), each [frames] or [B, frames]"""
    if not isinstance(log_obs, torch.Tensor) or not log_obs.is_cuda or log_obs.dtype != torch.float32 or log_obs.dim() not in (2, 3):
        raise L.JatError("pitch: log_obs must be a float32 CUDA tensor [frames, n_bins + 1] or [B, frames, n_bins + 1]")
    h = pyin_handle(sr, fmin, fmax, frame_length, hop_length, device=log_obs.device, **prior)
    lo = log_obs.detach().reshape((-1,) + tuple(log_obs.shape[-2:])).contiguous()
    B, frames, width = lo.shape
    if width != h.n_bins + 1 or frames < 1:
        raise ValueError(f"pitch: log_obs must hold n_bins + 1 = {h.n_bins + 1} values a frame and at least one frame")
    dev = lo.device
    with _on(dev):
        out = {"state": torch.empty(B, frames, dtype=torch.int32, device=dev), "f0": torch.empty(B, frames, device=dev),
               "voiced": torch.empty(B, frames, dtype=torch.uint8, device=dev)}
        work = torch.empty(B * frames * h.n_bins * 4, dtype=torch.uint8, device=dev)
        L.check(L.lib().jat_pyin_decode(h.h, L.ptr(lo), B, frames, L.ptr(out["state"]), L.ptr(out["f0"]), L.ptr(out["voiced"]),
                                        L.ptr(work), work.numel(), L.stream_ptr()))
    return {k: (v if log_obs.dim() == 3 else v[0]) for k, v in out.items()}


def pyin(x, sr: int = 44100, fmin: float = 50.0, fmax: float = 1000.0, frame_length: int = 2048, hop_length: int = 512,
         **prior):
    """fp32 CUDA [L] or [B, L] -> (f0 fp32, voiced bool, voiced_prob fp32), each [frames] or [B, frames] with
    frames = 1 + L // hop_length, on the device.  f0 is the centre of the decoded pitch bin, so it is quantised to
    100 * resolution cents (10 cents by default) above fmin, and it is 0 where the frame is unvoiced (librosa: NaN).
    `prior`: n_thresholds, beta_parameters, boltzmann_parameter, resolution, max_transition_rate, switch_prob, no_trough_prob."""
    r = pyin_full(x, sr, fmin, fmax, frame_length, hop_length, **prior)
    return r["f0"], r["voiced"].view(torch.bool), r["voiced_prob"]


def _track(name, f0, voiced):
    if not (isinstance(f0, torch.Tensor) and isinstance(voiced, torch.Tensor)) or not (f0.is_cuda and voiced.is_cuda):
        raise L.JatError(f"pitch: {name} must be CUDA tensors (there is no CPU path)")
    if f0.dtype != torch.float32 or voiced.dtype not in (torch.bool, torch.uint8) or f0.shape != voiced.shape or \
            f0.dim() not in (1, 2):
        raise L.JatError(f"pitch: {name} must be f0 float32 and voiced bool / uint8 of one shape [frames] or [B, frames]")
    f0 = f0.detach().reshape(-1, f0.shape[-1]).contiguous()
    voiced = voiced.detach().reshape(f0.shape).contiguous()
    return f0, voiced.view(torch.uint8) if voiced.dtype == torch.bool else voiced


def _counts(f0_a, voiced_a, f0_b, voiced_b, gross_cents, out=None):
    """-> fp64 [B, 6] on the device (jat_f0_compare)"""
    fa, va = _track("track a", f0_a, voiced_a)
    fb, vb = _track("track b", f0_b, voiced_b)
    if fa.shape != fb.shape or fa.device != fb.device:
        raise L.JatError(f"pitch: the tracks {tuple(fa.shape)} and {tuple(fb.shape)} must have one shape")
    B, frames = fa.shape
    with _on(fa.device):
        if out is None:
            out = torch.empty(B, 6, dtype=torch.float64, device=fa.device)
        L.check(L.lib().jat_f0_compare(L.ptr(fa), L.ptr(va), L.ptr(fb), L.ptr(vb), B, frames, float(gross_cents), L.ptr(out),
                                       L.stream_ptr()))
    return out


def report_from_counts(counts, frames: int) -> dict:
    """The six figures of one row of jat_f0_compare and the frame count -> the report.
    voicing_error_rate = flags that differ / frames;  gross_error_rate = gross / both voiced;  raw_pitch_accuracy = both voiced
    and within gross_cents / voiced in the reference;  mean_abs_cents over the both-voiced frames, fine_mean_abs_cents over
    those that are not gross.  A rate whose denominator is 0 is 0."""
    n_ref, n_both, n_verr, n_gross, s_all, s_fine = (float(v) for v in counts)

    def ratio(a, b):
        return a / b if b > 0 else 0.0
    return {"voicing_error_rate": ratio(n_verr, float(frames)), "gross_error_rate": ratio(n_gross, n_both),
            "raw_pitch_accuracy": ratio(n_both - n_gross, n_ref), "mean_abs_cents": ratio(s_all, n_both),
            "fine_mean_abs_cents": ratio(s_fine, n_both - n_gross), "n_frames": int(frames), "n_ref_voiced": int(n_ref),
            "n_both_voiced": int(n_both), "n_voicing_errors": int(n_verr), "n_gross": int(n_gross)}


def _reports(o, frames, batched):
    rows = [report_from_counts(r, frames) for r in o]
    return {k: [r[k] for r in rows] for k in rows[0]} if batched else rows[0]


@torch.no_grad()
def compare_f0(f0_a, voiced_a, f0_b, voiced_b, gross_cents: float = 50.0) -> dict:
    """Two tracks [frames] or [B, frames] on the device, (f0_b, voiced_b) being the reference -> dict of Python numbers
    (lists for a batch): the RATE_KEYS and the COUNT_KEYS.  cents = 1200 log2(f0_a / f0_b)."""
    o = _counts(f0_a, voiced_a, f0_b, voiced_b, gross_cents).cpu().numpy()
    return _reports(o, f0_a.shape[-1], f0_a.dim() == 2)


def _tracks_of_pair(a, ref, method="yin", **kw):
    """-> (a [B, n], ref [B, n], batched, tracks of a, tracks of ref): both cut to the shorter, one launch for the two"""
    a, ref = _signal("pred", a), _signal("gt", ref)
    if a.dim() != ref.dim() or a.shape[:-1] != ref.shape[:-1] or a.device != ref.device:
        raise L.JatError(f"pitch: pred {tuple(a.shape)} and gt {tuple(ref.shape)} must agree but for their length")
    n = min(a.shape[-1], ref.shape[-1])
    if n < 1:
        raise ValueError("pitch: the signals must hold at least one sample")
    a2, r2 = (v[..., :n].reshape(-1, n) for v in (a, ref))
    B = a2.shape[0]
    r = yin_full(torch.cat([a2, r2]), **kw) if method == "yin" else pyin_full(torch.cat([a2, r2]), **kw)
    return a.dim() == 2, (r["f0"][:B], r["voiced"][:B]), (r["f0"][B:], r["voiced"][B:])


@torch.no_grad()
def f0_metrics(pred, gt, lr=None, sr: int = 44100, fmin: float = 50.0, fmax: float = 1000.0, frame_length: int = 2048,
               hop_length: int = 512, trough_threshold: float = 0.1, gross_cents: float = 50.0, tracks: dict | None = None,
               method: str = "yin", **prior):
    """F0 preservation of `pred` (and of `lr`) against the reference recording `gt`: fp32 CUDA [L] or [B, L], each pair cut
    to its shorter length -> {"generated": report, "lr_input": report} of Python numbers, after one device-to-host copy.
    `tracks`, when a dict, receives the device tracks {"pred": (f0, voiced), "gt": ..., "lr": ...}.
    method "yin" (the default) or "pyin" (`prior`: its PYIN_DEFAULTS keys; trough_threshold is not used, and f0 is quantised
    to pitch bins, so two pYIN tracks differ by whole bins)."""
    if method not in ("yin", "pyin"):
        raise ValueError(f"pitch: method must be 'yin' or 'pyin', got {method!r}")
    if prior and method == "yin":
        raise TypeError(f"pitch: {sorted(prior)} are arguments of method='pyin'")
    kw = dict(sr=sr, fmin=fmin, fmax=fmax, frame_length=frame_length, hop_length=hop_length)
    kw = dict(kw, trough_threshold=trough_threshold) if method == "yin" else dict(kw, method="pyin", **prior)
    batched, tp, tg = _tracks_of_pair(pred, gt, **kw)
    outs, frames = [_counts(*tp, *tg, gross_cents)], [tp[0].shape[-1]]
    if tracks is not None:
        tracks.update(pred=tp, gt=tg)
    if lr is not None:
        bl, tl, tgl = _tracks_of_pair(lr, gt, **kw)
        if bl != batched or tl[0].shape[0] != tp[0].shape[0]:
            raise L.JatError("pitch: lr must have the batch shape of pred")
        outs.append(_counts(*tl, *tgl, gross_cents))
        frames.append(tl[0].shape[-1])
        if tracks is not None:
            tracks.update(lr=tl)
    o = torch.stack(outs).cpu().numpy()                      # the one synchronisation
    rep = {"generated": _reports(o[0], frames[0], batched)}
    if lr is not None:
        rep["lr_input"] = _reports(o[1], frames[1], batched)
    return rep


def format_report(rep: dict, method: str = "yin") -> str:
    """a few plain ASCII lines for one (unbatched) report of f0_metrics"""
    names = {"voicing_error_rate": "Voicing error rate", "gross_error_rate": "Gross pitch error rate",
             "raw_pitch_accuracy": "Raw pitch accuracy", "mean_abs_cents": "Mean |cents| (voiced)",
             "fine_mean_abs_cents": "Mean |cents| (not gross)"}
    gen, low = rep["generated"], rep.get("lr_input")
    lines = [f"{'F0 (pYIN) vs GT' if method == 'pyin' else 'F0 (YIN) vs GT':<26}{'Generated':>12}" + (f"{'LR':>12}" if low else "")]
    for k in RATE_KEYS:
        lines.append(f"{names[k]:<26}{gen[k]:>12.4f}" + (f"{low[k]:>12.4f}" if low else ""))
    lines.append(f"{'Voiced in GT / frames':<26}{gen['n_ref_voiced']:>6d}/{gen['n_frames']:<5d}")
    return "\n".join(lines)


def build_parser():
    p = argparse.ArgumentParser(prog="python -m jatsr_amd.pitch",
                                description="YIN pitch tracks of a generated WAV and its ground truth, and how far they agree, on MI355X")
    p.add_argument("--pred", type=str, required=True, help="generated WAV (any sample rate; resampled to --sr)")
    p.add_argument("--gt", type=str, required=True, help="ground-truth WAV: the reference track")
    p.add_argument("--lr", type=str, default=None, help="low-resolution input WAV: adds LR vs GT")
    p.add_argument("--sr", type=int, default=44100, help="sample rate the tracks are taken at")
    p.add_argument("--fmin", type=float, default=50.0, help="lowest pitch searched, Hz")
    p.add_argument("--fmax", type=float, default=1000.0, help="highest pitch searched, Hz")
    p.add_argument("--frame-length", type=int, default=2048, help="samples per analysis frame (even, 16..8192)")
    p.add_argument("--hop-length", type=int, default=512, help="samples between frames (512: one value per DAC latent frame)")
    p.add_argument("--trough-threshold", type=float, default=0.1, help="a frame is voiced when a trough lies under it")
    p.add_argument("--method", choices=("yin", "pyin"), default="yin",
                   help="yin: every frame alone; pyin: threshold prior and Viterbi decoding (--trough-threshold is not used)")
    p.add_argument("--gross-cents", type=float, default=50.0, help="a both-voiced frame further off than this is a gross error")
    p.add_argument("--json", type=str, default=None, help="write the report as JSON")
    p.add_argument("--track", type=str, default=None,
                   help="write the tracks as .npy: fp32 [2 per signal, frames], rows f0 and voiced of pred, gt (and lr)")
    p.add_argument("--device", type=str, default="cuda", help="Device (an AMD GPU; there is no CPU path)")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    L.require_gpu()
    from .metrics import load_audio
    sig = {k: load_audio(getattr(args, k), args.sr, args.device)[0] for k in ("pred", "gt", "lr") if getattr(args, k)}
    for k, v in sig.items():
        print(f"{k:>5}: {v.shape[-1] / args.sr:.2f} s")
    tracks: dict = {}
    rep = f0_metrics(sig["pred"], sig["gt"], sig.get("lr"), sr=args.sr, fmin=args.fmin, fmax=args.fmax,
                     frame_length=args.frame_length, hop_length=args.hop_length, trough_threshold=args.trough_threshold,
                     gross_cents=args.gross_cents, tracks=tracks, **({"method": "pyin"} if args.method == "pyin" else {}))
    print(format_report(rep, args.method))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rep, f, indent=2)
    if args.track:
        n = min(t[0].shape[-1] for t in tracks.values())
        rows = [v.reshape(-1, v.shape[-1])[0, :n].float() for k in ("pred", "gt", "lr") if k in tracks for v in tracks[k]]
        with open(args.track, "wb") as f:
            np.save(f, torch.stack(rows).cpu().numpy())
    return rep


if __name__ == "__main__":
    main()
