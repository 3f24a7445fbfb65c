"""Audio -> HR / LR latent pairs and per-channel statistics: the MI355X counterpart of the reference's data preparation
(prepare_dataset_v5.py:120-264) and of its separated statistics (recalculate_stats.py:103-124).

Per file, in the reference's order: mono, divided by its peak only where the peak exceeds 1 (:130-132); 8 s chunks = 7 s valid
plus 0.5 s on each side (:143-168); resample to 48 kHz (:198); LR simulation 48 -> 16 -> 48 kHz (:203-205); both to
44.1 kHz and through the DAC encoder (:207-219); the overlap frames trimmed (:221-232); concatenated and cut to the file's
frame count (:239-245); per-channel sum and sum of squares in fp64 (:251-253).  All arithmetic on audio and latents runs on
the GPU (csrc/resample.hip, csrc/dac_enc.hip).  Differences:
  * one process on one GPU (no worker pool, no file sharding); WAV files only;
  * the 48 -> 44.1 kHz step is the same windowed-sinc kernel with width 24 / rolloff 0.945, a same-family approximation of
    the reference's audiotools (julius) call there;
  * the statistics are kept separately for HR and LR (2048 channels: HR first, then LR), over the fp16-rounded values that
    the latent files hold;
  * the encoder runs in the codec's precision (bf16x3 by default), not under fp16 autocast;
  * consecutive chunks are batched only where their lengths are equal (the reference pads a batch to its first chunk);
  * `--f0` also stores a pitch track of the HR recording, one value per latent frame (jatsr_amd.pitch: YIN at the codec's
    44.1 kHz with hop 512 over the whole file, so frame t is centred on the first sample of latent frame t): `hr_f0` fp32 [T]
    and `hr_voiced` uint8 [T] beside the latents.  Without the flag the files are what they were.  `--f0-method pyin` takes
    the track with pYIN (f0 quantised to 10-cent bins, 0 where unvoiced) and also stores `hr_voiced_prob` fp32 [T].
  * `--f0 --harmonics H` also stores `hr_harmonics` fp16 [T, H]: the amplitudes of the first H harmonics of that track in the
    HR recording (jatsr_amd.harmonic.analyze at the stored `hr_f0` / `hr_voiced`), 0 where the track does not reach.  With
    `--f0-method pyin` the table is taken at the refined track (YIN's f0 within 50 cents of pYIN's bin), not at the quantised
    `hr_f0`.

    python -m jatsr_amd.prepare --source-dir wavs --output-dir data --dac-weights dac.pth
"""
from __future__ import annotations

import argparse
import json
import math
import os
import random

HIGH_SR = 48000
CHUNK_SECONDS, OVERLAP_SECONDS, MIN_SECONDS = 7.0, 0.5, 1.0


def chunk_bounds(total_samples: int, sr: int, chunk: float = CHUNK_SECONDS, overlap: float = OVERLAP_SECONDS):
    """The reference's chunk list (prepare_dataset_v5.py:143-168) with its int() truncations:
    [(idx_start, idx_end, pad_left, pad_right)]; [] for a file shorter than 1 s (:137-139).  Pure host code."""
    duration = total_samples / sr
    if duration < MIN_SECONDS:
        return []
    out = []
    for i in range(math.ceil(duration / chunk)):
        t_start = i * chunk - overlap
        t_end = t_start + chunk + (2 * overlap)
        a, b = int(t_start * sr), int(t_end * sr)
        pad_left = pad_right = 0
        if a < 0:
            pad_left, a = -a, 0
        if b > total_samples:
            pad_right, b = b - total_samples, total_samples
        out.append((a, b, pad_left, pad_right))
    return out


class _Clock:
    """Device-event brackets of the three stages, only when the caller asks for timings."""

    def __init__(self, sink):
        self.sink = sink

    def run(self, name, fn):
        if self.sink is None:
            return fn()
        import torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        self.sink[name] = self.sink.get(name, 0.0) + e0.elapsed_time(e1)
        return out


def to_codec_rate(x, codec):
    """48 kHz audio -> the codec's 44.1 kHz (the `signal.resample(dac_model.sample_rate)` of prepare_dataset_v5.py:211)."""
    from .resample import CODEC_LOWPASS_WIDTH, CODEC_ROLLOFF, resample
    return resample(x, HIGH_SR, codec.sample_rate, CODEC_LOWPASS_WIDTH, CODEC_ROLLOFF)


def hr_codec_signal(x, sr: int, codec):
    """The peak-normalised mono recording x [L] at `sr` -> the whole recording at the codec's rate [L'], as the tracks and the
    harmonic table read it"""
    from .resample import resample
    hr48 = resample(x[None], sr, HIGH_SR) if sr != HIGH_SR else x[None]
    return to_codec_rate(hr48, codec)[0].contiguous()


def hr_pitch_track(x, sr: int, codec, frames: int, method: str = "yin", signal=None):
    """The peak-normalised mono recording x [L] at `sr` -> (hr_f0 fp32 [frames], hr_voiced uint8 [frames]) on the GPU: YIN
    (jatsr_amd.pitch defaults, hop 512) on the whole recording at the codec's rate, cut to the latent frame count; frames the
    track does not reach are f0 = 0 and unvoiced.  method "pyin": the pYIN track instead, and a third value, hr_voiced_prob
    fp32 [frames] (0 where the track does not reach).  `signal`: hr_codec_signal(x, sr, codec) where the caller has it."""
    import torch

    from .pitch import pyin, yin
    if method not in ("yin", "pyin"):
        raise ValueError(f"prepare: f0 method must be 'yin' or 'pyin', got {method!r}")
    y = hr_codec_signal(x, sr, codec) if signal is None else signal
    f0, voiced, third = (yin if method == "yin" else pyin)(y, sr=codec.sample_rate, hop_length=512)
    n = min(frames, f0.shape[0])
    hr_f0 = torch.zeros(frames, dtype=torch.float32, device=f0.device)
    hr_voiced = torch.zeros(frames, dtype=torch.uint8, device=f0.device)
    hr_f0[:n], hr_voiced[:n] = f0[:n], voiced[:n].view(torch.uint8)
    if method == "yin":
        return hr_f0, hr_voiced
    hr_prob = torch.zeros(frames, dtype=torch.float32, device=f0.device)
    hr_prob[:n] = third[:n]
    return hr_f0, hr_voiced, hr_prob


def hr_harmonic_table(signal, codec, hr_f0, hr_voiced, n_harmonics: int, method: str = "yin"):
    """hr_codec_signal's recording and the track of hr_pitch_track [frames] -> hr_harmonics fp16 [frames, n_harmonics] on the
    GPU: the harmonic amplitudes (jatsr_amd.harmonic.analyze, hop 512 at the codec's rate) at that track; rows the recording
    does not reach are 0.  method "pyin": the stored hr_f0 is quantised to 10-cent bins, which misplaces high harmonics by more
    than a bin, so the table is taken at the refined track of jatsr_amd.harmonic (refine_f0: YIN's f0 of the same frame where it
    lies within 50 cents of the bin); hr_f0 itself stays pYIN's."""
    import torch

    from .harmonic import analyze, refine_f0
    y = signal
    frames, have = hr_f0.shape[0], 1 + y.shape[0] // 512
    f0 = torch.zeros(have, dtype=torch.float32, device=y.device)
    voiced = torch.zeros(have, dtype=torch.uint8, device=y.device)
    n = min(frames, have)
    f0[:n], voiced[:n] = hr_f0[:n], hr_voiced[:n]
    if method == "pyin":
        from .pitch import yin
        f0 = refine_f0(f0, voiced, yin(y, sr=codec.sample_rate, hop_length=512)[0])
    amp, _ = analyze(y, f0, voiced, n_harmonics=n_harmonics, sr=codec.sample_rate, hop_length=512)
    out = torch.zeros(frames, amp.shape[1], dtype=torch.float16, device=y.device)
    out[:n] = amp[:n].to(torch.float16)
    return out


def prepare_audio(audio, sr: int, codec, low_sr: int = 16000, batch: int = 8, device="cuda", timings: dict | None = None,
                  f0: bool = False, f0_method: str = "yin", harmonics: int = 0, lr_filter: dict | None = None):
    """One recording -> dict(hr_latent fp32 [1024, T], lr_latent, sum fp64 [2048], sq_sum, count, metadata), tensors on the
    GPU; None for a recording shorter than 1 s.  `audio`: [L] or [channels, L], array or tensor; `codec`: a DacCodec with an
    encoder.  sum / sq_sum: HR channels first, then LR, over the values rounded to fp16; count: T (frames of each).
    With `f0` also hr_f0 fp32 [T] and hr_voiced uint8 [T] (hr_pitch_track), and with f0_method "pyin" hr_voiced_prob fp32 [T];
    with `f0` and `harmonics` = H > 0 also hr_harmonics fp16 [T, H] (hr_harmonic_table).
    `lr_filter` = {"kind": "butter" | "cheby1", "order", "cutoff_hz"[, "ripple_db"]}: the LR half is made with that zero-phase
    IIR low-pass at 48 kHz (jatsr_amd.lowpass) in the place of the round trip through `low_sr`, and the result holds `lr_filter`;
    None or {"kind": "sinc"}: the round trip."""
    import torch

    from . import _lib as L
    from .resample import channel_stats, resample, simulate_lr
    L.require_gpu()
    if int(sr) != sr or sr < 1 or int(low_sr) != low_sr or low_sr < 1:
        raise ValueError(f"prepare_audio: sample rates must be positive integers, got {sr!r}, {low_sr!r}")
    if batch < 1:
        raise ValueError(f"prepare_audio: batch {batch} must be >= 1")
    if harmonics and not f0:
        raise ValueError("prepare_audio: harmonics needs f0 (the table is taken at the stored track)")
    sr, low_sr = int(sr), int(low_sr)
    iir = lr_filter if lr_filter is not None and lr_filter.get("kind") != "sinc" else None
    if iir is not None:
        from .lowpass import check_filter, simulate_lr_filtered
        iir = {"kind": iir["kind"], "order": int(iir["order"]), "cutoff_hz": float(iir["cutoff_hz"]),
               "ripple_db": float(iir.get("ripple_db", 1.0))}
        check_filter(iir["kind"], iir["order"], iir["cutoff_hz"], HIGH_SR, iir["ripple_db"])
    x = torch.as_tensor(audio)
    if not x.is_cuda:
        x = x.to(device)
    x = x.to(torch.float32)
    if x.dim() == 2:
        x = x.mean(dim=0)                                   # :130
    if x.dim() != 1:
        raise ValueError(f"prepare_audio: audio must be [L] or [channels, L], got {tuple(x.shape)}")
    total = x.shape[0]
    duration = total / sr
    bounds = chunk_bounds(total, sr)
    if not bounds:
        return None
    peak = float(x.abs().max())
    if peak > 1.0:                                          # :131-132
        x = x / peak
    chunks = [torch.nn.functional.pad(x[a:b], (pl, pr)) if pl or pr else x[a:b] for a, b, pl, pr in bounds]
    clock = _Clock(timings)
    hr_parts, lr_parts = [], []
    hop48 = trim = valid = None
    i = 0
    while i < len(chunks):
        j = i + 1
        while j < len(chunks) and j - i < batch and chunks[j].shape[0] == chunks[i].shape[0]:
            j += 1
        raw = torch.stack(chunks[i:j])
        i = j

        def both(raw=raw):
            hr = resample(raw, sr, HIGH_SR) if sr != HIGH_SR else raw                    # :197-200
            lr = simulate_lr(hr, HIGH_SR, low_sr) if iir is None else simulate_lr_filtered(hr, HIGH_SR, iir)   # :203-205
            return hr, to_codec_rate(hr, codec), to_codec_rate(lr, codec)
        hr48, hr44, lr44 = clock.run("resample", both)
        z_hr, z_lr = clock.run("encode", lambda: (codec.encode(hr44[:, None])[0], codec.encode(lr44[:, None])[0]))
        if hop48 is None:                                                                 # :222-227
            hop48 = hr48.shape[-1] / z_hr.shape[-1]
            trim = int(int(OVERLAP_SECONDS * HIGH_SR) / hop48)
            valid = int(int(CHUNK_SECONDS * HIGH_SR) / hop48)
        hr_parts.extend(z_hr[..., trim:trim + valid])                                     # :230-235
        lr_parts.extend(z_lr[..., trim:trim + valid])
    frames = int(int(duration * HIGH_SR) / hop48)                                         # :242-245
    hr = torch.cat(hr_parts, dim=-1)[..., :frames].contiguous()
    lr = torch.cat(lr_parts, dim=-1)[..., :frames].contiguous()
    C = hr.shape[0]
    s = torch.zeros(2 * C, dtype=torch.float64, device=hr.device)
    q = torch.zeros(2 * C, dtype=torch.float64, device=hr.device)

    def stats():
        channel_stats(hr, s[:C], q[:C])
        channel_stats(lr, s[C:], q[C:])
    clock.run("stats", stats)
    out = {"hr_latent": hr, "lr_latent": lr, "sum": s, "sq_sum": q, "count": hr.shape[-1],
           "metadata": {"duration": duration, "sr": sr, "chunks": len(chunks), "frames": hr.shape[-1],
                        "hop_48k": hop48, "trim_frames": trim, "valid_frames": valid}}
    if lr_filter is not None:
        out["lr_filter"] = iir if iir is not None else {"kind": "sinc", "low_sr": low_sr}
    sig_kw = {"signal": hr_codec_signal(x, sr, codec)} if f0 and harmonics else {}     # resampled once for the track and the table
    if f0 and f0_method == "yin":
        out["hr_f0"], out["hr_voiced"] = clock.run("f0", lambda: hr_pitch_track(x, sr, codec, hr.shape[-1], **sig_kw))
    elif f0:
        out["hr_f0"], out["hr_voiced"], out["hr_voiced_prob"] = clock.run(
            "f0", lambda: hr_pitch_track(x, sr, codec, hr.shape[-1], f0_method, **sig_kw))
    if f0 and harmonics:
        out["hr_harmonics"] = clock.run("harmonics", lambda: hr_harmonic_table(sig_kw["signal"], codec, out["hr_f0"],
                                                                               out["hr_voiced"], harmonics, f0_method))
    return out


def final_stats(sum_, sq_sum, count, channels: int = 1024) -> dict:
    """Running totals (HR first, then LR) -> hr_mean / hr_std / lr_mean / lr_std lists with std = sqrt(clamp(var, 1e-6))
    (recalculate_stats.py:103-121)."""
    import torch
    mean = sum_.double().cpu() / float(count)
    var = sq_sum.double().cpu() / float(count) - mean ** 2
    std = torch.sqrt(torch.clamp(var, min=1e-6))
    return {"hr_mean": mean[:channels].float().tolist(), "hr_std": std[:channels].float().tolist(),
            "lr_mean": mean[channels:].float().tolist(), "lr_std": std[channels:].float().tolist(),
            "hr_total_frames": int(count), "lr_total_frames": int(count),
            "note": "HR and LR statistics are separated"}


def build_parser():
    p = argparse.ArgumentParser(description="WAV folders -> HR/LR DAC latent pairs and normalisation statistics on MI355X")
    p.add_argument("--source-dir", action="append", required=True, help="folder of *.wav files (searched recursively); repeatable")
    p.add_argument("--output-dir", required=True, help="receives train/, val/, running_stats.pt, global_stats_separated.json")
    p.add_argument("--dac-weights", required=True, help="DAC 44.1 kHz weight file with encoder and quantizer weights")
    p.add_argument("--val-fraction", type=float, default=0.05, help="share of the files that goes to val/")
    p.add_argument("--seed", type=int, default=42, help="seed of the train / val shuffle")
    p.add_argument("--low-sr", type=int, default=16000, help="sample rate of the simulated low-resolution audio")
    p.add_argument("--dac-precision", default="bf16x3", choices=["bf16x3", "bf16"], help="DAC encoder arithmetic")
    p.add_argument("--batch", type=int, default=8, help="chunks per resampler / encoder call")
    p.add_argument("--f0", action="store_true",
                   help="also store hr_f0 / hr_voiced: a YIN pitch track of the HR recording, one value per latent frame")
    p.add_argument("--f0-method", choices=("yin", "pyin"), default="yin",
                   help="with --f0: the tracker; pyin also stores hr_voiced_prob fp32 [T]")
    p.add_argument("--harmonics", type=int, default=0, metavar="H",
                   help="with --f0: also store hr_harmonics fp16 [T, H], the amplitudes of the track's first H harmonics (1..128)")
    p.add_argument("--lr-filter", choices=("sinc", "butter", "cheby1", "mix"), default="sinc",
                   help="how the LR half is made: sinc (the round trip through --low-sr), or one zero-phase IIR low-pass per "
                        "recording at 48 kHz, drawn from (--lr-seed, the file's stem); mix draws among the three kinds")
    p.add_argument("--lr-cutoff-hz", type=str, default=None, metavar="LO,HI",
                   help="with --lr-filter butter / cheby1 / mix: the cutoff is drawn log-uniformly from LO..HI Hz (default 4000,12000)")
    p.add_argument("--lr-order", type=str, default=None, metavar="LO,HI",
                   help="with --lr-filter butter / cheby1 / mix: the order is drawn uniformly from LO..HI, within 1..10 (default 4,10)")
    p.add_argument("--lr-ripple-db", type=float, default=None, metavar="D",
                   help="with --lr-filter cheby1 / mix: the Chebyshev passband ripple in dB, (0, 3] (default 1)")
    p.add_argument("--lr-seed", type=int, default=None, help="with --lr-filter butter / cheby1 / mix: seed of the draw (default --seed)")
    p.add_argument("--device", default="cuda", help="an AMD GPU; there is no CPU path")
    return p


LR_KINDS = {"butter": ("butter",), "cheby1": ("cheby1",), "mix": ("sinc", "butter", "cheby1")}


def lr_filter_plan(args):
    """--lr-filter and its companions -> None (sinc: today's path) or the keyword arguments of lowpass.random_filter; refuses
    the combinations that mean nothing"""
    kind = getattr(args, "lr_filter", "sinc") or "sinc"
    given = {k: getattr(args, "lr_" + k, None) for k in ("cutoff_hz", "order", "ripple_db", "seed")}
    if kind == "sinc":
        extra = [k for k, v in given.items() if v is not None]
        if extra:
            raise SystemExit("--lr-" + extra[0].replace("_", "-") + " means nothing with --lr-filter sinc")
        return None
    if given["ripple_db"] is not None and kind == "butter":
        raise SystemExit("--lr-ripple-db means nothing with --lr-filter butter")
    from .lowpass import JatError, check_filter, parse_range
    cutoff = parse_range(given["cutoff_hz"] or "4000,12000", "--lr-cutoff-hz", float)
    order = parse_range(given["order"] or "4,10", "--lr-order", int)
    ripple = 1.0 if given["ripple_db"] is None else given["ripple_db"]
    if cutoff[0] > cutoff[1] or order[0] > order[1]:
        raise SystemExit("--lr-cutoff-hz and --lr-order: LO must not exceed HI")
    try:
        for c in cutoff:
            for o in order:
                check_filter("cheby1", o, c, HIGH_SR, ripple)
    except JatError as e:
        raise SystemExit(f"--lr-filter: {e}")
    return {"seed": args.seed if given["seed"] is None else given["seed"], "kinds": LR_KINDS[kind], "cutoff_hz": cutoff,
            "order": order, "ripple_db": ripple}


def find_wavs(dirs):
    files = []
    for d in dirs:
        for dp, _, names in sorted(os.walk(d)):
            files.extend(os.path.join(dp, f) for f in sorted(names) if f.lower().endswith(".wav"))
    return files


def run(args):
    import torch

    from . import io as jio
    from .dac import load_dac_codec
    files = find_wavs(args.source_dir)
    random.Random(args.seed).shuffle(files)                 # :301-305
    split = int(len(files) * (1 - args.val_fraction))
    tasks = [(f, "train") for f in files[:split]] + [(f, "val") for f in files[split:]]
    for sub in ("train", "val"):
        os.makedirs(os.path.join(args.output_dir, sub), exist_ok=True)
    stats_path = os.path.join(args.output_dir, "running_stats.pt")
    if os.path.exists(stats_path):
        st = torch.load(stats_path, map_location="cpu", weights_only=False)
        total_sum, total_sq, total_count = st["sum"].double(), st["sq_sum"].double(), int(st["count"])
    else:
        total_sum = total_sq = None
        total_count = 0
    codec = None
    lr_plan = lr_filter_plan(args)
    report = {"written": [], "skipped": [], "existing": []}
    if lr_plan is not None:
        report["lr_filters"] = {}
    for path, sub in tasks:
        stem = os.path.splitext(os.path.basename(path))[0]
        out_path = os.path.join(args.output_dir, sub, f"{stem}.pt")
        # a file added to the sources later can move others across the split: what either folder holds already stays there
        if any(os.path.exists(os.path.join(args.output_dir, d, f"{stem}.pt")) for d in ("train", "val")):
            report["existing"].append(path)
            continue
        if codec is None:
            codec = load_dac_codec(args.dac_weights, device=args.device, precision=args.dac_precision)
        x, sr = jio.read_wav(path)
        want_f0 = getattr(args, "f0", False)
        f0_method = getattr(args, "f0_method", "yin")
        harmonics = getattr(args, "harmonics", 0)
        if harmonics and not want_f0:
            raise SystemExit("--harmonics needs --f0")
        lr_kw = {}
        if lr_plan is not None:
            from .lowpass import random_filter
            lr_kw = {"lr_filter": random_filter(lr_plan["seed"], stem, lr_plan["kinds"], lr_plan["cutoff_hz"], lr_plan["order"],
                                                lr_plan["ripple_db"])}
        res = prepare_audio(x, sr, codec, low_sr=args.low_sr, batch=args.batch, device=args.device, f0=want_f0, **lr_kw,
                            **({"f0_method": f0_method} if f0_method != "yin" else {}),
                            **({"harmonics": harmonics} if harmonics else {}))
        if res is None:
            print(f"skipped {path}: shorter than {MIN_SECONDS:g} s")
            report["skipped"].append(path)
            continue
        jio.save_latent_file(out_path, hr_latent=res["hr_latent"], lr_latent=res["lr_latent"],
                             metadata={"name": stem, "path": path, "duration": res["metadata"]["duration"], "sr": sr},
                             **({"lr_filter": res["lr_filter"]} if "lr_filter" in res else {}),
                             **({k: res[k].cpu() for k in ("hr_f0", "hr_voiced", "hr_voiced_prob", "hr_harmonics") if k in res} if want_f0 else {}))
        s, q = res["sum"].cpu(), res["sq_sum"].cpu()
        total_sum = s if total_sum is None else total_sum + s
        total_sq = q if total_sq is None else total_sq + q
        total_count += res["count"]
        torch.save({"sum": total_sum, "sq_sum": total_sq, "count": total_count}, stats_path)
        report["written"].append(out_path)
        if "lr_filter" in res:
            kinds = report["lr_filters"]
            kinds[res["lr_filter"]["kind"]] = kinds.get(res["lr_filter"]["kind"], 0) + 1
        print(f"{path} -> {out_path}: {res['count']} frames" + (f", LR through {res['lr_filter']}" if "lr_filter" in res else ""))
    if total_count > 0:
        with open(os.path.join(args.output_dir, "global_stats_separated.json"), "w") as f:
            json.dump(final_stats(total_sum, total_sq, total_count, total_sum.numel() // 2), f, indent=4)
    print(f"prepared {len(report['written'])} file(s), skipped {len(report['skipped'])}, "
          f"{len(report['existing'])} already present; {total_count} frames in the statistics" +
          (f"; LR filters {report['lr_filters']}" if lr_plan is not None else ""))
    return report


def main(argv=None):
    return run(build_parser().parse_args(argv))


if __name__ == "__main__":
    main()
