"""Inference driver — the MI355X counterpart of reference `infer_test_v3m2.py:main` (:236-450).

Same flags (`--checkpoint --val-dir --stats-file --output-dir --steps --cfg-scale --total-seconds --device
--input-file`), same chunk plan (16 s chunks = 1378 latent frames, 2 s = 172-frame linear crossfade, :340-404), same
per-channel normalisation (:381-394).  Differences, all outside the hot path's semantics:
  * equal-length chunks are batched into one captured sampler launch instead of the reference's serial B=1 loop;
  * the generated / HR / LR latents are always written as a `.pt` file in the reference's latent container format;
    with `--dac-weights PATH` (a DAC 44.1 kHz weight file: there is no download) they are also decoded on the GPU
    (jatsr_amd.dac, csrc/dac.hip) and written as the reference's three 44.1 kHz WAV files (:408-437);
    `--dac-precision` picks bf16x3 (default, fp32-accurate) or bf16;
  * `--input-audio PATH.wav` (44.1 kHz, with `--dac-weights`) starts from audio: the WAV is DAC-encoded on the GPU
    (csrc/dac_enc.hip) and its latent is the LR input; there is no HR latent;
  * `--seed` makes the initial noise reproducible (the reference draws it with torch.randn, :133);
  * `--metrics` (with `--dac-weights`, where an HR ground truth exists: `--simulate-lr`, or a latent file with `hr_latent`)
    evaluates the decoded generated / HR / LR audio as the reference's calculate_metrics.py does (jatsr_amd.metrics) and
    writes `{stem}_metrics.json` (with the `_cfgX` suffix of the generated files, if any) next to the WAVs;
  * `--f0-metrics` (valid where `--metrics` is) adds an `"f0"` entry to that JSON: how far the YIN pitch tracks of the decoded
    generated and LR audio agree with the HR audio's (jatsr_amd.pitch); without `--metrics` the JSON holds that entry alone;
    `--f0-method pyin` takes the tracks with pYIN instead and records `"method": "pyin"` inside that entry;
  * `--harmonic-metrics` (valid where `--metrics` is) adds a `"harmonic"` entry to that JSON: the amplitudes of the harmonics of
    the HR audio's pitch track in the decoded generated and LR audio against the HR audio's, split at the LR audio's detected
    band limit into kept and regenerated harmonics (jatsr_amd.harmonic); the track is taken with `--f0-method`;
  * `--lf-replace [HZ]` (with `--dac-weights`) also writes `{stem}_generated{suffix}_lf.wav`: the decoded audio with its
    band below HZ (bare flag: the detected band limit of the source) replaced by the source's own (jatsr_amd.splice,
    csrc/splice.hip).  The source is the 44.1 kHz waveform that was encoded (`--input-audio`), the whole file taken through
    the LR simulation (`--simulate-lr`), or the decoded LR latent (latent-file input).  Every other file is unchanged.
  * `--index-bank PATH --index-rate R` also writes `{stem}_generated{suffix}_idx.pt` (and, with `--dac-weights`,
    `{stem}_generated{suffix}_idx.wav`): the generated latent with R of each frame's nearest neighbour in a latent bank
    (`python -m jatsr_amd.retrieval build`) mixed in (jatsr_amd.retrieval, csrc/retrieval.hip).  `--index-k K` (1..8,
    default 1) mixes in the inverse-square-distance weighted mean of the K nearest frames instead; the file's metadata
    records `index_k`, and for K > 1 the file also holds `idx` and `dist2` [frames, K].  Every other file is unchanged.
    A multi-scale bank file (`retrieval build --scales 1,2,4`) needs no switch: `--index-bank` loads either
    format, `--index-scale-weights W1,W2,...` replaces the stored scale weights, and the metadata gains `index_scales` and
    `index_scale_weights` (for K > 1 the lists are `idx_s{scale}` / `dist2_s{scale}`, one pair per scale).
  * `--index-protect P`, `--index-unstable U`, `--index-smooth S` (any of them, with `--index-bank`) make the index
    rate a per-frame track: the pitch track of the LR input at the codec's rate (hop 512, `--index-f0-method yin|pyin`; the LR
    waveform itself with `--input-audio`, else the DAC-decoded LR latent, which needs `--dac-weights`) is classed frame by frame
    as not live / unstable / stable, and those frames get R * P, R * U and R of the retrieved frame, averaged over S frames
    on either side (defaults 1, 1, 2).  The `_idx.pt` file gains `rates` and `f0_classes` [frames] and its metadata the four
    settings, `voiced_share` and `stable_share`.  Without these flags every file is what it was.

    python -m jatsr_amd.infer --checkpoint ckpt.pt --input-file clip.pt --stats-file stats.json --cfg-scale 3.0
"""
from __future__ import annotations

import argparse
import os
import time

import torch

from . import io as jio
from .model import JaT_AudioSR_V2, JaT_AudioSR_V3, load_model
from .retrieval import index_k_arg, index_rate_arg, nprobe_arg, protect_arg, scale_weights_arg, smooth_arg, unstable_arg
from .sampler import chunk_plan, sample_long


def build_parser():
    p = argparse.ArgumentParser(description="JaT-AudioSR V3 inference on MI355X (latent in, latent out)")
    p.add_argument("--checkpoint", type=str, default="checkpoints/v3_full_run/last.pt", help="V3 checkpoint path")
    p.add_argument("--val-dir", type=str, default="data_processed_v13_final/val", help="Validation latents directory")
    p.add_argument("--stats-file", type=str, default="data_processed_v13_final/global_stats_separated.json",
                   help="Normalization stats file (JSON or PT)")
    p.add_argument("--output-dir", type=str, default="inference_output_v3", help="Output directory")
    p.add_argument("--steps", type=int, default=50, help="Number of sampling steps")
    p.add_argument("--solver", type=str, default="euler", choices=["euler", "midpoint", "heun"],
                   help="integration rule: euler (the reference's step), midpoint or heun (two model evaluations per step)")
    p.add_argument("--cfg-scale", type=float, default=1.0, help="CFG guidance scale (1.0 = no CFG)")
    p.add_argument("--total-seconds", type=float, default=None, help="Total output duration in seconds")
    p.add_argument("--device", type=str, default="cuda", help="Device (an AMD GPU; there is no CPU path)")
    p.add_argument("--input-file", type=str, default=None, help="Specific input file; default: first file in val-dir")
    p.add_argument("--layernorm", action="store_true", help="checkpoint is a v3mod2 (LayerNorm, JaT_AudioSR_V2) model")
    p.add_argument("--seed", type=int, default=None, help="seed for the initial noise")
    p.add_argument("--ema", action="store_true",
                   help="sample from the checkpoint's moving average of the weights (written by fit --ema-decay) instead of the "
                        "last iterate")
    p.add_argument("--dac-weights", type=str, default=None,
                   help="DAC 44.1 kHz weight file (.safetensors/.pt/.bin/.pth); decode to WAV when given")
    p.add_argument("--dac-precision", type=str, default="bf16x3", choices=["bf16x3", "bf16"],
                   help="DAC decoder arithmetic: bf16x3 (three-pass split, fp32-accurate) or bf16")
    p.add_argument("--input-audio", type=str, default=None,
                   help="44.1 kHz WAV to super-resolve: DAC-encoded on the GPU as the LR latent (needs --dac-weights; "
                        "not with --input-file)")
    p.add_argument("--resample", action="store_true",
                   help="with --input-audio: convert a WAV of any sample rate to 44.1 kHz on the GPU before the encode")
    p.add_argument("--simulate-lr", type=int, nargs="?", const=16000, default=None, metavar="LOW_SR",
                   help="with --input-audio: the WAV is the HR recording; its LR latent (through LOW_SR, default 16000) "
                        "is the sampler's input, made as the training data is (implies --resample)")
    p.add_argument("--lr-filter", choices=("butter", "cheby1"), default=None,
                   help="with --simulate-lr: make the LR input with one zero-phase IIR low-pass at 48 kHz (jatsr_amd.lowpass) in "
                        "place of the resampling round trip; needs --lr-cutoff-hz")
    p.add_argument("--lr-cutoff-hz", type=float, default=None, metavar="HZ", help="with --lr-filter: the cutoff, 1000..23520 Hz")
    p.add_argument("--lr-order", type=int, default=None, metavar="N", help="with --lr-filter: the order, 1..10 (default 8)")
    p.add_argument("--lr-ripple-db", type=float, default=None, metavar="D",
                   help="with --lr-filter cheby1: the passband ripple in dB, (0, 3] (default 1)")
    p.add_argument("--metrics", action="store_true",
                   help="LSD and mel losses of the decoded generated and LR audio against the HR ground truth, written as "
                        "{stem}_metrics.json (needs --dac-weights and a ground truth: --simulate-lr or a latent file with hr_latent)")
    p.add_argument("--f0-metrics", action="store_true",
                   help="YIN pitch tracks of the decoded generated and LR audio against the HR ground truth's: an \"f0\" entry in "
                        "{stem}_metrics.json (valid where --metrics is; jatsr_amd.pitch)")
    p.add_argument("--f0-method", choices=("yin", "pyin"), default="yin",
                   help="with --f0-metrics: the tracker; pyin adds \"method\": \"pyin\" to the \"f0\" entry")
    p.add_argument("--harmonic-metrics", action="store_true",
                   help="harmonic amplitudes of the decoded generated and LR audio at the HR ground truth's pitch track, below and "
                        "above the LR audio's band limit: a \"harmonic\" entry in {stem}_metrics.json (valid where --metrics is; "
                        "jatsr_amd.harmonic)")
    p.add_argument("--lf-replace", type=str, nargs="?", const="auto", default=None, metavar="HZ",
                   help="also write {stem}_generated_lf.wav: the decoded audio with the band below HZ (bare flag: the "
                        "detected band limit of the source) taken from the source waveform (needs --dac-weights).  With a "
                        "latent-file input the source is the decoded LR latent: that only removes generator drift, not "
                        "codec error")
    p.add_argument("--lf-transition-hz", type=float, default=500.0,
                   help="with --lf-replace: width of the crossfade in frequency, below the cutoff")
    p.add_argument("--index-bank", type=str, default=None, metavar="PATH",
                   help="latent bank file (python -m jatsr_amd.retrieval build); also write {stem}_generated_idx.pt, the "
                        "generated latent blended with each frame's nearest bank frame")
    p.add_argument("--index-rate", type=index_rate_arg, default=0.4, metavar="R",
                   help="with --index-bank: share of the retrieved frame in the blend, in [0, 1] (0.3 to 0.6 are usual)")
    p.add_argument("--index-k", type=index_k_arg, default=1, metavar="K",
                   help="with --index-bank: blend in the inverse-square-distance weighted mean of each frame's K nearest bank "
                        "frames, 1..8 (1: the single nearest frame; RVC's index uses 8)")
    p.add_argument("--index-scale-weights", type=scale_weights_arg, default=None, metavar="W1,W2,...",
                   help="with a multi-scale --index-bank (retrieval build --scales): the share of each scale's track, one "
                        "positive number per scale, normalised to sum 1 (default: the weights stored in the bank file)")
    p.add_argument("--index-nprobe", type=nprobe_arg, default=None, metavar="P",
                   help="with an IVF --index-bank (retrieval build --ivf): the lists a search scans, 1..8 (default: the "
                        "number stored in the bank file)")
    p.add_argument("--index-protect", type=protect_arg, default=None, metavar="P",
                   help="with --index-bank: frames without a pitch (consonants, breaths, noise) get R * P of the retrieved "
                        "frame in place of R, P in [0, 1] (default 1: no effect).  This is the plain factor: RVC's slider of "
                        "the same name means \"off\" at 0.5 and defaults to 0.33.  Makes the index rate a per-frame track")
    p.add_argument("--index-unstable", type=unstable_arg, default=None, metavar="U",
                   help="with --index-bank: voiced frames whose F0 is not steady (fewer than 7 of the 9 frames around them within "
                        "50 cents) get R * U, U in [0, 1] (default 1: no effect).  Makes the index rate a per-frame track")
    p.add_argument("--index-smooth", type=smooth_arg, default=None, metavar="S",
                   help="with --index-bank: the per-frame rate is averaged over S frames on either side, 0..16 (default 2).  "
                        "Makes the index rate a per-frame track")
    p.add_argument("--index-f0-method", choices=("yin", "pyin"), default=None,
                   help="with --index-protect / --index-unstable / --index-smooth: the tracker of the LR input's pitch (default yin)")
    return p


RATE_FLAGS = ("index_protect", "index_unstable", "index_smooth")


def rate_flags(args):
    """Whether the index rate is a per-frame track: any of --index-protect, --index-unstable, --index-smooth was given."""
    return any(getattr(args, name, None) is not None for name in RATE_FLAGS)


def lr_filter_of(args):
    """--lr-filter and its companions -> {"kind", "order", "cutoff_hz", "ripple_db"}, or None when none of them was given"""
    kind, cutoff = getattr(args, "lr_filter", None), getattr(args, "lr_cutoff_hz", None)
    order, ripple = getattr(args, "lr_order", None), getattr(args, "lr_ripple_db", None)
    if kind is None:
        if cutoff is not None or order is not None or ripple is not None:
            raise SystemExit("--lr-cutoff-hz, --lr-order and --lr-ripple-db need --lr-filter")
        return None
    if getattr(args, "simulate_lr", None) is None:
        raise SystemExit("--lr-filter needs --simulate-lr (it replaces the resampling round trip of the simulated LR input)")
    if cutoff is None:
        raise SystemExit("--lr-filter needs --lr-cutoff-hz")
    if ripple is not None and kind != "cheby1":
        raise SystemExit("--lr-ripple-db needs --lr-filter cheby1")
    from .lowpass import JatError, check_filter
    from .prepare import HIGH_SR
    filt = {"kind": kind, "order": 8 if order is None else order, "cutoff_hz": cutoff, "ripple_db": 1.0 if ripple is None else ripple}
    try:
        check_filter(kind, filt["order"], cutoff, HIGH_SR, filt["ripple_db"])
    except JatError as e:
        raise SystemExit(f"--lr-filter: {e}")
    return filt


def run(args):
    lr_filter_of(args)
    if args.lf_replace is not None:
        if not args.dac_weights:
            raise SystemExit("--lf-replace needs --dac-weights")
        if args.lf_replace != "auto":
            try:
                float(args.lf_replace)
            except ValueError:
                raise SystemExit(f"--lf-replace: {args.lf_replace!r} is not a frequency in Hz")
    if args.input_audio and (args.input_file or not args.dac_weights):
        raise SystemExit("--input-audio needs --dac-weights and cannot be combined with --input-file")
    if (args.resample or args.simulate_lr is not None) and not args.input_audio:
        raise SystemExit("--resample and --simulate-lr need --input-audio")
    if args.metrics and (not args.dac_weights or (args.input_audio and args.simulate_lr is None)):
        raise SystemExit("--metrics needs --dac-weights and an HR ground truth (--simulate-lr, or a latent file with hr_latent)")
    f0_metrics = getattr(args, "f0_metrics", False)
    if f0_metrics and (not args.dac_weights or (args.input_audio and args.simulate_lr is None)):
        raise SystemExit("--f0-metrics needs --dac-weights and an HR ground truth (--simulate-lr, or a latent file with hr_latent)")
    harmonic_metrics = getattr(args, "harmonic_metrics", False)
    if harmonic_metrics and (not args.dac_weights or (args.input_audio and args.simulate_lr is None)):
        raise SystemExit("--harmonic-metrics needs --dac-weights and an HR ground truth (--simulate-lr, or a latent file with hr_latent)")
    index_bank = getattr(args, "index_bank", None)
    index_rate = index_rate_arg(getattr(args, "index_rate", 0.4)) if index_bank else 0.0
    index_k = index_k_arg(getattr(args, "index_k", 1)) if index_bank else 1
    index_track = rate_flags(args)
    if (index_track or getattr(args, "index_f0_method", None) is not None) and not index_bank:
        raise SystemExit("--index-protect, --index-unstable, --index-smooth and --index-f0-method need --index-bank")
    if getattr(args, "index_f0_method", None) is not None and not index_track:
        raise SystemExit("--index-f0-method needs --index-protect, --index-unstable or --index-smooth")
    if index_track and not args.input_audio and not args.dac_weights:
        raise SystemExit("--index-protect, --index-unstable and --index-smooth take the pitch of the LR audio: give "
                         "--input-audio, or --dac-weights to decode the LR latent")
    device = torch.device(args.device)
    os.makedirs(args.output_dir, exist_ok=True)
    model = load_model(args.checkpoint, device=device, cls=JaT_AudioSR_V2 if args.layernorm else JaT_AudioSR_V3,
                       use_ema=args.ema)
    codec = source = None
    if args.input_audio:
        path = args.input_audio
        codec, hr, lr, source = encode_audio(args, device)
    elif args.input_file:
        path = args.input_file if os.path.exists(args.input_file) else os.path.join(args.val_dir, args.input_file)
        if not os.path.exists(path):
            raise FileNotFoundError(f"File not found: {path}")
    else:
        path = jio.first_latent_file(args.val_dir)
    if not args.input_audio:
        hr, lr = jio.load_latent_file(path)
    if args.metrics and hr is None:
        raise SystemExit(f"--metrics: {path} holds no hr_latent, so there is no ground truth to compare with")
    if f0_metrics and hr is None:
        raise SystemExit(f"--f0-metrics: {path} holds no hr_latent, so there is no ground truth to compare with")
    if harmonic_metrics and hr is None:
        raise SystemExit(f"--harmonic-metrics: {path} holds no hr_latent, so there is no ground truth to compare with")
    C = model.input_channels
    stats = jio.load_stats(args.stats_file, channels=C, device=device)

    total = lr.shape[-1]
    if args.total_seconds is not None:
        total = min(total, jio.frames_for_seconds(args.total_seconds))
    chunk_frames, overlap = jio.frames_for_seconds(16.0), jio.frames_for_seconds(2.0)   # 1378, 172
    plan = chunk_plan(total, chunk_frames, overlap)
    print(f"input {os.path.basename(path)}: {total} frames -> {len(plan)} chunk(s) {[b - a for a, b in plan]}, "
          f"steps={args.steps}, cfg_scale={args.cfg_scale}" + (f", solver={args.solver}" if args.solver != "euler" else ""))
    noise = None
    if args.seed is not None:
        g = torch.Generator(device="cpu").manual_seed(args.seed)
        noise = [torch.randn(1, C, b - a, generator=g).to(device) for a, b in plan]
    t0 = time.time()
    gen = sample_long(model, lr[:, :total].to(device), stats["hr_mean"], stats["hr_std"], stats["lr_mean"],
                      stats["lr_std"], num_steps=args.steps, cfg_scale=args.cfg_scale, chunk_frames=chunk_frames,
                      overlap_frames=overlap, noise=noise, solver=args.solver)
    torch.cuda.synchronize()
    dt = time.time() - t0
    stem = os.path.splitext(os.path.basename(path))[0]
    suffix = f"_cfg{args.cfg_scale:.1f}" if args.cfg_scale != 1.0 else ""
    out_path = os.path.join(args.output_dir, f"{stem}_generated{suffix}.pt")
    jio.save_latent_file(out_path, hr_latent=None if hr is None else hr[:, :total], lr_latent=lr[:, :total],
                         generated_latent=gen[0].to("cpu", torch.float16),
                         metadata={"source": os.path.basename(path), "steps": args.steps, "cfg_scale": args.cfg_scale,
                                   "frames": total, "seconds": dt})
    print(f"generated {gen.shape[-1]} frames in {dt:.2f} s -> {out_path}")
    if args.dac_weights:
        codec = decode_to_wav(args, gen, hr, lr, total, stem, suffix, device, codec, source)
    if index_bank:
        from .retrieval import IVFBank, MultiScaleBank, load_bank
        bank = load_bank(index_bank, device=device)            # any format: a LatentBank, a MultiScaleBank or an IVFBank
        multi = isinstance(bank, MultiScaleBank)
        index_nprobe = getattr(args, "index_nprobe", None)
        if index_nprobe is not None:
            if not isinstance(bank, IVFBank):
                raise SystemExit("--index-nprobe needs an IVF bank (retrieval build --ivf)")
            bank.nprobe = nprobe_arg(index_nprobe)
        scale_weights = getattr(args, "index_scale_weights", None)
        if scale_weights is not None:
            if not multi:
                raise SystemExit("--index-scale-weights needs a multi-scale bank (retrieval build --scales)")
            try:
                bank.set_weights(scale_weights)
            except ValueError as e:
                raise SystemExit(f"--index-scale-weights: {e}")
        query = lr[None, :, :total].to(device).float() if bank.key == "lr" else None
        lists, extra, track = {}, {}, {}
        rate = index_rate
        if index_track:
            if source is None:                                 # latent-file input: the decoded LR latent
                source = codec.decode(lr[None, :, :total].to(device))[0, 0].float().contiguous()
            rate, cls, track = index_rate_track(args, source, codec.sample_rate, total, index_rate)
            lists.update({"rates": rate.cpu(), "f0_classes": cls.cpu()})
        enhanced, nn_idx, nn_dist2 = bank.retrieve(gen, rate, stats=stats, query=query, k=index_k, neighbours=True)
        idx_path = os.path.join(args.output_dir, f"{stem}_generated{suffix}_idx.pt")
        if multi:                                              # per scale s: idx_s{s}, dist2_s{s} [ceil(frames / s), K]
            extra = {"index_scales": list(bank.scales), "index_scale_weights": list(bank.weights)}
            if index_k > 1:
                for sc, i, d in zip(bank.scales, nn_idx, nn_dist2):
                    lists.update({f"idx_s{sc}": i[0].cpu(), f"dist2_s{sc}": d[0].cpu()})
        elif index_k > 1:
            lists = {"idx": nn_idx[0].cpu(), "dist2": nn_dist2[0].cpu()}                         # [frames, K]
        if isinstance(bank, IVFBank):                          # idx are positions in the grouped bank
            extra = {"index_lists": bank.nlist, "index_nprobe": bank.nprobe}
        jio.save_latent_file(idx_path, generated_latent=enhanced[0].to("cpu", torch.float16),
                             metadata={"source": os.path.basename(path), "index_bank": os.path.basename(index_bank),
                                       "index_rate": index_rate, "index_k": index_k, "bank_rows": len(bank),
                                       "bank_key": bank.key, **extra, **track}, **lists)
        print(f"retrieval: {len(bank)} bank rows (key={bank.key}), index rate {index_rate}" +
              (f", {index_k} nearest frames" if index_k > 1 else "") +
              (f", scales {list(bank.scales)}" if multi else "") +
              (f", {bank.nlist} lists, nprobe {bank.nprobe}" if isinstance(bank, IVFBank) else "") +
              (f", per-frame rate: protect {track['index_protect']}, unstable {track['index_unstable']}, smooth "
               f"{track['index_smooth']} ({track['index_f0_method']}; {track['voiced_share']:.3f} of the frames voiced, "
               f"{track['stable_share']:.3f} stable)" if track else "") + f" -> {idx_path}")
        if args.dac_weights:
            name = f"{stem}_generated{suffix}_idx.wav"
            jio.write_wav_float32(os.path.join(args.output_dir, name), codec.decode(enhanced[:1])[0, 0], codec.sample_rate)
            print(f"decoded the blended latent -> {name}")
    return out_path


def index_rate_track(args, signal, sr, frames, index_rate):
    """The per-frame index rate of --index-protect / --index-unstable / --index-smooth from the LR waveform `signal` fp32 [L]
    on the GPU at the codec's rate: its pitch track (jatsr_amd.pitch defaults, hop 512: one value per latent frame), the
    stability classes, the rate track -> (rates fp32 [frames], classes uint8 [frames], metadata).  Frames behind the end of the
    pitch track are class 0.  The shares are taken over the frames of the pitch track; they carry no speech / music label."""
    from . import pitch
    from .retrieval import f0_classes, rate_track
    protect = 1.0 if getattr(args, "index_protect", None) is None else args.index_protect
    unstable = 1.0 if getattr(args, "index_unstable", None) is None else args.index_unstable
    smooth = 2 if getattr(args, "index_smooth", None) is None else args.index_smooth
    method = getattr(args, "index_f0_method", None) or "yin"
    f0, voiced, _ = (pitch.pyin if method == "pyin" else pitch.yin)(signal, sr=sr, hop_length=512)
    cls, summary = f0_classes(f0, voiced)
    rates = rate_track(cls, frames, index_rate, protect=protect, unstable=unstable, smooth=smooth)
    classes = torch.zeros(frames, dtype=torch.uint8, device=cls.device)
    n = min(frames, cls.shape[0])
    classes[:n] = cls[:n]
    live, stable = (int(v) for v in summary.cpu())
    meta = {"index_protect": protect, "index_unstable": unstable, "index_smooth": smooth, "index_f0_method": method,
            "voiced_share": live / cls.shape[0], "stable_share": stable / cls.shape[0]}
    return rates, classes, meta


def encode_audio(args, device):
    """--input-audio: the WAV's DAC latent (the reference's data preparation, prepare_dataset_v5.py:206-219) becomes the
    LR latent; there is no HR latent.  -> (codec, None, lr fp32 [1024, T] on the CPU, source).  With --resample a WAV of
    another rate is converted to 44.1 kHz first; with --simulate-lr the WAV is the HR recording and both latents come from
    prepare_audio -> (codec, hr, lr, source).  source: with --lf-replace the 44.1 kHz low-resolution waveform fp32 [L] on
    the GPU (also kept for the per-frame index rate), else None."""
    from .dac import load_dac_codec
    x, sr = jio.read_wav(args.input_audio)
    if args.simulate_lr is not None:
        from .prepare import prepare_audio
        codec = load_dac_codec(args.dac_weights, device=device, precision=args.dac_precision)
        filt = lr_filter_of(args)
        res = prepare_audio(x, sr, codec, low_sr=args.simulate_lr, device=device, **({"lr_filter": filt} if filt else {}))
        if res is None:
            raise SystemExit(f"{args.input_audio}: shorter than 1 s")
        print(f"prepared {os.path.basename(args.input_audio)}: {x.shape[0]} samples at {sr} Hz -> {res['count']} frames "
              f"(HR and LR through " + (f"{args.simulate_lr} Hz" if not filt else
                                         f"{filt['kind']} order {filt['order']} at {filt['cutoff_hz']:g} Hz") +
              f", DAC {args.dac_precision})")
        keep = args.lf_replace is not None or rate_flags(args)
        source = simulated_lr_waveform(x, sr, codec, args.simulate_lr, device, **({"lr_filter": filt} if filt else {})) if keep else None
        return codec, res["hr_latent"].cpu(), res["lr_latent"].cpu(), source
    if sr != 44100 and not args.resample:
        raise SystemExit(f"{args.input_audio}: sample rate {sr} Hz; the DAC 44.1 kHz model needs 44100 Hz "
                         "(resampling is not provided unless --resample is given)")
    codec = load_dac_codec(args.dac_weights, device=device, precision=args.dac_precision)
    audio = torch.from_numpy(x).to(device)[None]
    if sr != 44100:
        from .resample import resample
        audio = resample(audio, sr, 44100)
        print(f"resampled {os.path.basename(args.input_audio)}: {sr} Hz -> 44100 Hz, {audio.shape[-1]} samples")
    z = codec.encode(audio[None])[0]
    print(f"encoded {os.path.basename(args.input_audio)}: {x.shape[0]} samples -> {z.shape[-1]} frames "
          f"(DAC {args.dac_precision})")
    keep = args.lf_replace is not None or rate_flags(args)
    return codec, None, z[0].cpu(), audio[0].contiguous() if keep else None


def simulated_lr_waveform(x, sr, codec, low_sr, device, lr_filter=None):
    """The whole recording through the resample calls prepare_audio runs on its chunks (peak rule, -> 48 kHz ->
    simulate_lr -> codec rate): the low-resolution waveform at 44.1 kHz, fp32 [L] on the GPU."""
    from .prepare import HIGH_SR, to_codec_rate
    from .resample import resample, simulate_lr
    w = torch.as_tensor(x).to(device, torch.float32)
    if w.dim() == 2:
        w = w.mean(dim=0)
    peak = float(w.abs().max())
    if peak > 1.0:
        w = w / peak
    hr48 = resample(w[None], sr, HIGH_SR) if sr != HIGH_SR else w[None]
    if lr_filter is not None:
        from .lowpass import simulate_lr_filtered
        return to_codec_rate(simulate_lr_filtered(hr48, HIGH_SR, lr_filter), codec)[0].contiguous()
    return to_codec_rate(simulate_lr(hr48, HIGH_SR, low_sr), codec)[0].contiguous()


def decode_to_wav(args, gen, hr, lr, total, stem, suffix, device, codec=None, source=None):
    """DAC decode of the generated, HR and LR latents and the three WAV files of infer_test_v3m2.py:408-437; with
    --lf-replace also the generated audio with its low band taken from `source` (the decoded LR latent when None)."""
    from .dac import load_dac_codec
    if codec is None:
        codec = load_dac_codec(args.dac_weights, device=device, precision=args.dac_precision)
    outs = [(f"{stem}_generated{suffix}.wav", gen[:1].float())]
    if hr is not None:
        outs.append((f"{stem}_hr_gt.wav", hr[None, :, :total].to(device)))
    outs.append((f"{stem}_lr_input.wav", lr[None, :, :total].to(device)))
    decoded = []
    f0_metrics = getattr(args, "f0_metrics", False)
    harmonic_metrics = getattr(args, "harmonic_metrics", False)
    keep = args.metrics or f0_metrics or harmonic_metrics or args.lf_replace is not None
    for name, z in outs:
        audio = codec.decode(z)                      # [1, 1, frames * 512]
        jio.write_wav_float32(os.path.join(args.output_dir, name), audio[0, 0], codec.sample_rate)
        if keep:
            decoded.append(audio[0, 0].float().contiguous())
    print(f"decoded {len(outs)} latents with DAC ({args.dac_precision}) -> {[n for n, _ in outs]}")
    spliced = None
    if args.lf_replace is not None:
        from .splice import splice_lowband
        spliced, hz = splice_lowband(decoded[0], decoded[-1] if source is None else source,
                                     None if args.lf_replace == "auto" else float(args.lf_replace),
                                     args.lf_transition_hz, sr=codec.sample_rate)
        name = f"{stem}_generated{suffix}_lf.wav"
        jio.write_wav_float32(os.path.join(args.output_dir, name), spliced, codec.sample_rate)
        print(f"low band below {hz:.1f} Hz ({'detected' if args.lf_replace == 'auto' else 'given'}) taken from the "
              f"{'decoded LR latent' if source is None else 'input waveform'} -> {name}")
    if args.metrics or f0_metrics or harmonic_metrics:
        import json

        generated, hr_gt, lr_input = decoded
        rep = {}
        if args.metrics:
            from . import metrics
            rep = metrics.evaluate(generated, hr_gt, lr_input, sr=codec.sample_rate)
            print(metrics.format_report(rep))
            if spliced is not None:
                lf = metrics.evaluate(spliced, hr_gt, sr=codec.sample_rate)
                rep["generated_lf"] = lf["generated"]
                print("low band replaced (generated_lf) vs GT:")
                print(metrics.format_report(lf))
        if f0_metrics:
            from . import pitch
            f0_kw = {"method": "pyin"} if getattr(args, "f0_method", "yin") == "pyin" else {}
            rep["f0"] = pitch.f0_metrics(generated, hr_gt, lr_input, sr=codec.sample_rate, **f0_kw)
            print(pitch.format_report(rep["f0"], **f0_kw))
            if spliced is not None:
                rep["f0"]["generated_lf"] = pitch.f0_metrics(spliced, hr_gt, sr=codec.sample_rate, **f0_kw)["generated"]
            rep["f0"].update(f0_kw)
        if harmonic_metrics:
            from . import harmonic
            rep["harmonic"] = harmonic.harmonic_metrics(generated, hr_gt, lr_input, sr=codec.sample_rate,
                                                        method=getattr(args, "f0_method", "yin"))
            print(harmonic.format_report(rep["harmonic"]))
        out = os.path.join(args.output_dir, f"{stem}_metrics{suffix}.json")
        with open(out, "w") as f:
            json.dump(rep, f, indent=2)
        print(f"metrics -> {out}")
    return codec


def main(argv=None):
    return run(build_parser().parse_args(argv))


if __name__ == "__main__":
    main()
