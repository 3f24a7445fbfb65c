"""Data formats either side of the sampling path (reference infer_test_v3m2.py / prepare_dataset_v5.py).

* latent files: `torch.save({'hr_latent': fp16 [1024, T], 'lr_latent': fp16 [1024, T], 'metadata': ...})`
  (prepare_dataset_v5.py:255-264), read with `torch.load(..., mmap=True)` and `.float()` (infer_test_v3m2.py:292-294);
* normalisation statistics (infer_test_v3m2.py:300-332): JSON with hr_mean / hr_std / lr_mean / lr_std lists
  (recalculate_stats.py:113-121), or a `.pt` dict with those keys, or running sums {sum, sq_sum, count} over the
  2048 concatenated channels;
* checkpoints: `jatsr_amd.model.load_model` (infer_test_v3m2.py:33-94).

Pure host code (PyTorch only as the container / file reader); nothing here computes on the hot path.
"""
from __future__ import annotations

import json
import os

import torch


def load_latent_file(path, mmap=True):
    """-> (hr_latent or None, lr_latent) as fp32 [C, T] CPU tensors (infer_test_v3m2.py:292-294)."""
    data = torch.load(path, map_location="cpu", mmap=mmap, weights_only=False)
    if "lr_latent" not in data:
        raise KeyError(f"{path}: no 'lr_latent' (keys: {list(data.keys())})")
    hr = data["hr_latent"].float() if "hr_latent" in data else None
    return hr, data["lr_latent"].float()


def save_latent_file(path, hr_latent=None, lr_latent=None, metadata=None, **extra):
    """Write the reference's latent container (fp16 tensors, prepare_dataset_v5.py:255-264)."""
    out = dict(extra)
    if hr_latent is not None:
        out["hr_latent"] = hr_latent.detach().to("cpu", torch.float16)
    if lr_latent is not None:
        out["lr_latent"] = lr_latent.detach().to("cpu", torch.float16)
    out["metadata"] = metadata or {}
    torch.save(out, path)


def load_stats(path, channels=1024, device="cpu"):
    """Per-channel normalisation statistics -> dict(hr_mean, hr_std, lr_mean, lr_std), each fp32 [channels].

    Accepts the three formats infer_test_v3m2.py:300-332 accepts; raises ValueError on anything else."""
    if str(path).endswith(".json"):
        with open(path, "r") as f:
            raw = json.load(f)
        stats = {k: torch.tensor(raw[k], dtype=torch.float32) for k in ("hr_mean", "hr_std", "lr_mean", "lr_std")}
    else:
        raw = torch.load(path, map_location="cpu", weights_only=False)
        if "hr_mean" in raw:
            stats = {k: torch.as_tensor(raw[k]).float() for k in ("hr_mean", "hr_std", "lr_mean", "lr_std")}
        elif "sum" in raw:
            count = raw["count"]
            mean = torch.as_tensor(raw["sum"]).double() / count
            var = torch.as_tensor(raw["sq_sum"]).double() / count - mean ** 2
            std = torch.sqrt(var + 1e-8)
            # first `channels` entries are HR, the rest LR (infer_test_v3m2.py:322-326)
            stats = {"hr_mean": mean[:channels].float(), "hr_std": std[:channels].float(),
                     "lr_mean": mean[channels:].float(), "lr_std": std[channels:].float()}
        else:
            raise ValueError(f"Unknown stats format. Keys: {list(raw.keys())}")
    for k, v in stats.items():
        v = v.reshape(-1)
        if v.numel() != channels:
            raise ValueError(f"{path}: {k} has {v.numel()} entries, expected {channels}")
        stats[k] = v.to(device)
    return stats


def frames_for_seconds(seconds, sample_rate=44100, hop=512):
    """DAC 44.1 kHz latent frames for a duration (infer_test_v3m2.py:340-350): 16 s -> 1378, 2 s -> 172."""
    return int(seconds * sample_rate / hop)


def first_latent_file(val_dir):
    """Default input: the first `*.pt` of the validation directory (infer_test_v3m2.py:283-289)."""
    files = sorted(f for f in os.listdir(val_dir) if f.endswith(".pt"))
    if not files:
        raise FileNotFoundError(f"No files found in {val_dir}")
    return os.path.join(val_dir, files[0])


def write_wav_float32(path, samples, sample_rate=44100):
    """32-bit IEEE-float WAV (format tag 3), what `torchaudio.save` writes for a float32 tensor
    (infer_test_v3m2.py:425-436).  Stdlib only; `samples`: 1-D array-like or a [1, n] tensor (mono), or a [channels, n]
    tensor or array (interleaved on disk)."""
    import array
    import struct
    channels = 1
    if getattr(samples, "ndim", 1) == 2 and samples.shape[0] > 1:
        channels = int(samples.shape[0])
        samples = samples.T                                   # [n, channels]: frames of interleaved samples
    if hasattr(samples, "detach"):
        samples = samples.detach().to("cpu", torch.float32).reshape(-1).tolist()
    elif channels > 1:
        samples = samples.reshape(-1).tolist()
    data = array.array("f", samples)
    if struct.pack("=f", 1.0) != struct.pack("<f", 1.0):
        data.byteswap()
    body = data.tobytes()
    fmt = struct.pack("<HHIIHH", 3, channels, sample_rate, sample_rate * 4 * channels, 4 * channels, 32)
    # WAVE_FORMAT_IEEE_FLOAT: fmt chunk with cbSize = 0 and a fact chunk (sample count), as libsndfile writes it
    fmt += struct.pack("<H", 0)
    fact = struct.pack("<4sII", b"fact", 4, len(data) // channels)
    size = 4 + (8 + len(fmt)) + len(fact) + (8 + len(body))
    with open(path, "wb") as f:
        f.write(struct.pack("<4sI4s", b"RIFF", size, b"WAVE"))
        f.write(struct.pack("<4sI", b"fmt ", len(fmt)) + fmt)
        f.write(fact)
        f.write(struct.pack("<4sI", b"data", len(body)) + body)
    return path


def read_wav(path, mono=True):
    """WAV file -> (float32 numpy [L], sample_rate).  Reads PCM 16 / 24 / 32-bit integer (format tag 1) and 32-bit IEEE
    float (tag 3), also inside WAVE_FORMAT_EXTENSIBLE (tag 0xFFFE); integers are scaled by 2^-(bits-1).  Multi-channel
    audio is averaged to mono, as the reference does (prepare_dataset_v5.py:130), unless mono=False, which keeps the
    channels: [channels, L].  Stdlib + numpy only; a malformed or unsupported file raises ValueError."""
    import struct

    import numpy as np
    with open(path, "rb") as f:
        raw = f.read()
    if len(raw) < 12 or raw[:4] != b"RIFF" or raw[8:12] != b"WAVE":
        raise ValueError(f"{path}: not a RIFF/WAVE file")
    pos, fmt, data = 12, None, None
    while pos + 8 <= len(raw):
        cid, n = struct.unpack("<4sI", raw[pos:pos + 8])
        body = raw[pos + 8:pos + 8 + n]
        if len(body) < n:
            raise ValueError(f"{path}: chunk {cid!r} is truncated")
        if cid == b"fmt ":
            if n < 16:
                raise ValueError(f"{path}: fmt chunk of {n} bytes")
            fmt = struct.unpack("<HHIIHH", body[:16])
            if fmt[0] == 0xFFFE:
                if n < 26:
                    raise ValueError(f"{path}: WAVE_FORMAT_EXTENSIBLE fmt chunk of {n} bytes")
                fmt = (struct.unpack("<H", body[24:26])[0],) + fmt[1:]   # the sub-format GUID's leading tag
        elif cid == b"data":
            data = body
        pos += 8 + n + (n & 1)
    if fmt is None or data is None:
        raise ValueError(f"{path}: missing {'fmt' if fmt is None else 'data'} chunk")
    tag, ch, sr, _, align, bits = fmt
    if ch < 1 or sr < 1 or align != ch * bits // 8:
        raise ValueError(f"{path}: inconsistent fmt chunk (channels {ch}, rate {sr}, block align {align}, bits {bits})")
    usable = len(data) - len(data) % align
    if tag == 3 and bits == 32:
        x = np.frombuffer(data[:usable], "<f4").astype(np.float32)
    elif tag == 1 and bits in (16, 32):
        x = np.frombuffer(data[:usable], "<i2" if bits == 16 else "<i4").astype(np.float64) / 2.0 ** (bits - 1)
    elif tag == 1 and bits == 24:
        b = np.frombuffer(data[:usable], np.uint8).reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        x = (v - ((v & 0x800000) << 1)).astype(np.float64) / 2.0 ** 23
    else:
        raise ValueError(f"{path}: unsupported WAV format tag {tag} with {bits} bits")
    if not mono:
        return np.ascontiguousarray(x.reshape(-1, ch).T).astype(np.float32), sr
    x = x.reshape(-1, ch).mean(axis=1) if ch > 1 else x
    return x.astype(np.float32), sr
