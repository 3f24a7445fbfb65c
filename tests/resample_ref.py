"""fp64 numpy restatement of the windowed-sinc resampler (Hann window), written from its formula:

    g = gcd(orig, new);  o = orig / g;  n = new / g;  base = min(o, n) * rolloff
    width = ceil(lpw * o / base);  K = 2 width + o
    t = clamp((-p / n + (k - width) / o) * base, -lpw, +lpw)
    h[p][k] = (t == 0 ? 1 : sin(pi t) / (pi t)) * cos(pi t / lpw / 2)^2 * (base / o)
    y[f n + p] = sum_k h[p][k] x[f o + k - width]   (x = 0 outside [0, L)),   L_out = ceil(n L / o)

and of the reference's chunk bounds and the chain of the data preparation.  Test infrastructure only."""
import math

import numpy as np


def dims(orig, new, lpw=6, rolloff=0.99):
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    base = min(o, n) * rolloff
    width = int(math.ceil(lpw * o / base))
    return o, n, width, 2 * width + o, base


def table(orig, new, lpw=6, rolloff=0.99):
    """-> h fp64 [n, K]"""
    o, n, width, K, base = dims(orig, new, lpw, rolloff)
    p = np.arange(n, dtype=np.float64)[:, None]
    k = np.arange(K, dtype=np.float64)[None, :]
    t = np.clip((-p / n + (k - width) / o) * base, -lpw, lpw)
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(t == 0, 1.0, np.sin(np.pi * t) / (np.pi * t))
    return sinc * np.cos(np.pi * t / lpw / 2) ** 2 * (base / o)


def out_length(L, orig, new):
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    return -(-n * L // o)


def resample(x, orig, new, lpw=6, rolloff=0.99):
    """x [..., L] -> fp64 [..., ceil(n L / o)]: per phase a strided dot product with the zero-padded input."""
    x = np.asarray(x, dtype=np.float64)
    if orig == new:
        return x.copy()
    o, n, width, K, _ = dims(orig, new, lpw, rolloff)
    h = table(orig, new, lpw, rolloff)
    L = x.shape[-1]
    L_out = out_length(L, orig, new)
    F = -(-L_out // n)
    lead = x.shape[:-1]
    xp = np.zeros(lead + (width + (F - 1) * o + K + o,), np.float64)
    xp[..., width:width + L] = x
    # windows[..., f, k] = xp[..., f o + k]
    idx = (np.arange(F) * o)[:, None] + np.arange(K)[None, :]
    y = np.empty(lead + (F, n), np.float64)
    step = max(1, (1 << 22) // K)
    for f0 in range(0, F, step):
        win = xp[..., idx[f0:f0 + step]]                     # [..., f, K]
        y[..., f0:f0 + step, :] = win @ h.T
    return y.reshape(lead + (F * n,))[..., :L_out]


def resample_at(x, orig, new, out_idx, lpw=6, rolloff=0.99):
    """The outputs at the given indices only (1-D x): for spot checks of long signals."""
    x = np.asarray(x, dtype=np.float64)
    o, n, width, K, _ = dims(orig, new, lpw, rolloff)
    h = table(orig, new, lpw, rolloff)
    L = x.shape[-1]
    out = np.empty(len(out_idx), np.float64)
    for j, i in enumerate(out_idx):
        f, p = divmod(int(i), n)
        s = f * o - width
        a, b = max(s, 0), min(s + K, L)
        out[j] = h[p, a - s:b - s] @ x[a:b] if b > a else 0.0
    return out


def simulate_lr(hr, high=48000, low=16000):
    y = resample(resample(hr, high, low), low, high)
    n = np.asarray(hr).shape[-1]
    if y.shape[-1] < n:
        y = np.concatenate([y, np.zeros(y.shape[:-1] + (n - y.shape[-1],))], axis=-1)
    return y[..., :n]


def chunk_bounds(total_samples, sr, chunk=7.0, overlap=0.5, min_duration=1.0):
    """The reference's chunking loop restated line by line: [(idx_start, idx_end, pad_left, pad_right)], [] when skipped."""
    duration_sec = total_samples / sr
    if duration_sec < min_duration:
        return []
    out = []
    num_chunks = math.ceil(duration_sec / chunk)
    for i in range(num_chunks):
        t_start = i * chunk - overlap
        t_end = t_start + chunk + (2 * overlap)
        idx_start = int(t_start * sr)
        idx_end = int(t_end * sr)
        pad_left = 0
        if idx_start < 0:
            pad_left = -idx_start
            idx_start = 0
        pad_right = 0
        if idx_end > total_samples:
            pad_right = idx_end - total_samples
            idx_end = total_samples
        out.append((idx_start, idx_end, pad_left, pad_right))
    return out
