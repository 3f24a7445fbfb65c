"""The normative statement of the pitch tracker (include/jat_hip.h, csrc/pitch.hip): steps 1-5 of de Cheveigne & Kawahara
(2002), arranged as librosa.yin arranges them, in numpy.  dtype=np.float64 is the reference; dtype=np.float32 is the
yardstick the GPU is compared with (the same formula in the GPU's precision, in numpy's own summation order).  Equality with
librosa itself is not claimed: it is not installed where these tests run.

The continuous stage (`difference`, `cmndf`) and the discrete stage (`select`, `shift`) are separate functions, so that a test
can run the discrete stage on the GPU's own cmndf, where every comparison of fp32 values is exact in fp64."""
import functools
import math

import numpy as np

TINY = float(np.finfo(np.float32).tiny)

# sr, frame_length, hop_length, fmin, fmax, L, seeds (one row each), trough_threshold: the smallest shapes that reach each branch
CASES = {
    "defaults": (44100, 2048, 512, 50.0, 1000.0, 44100 + 137, (0, 1, 2), 0.1),      # ragged tail, lags no multiple of the block
    "short": (44100, 2048, 512, 43.0, 2000.0, 700, (0,), 0.1),                       # shorter than a frame, max_period capped at 1023
    "sr16k": (16000, 1024, 256, 40.0, 800.0, 32005, (0, 1), 0.1),                    # a second frame size
    "frame4096": (48000, 4096, 1024, 30.0, 1200.0, 48001, (0,), 0.1),                # the largest LDS footprint under test
    "threshold": (44100, 2048, 512, 50.0, 1000.0, 44237, (0,), 0.3),                 # a different voiced set
}


def periods(sr, fmin, fmax, frame_length):
    W = frame_length // 2
    return int(math.floor(sr / fmax)), int(min(math.ceil(sr / fmin), frame_length - W - 1))


def frame(x, frame_length, hop_length):
    """[L] -> [1 + L // hop, frame_length]: the frames of the signal zero-padded by frame_length / 2 a side"""
    n = 1 + len(x) // hop_length
    xp = np.pad(np.asarray(x), frame_length // 2)
    return xp[np.arange(n)[:, None] * hop_length + np.arange(frame_length)[None, :]]


def difference(frames, max_period, dtype=np.float64):
    """d[f, tau] = sum_{j < W} (x[j] - x[j + tau])^2 for tau = 0 .. max_period (d[:, 0] = 0), the direct form"""
    fr = frames.astype(dtype)
    W = fr.shape[1] // 2
    d = np.zeros((fr.shape[0], max_period + 1), dtype)
    for tau in range(1, max_period + 1):
        e = fr[:, :W] - fr[:, tau:tau + W]
        d[:, tau] = (e * e).sum(axis=1, dtype=dtype)
    return d


def cmndf(d, dtype=np.float64):
    """c[f, tau] = d / ((1 / tau) sum_{u = 1 .. tau} d(u) + tiny) for tau >= 1, c[:, 0] = 1"""
    d = d.astype(dtype)
    tau = np.arange(1, d.shape[1], dtype=dtype)
    mean = np.cumsum(d[:, 1:], axis=1, dtype=dtype) / tau
    c = d[:, 1:] / (mean + dtype(TINY))
    return np.concatenate([np.ones((d.shape[0], 1), dtype), c], axis=1)


def select(c, min_period, max_period, threshold):
    """c [F, max_period + 1] -> (k int [F], voiced bool [F]): the first trough of y = c[:, min_period : max_period + 1] under
    the threshold, else the lowest-index minimum.  Comparisons only: exact in whatever dtype c has."""
    y = c[:, min_period:max_period + 1]
    trough = np.zeros(y.shape, bool)
    trough[:, 1:-1] = (y[:, 1:-1] < y[:, :-2]) & (y[:, 1:-1] <= y[:, 2:])
    trough[:, 0] = y[:, 0] < y[:, 1]
    under = trough & (y < threshold)
    voiced = under.any(axis=1)
    return np.where(voiced, under.argmax(axis=1), y.argmin(axis=1)).astype(np.int64), voiced


def shift(y, k):
    """the parabolic shift of the chosen index, in y's dtype: -b / a where |b| < |a|, 0 otherwise and at either end"""
    ny = y.shape[1]
    rows = np.arange(y.shape[0])
    ym, y0, yp = y[rows, np.clip(k - 1, 0, ny - 1)], y[rows, k], y[rows, np.clip(k + 1, 0, ny - 1)]
    a = (yp + ym) - y.dtype.type(2) * y0
    b = (yp - ym) / y.dtype.type(2)
    ok = (k > 0) & (k < ny - 1) & (np.abs(b) < np.abs(a))
    return np.where(ok, -b / np.where(ok, a, y.dtype.type(1)), y.dtype.type(0)).astype(y.dtype)


def finish(c, k, sr, min_period, max_period):
    """-> (f0, aperiodicity) in c's dtype from the chosen indices"""
    y = c[:, min_period:max_period + 1]
    t = y.dtype.type
    f0 = t(sr) / ((min_period + k).astype(y.dtype) + shift(y, k))
    return f0.astype(y.dtype), y[np.arange(y.shape[0]), k]


def yin(x, sr=44100, fmin=50.0, fmax=1000.0, frame_length=2048, hop_length=512, trough_threshold=0.1, dtype=np.float64):
    """x [L] (fp32 values) -> dict(d, cmndf, index, voiced, f0, aperiodicity); the threshold is rounded to fp32 first, as
    the C ABI carries it"""
    lo, hi = periods(sr, fmin, fmax, frame_length)
    d = difference(frame(np.asarray(x, np.float32), frame_length, hop_length), hi, dtype)
    c = cmndf(d, dtype)
    k, voiced = select(c, lo, hi, dtype(np.float32(trough_threshold)))
    f0, ap = finish(c, k, sr, lo, hi)
    return {"d": d, "cmndf": c, "index": k, "voiced": voiced, "f0": f0, "aperiodicity": ap}


def cents(a, b):
    return 1200.0 * np.log2(np.asarray(a, np.float64) / np.asarray(b, np.float64))


def mix(sr, L, seed, frame_length=2048):
    """The test signal, fp32 [L]: six harmonics (amplitudes 0.6^n) of a glide 110 -> 440 Hz with 1 % vibrato at 5.5 Hz, scaled by
    0.2, plus 0.01 white noise; the span [L/3, L/3 + L/8) replaced by 0.1 white noise and the L/10 samples after it by exact
    zeros.  A clip shorter than one frame is a plain 220 Hz harmonic tone."""
    rng = np.random.default_rng(1000 + seed)
    t = np.arange(L) / sr
    if L < frame_length:
        f_inst = np.full(L, 220.0)
    else:
        f_inst = 110.0 * 4.0 ** (t / (L / sr)) * (1.0 + 0.01 * np.sin(2 * np.pi * 5.5 * t))
    phase = 2 * np.pi * np.cumsum(f_inst) / sr
    x = 0.2 * sum(0.6 ** n * np.sin((n + 1) * phase) for n in range(6))
    if L >= frame_length:
        x = x + 0.01 * rng.standard_normal(L)
        a, b = L // 3, L // 3 + L // 8
        x[a:b] = 0.1 * rng.standard_normal(b - a)
        x[b:b + L // 10] = 0.0
    return x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (x fp32 [B, L], [fp64 result per row], [fp32 result per row]) of CASES[name]; computed once, never modified"""
    sr, fl, hop, fmin, fmax, L, seeds, thr = CASES[name]
    x = np.stack([mix(sr, L, s, fl) for s in seeds])
    x.setflags(write=False)
    r64 = [yin(row, sr, fmin, fmax, fl, hop, thr, np.float64) for row in x]
    r32 = [yin(row, sr, fmin, fmax, fl, hop, thr, np.float32) for row in x]
    return x, r64, r32


def compare_counts(f0_a, voiced_a, f0_b, voiced_b, gross_cents=50.0):
    """one pair of tracks -> the six figures of jat_f0_compare in fp64 (b is the reference track)"""
    a, r = np.asarray(voiced_a) != 0, np.asarray(voiced_b) != 0
    both = a & r
    c = np.abs(cents(np.asarray(f0_a, np.float32)[both], np.asarray(f0_b, np.float32)[both]))
    gross = ~(c <= gross_cents)
    return np.array([r.sum(), both.sum(), (a != r).sum(), gross.sum(), c.sum(), c[~gross].sum()], np.float64)
