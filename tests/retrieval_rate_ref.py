"""The normative statement of the voicing-aware index rates (include/jat_hip_rate.h, csrc/retrieval_rate.hip) in
numpy: the stability classes of a pitch track, the rate track they select and the mix with a per-frame rate.  fp32 with one
rounding per operation, in the order the header states, so the GPU is compared with these bit for bit.

Also the fixture the CPU and the GPU test share: a steady tone, noise and a gliding tone, with the frames far enough inside a
segment for their class to be decided by that segment alone."""
import functools

import numpy as np

from retrieval_ms_ref import fma32

MAX_HALF_WINDOW, MAX_SMOOTH = 32, 16
F32 = np.float32


def cents_ratio(cents):
    """float32(2 ** (cents / 1200)), the power taken in double"""
    return F32(2.0 ** (float(cents) / 1200.0))


def default_min_count(W):
    return 2 * W + 1 - W // 2


def live(f0, voiced):
    f0 = np.asarray(f0, F32)
    with np.errstate(invalid="ignore"):
        return (np.asarray(voiced) != 0) & (f0 > 0) & np.isfinite(f0)


def f0_classes(f0, voiced, W=4, ratio=None, min_count=None):
    """f0 fp32 [B, F], voiced [B, F] -> (cls uint8 [B, F], count int32 [B, F], summary int32 [B, 2])"""
    f0 = np.asarray(f0, F32)
    ratio = cents_ratio(50.0) if ratio is None else F32(ratio)
    m = default_min_count(W) if min_count is None else int(min_count)
    B, F = f0.shape
    lv = live(f0, voiced)
    count = np.zeros((B, F), np.int32)
    with np.errstate(over="ignore", invalid="ignore"):
        up = (f0 * ratio).astype(F32)                                     # one fp32 multiply per frame; may round to +inf
        for b in range(B):
            for t in range(F):
                if not lv[b, t]:
                    continue
                a, e = max(0, t - W), min(F - 1, t + W)
                j = np.arange(a, e + 1)
                count[b, t] = int((lv[b, j] & (f0[b, j] <= up[b, t]) & (f0[b, t] <= up[b, j])).sum())
    cls = np.where(lv, np.where(count >= m, 2, 1), 0).astype(np.uint8)
    summary = np.stack([(cls > 0).sum(axis=1), (cls == 2).sum(axis=1)], axis=1).astype(np.int32)
    return cls, count, summary


def rate_table(index_rate, protect=1.0, unstable=1.0):
    """{not live, unstable, stable}: the products in double, rounded to fp32 once"""
    r = float(index_rate)
    return np.array([F32(r * float(protect)), F32(r * float(unstable)), F32(r)], F32)


def rate_track(cls, T, table, S):
    """cls uint8 [B, F] -> r fp32 [B, T]; table fp32 [3]"""
    cls = np.asarray(cls)
    table = np.asarray(table, F32) + F32(0)                               # -0 -> +0
    B, F = cls.shape
    c = np.empty((B, T), F32)
    n = min(F, T)
    c[:, :n] = table[np.minimum(cls[:, :n], 2)]
    c[:, n:] = table[0]
    r = np.empty((B, T), F32)
    for t in range(T):
        a, e = max(0, t - S), min(T - 1, t + S)
        acc = (c[:, a] - c[:, t]).astype(F32)
        for j in range(a + 1, e + 1):
            acc = (acc + (c[:, j] - c[:, t]).astype(F32)).astype(F32)
        v = (c[:, t] + (acc / F32(e - a + 1)).astype(F32)).astype(F32)
        r[:, t] = np.where(v < 0, F32(0), np.where(v > 1, F32(1), v))
    return r


def mix(x, v, rates):
    """x, v fp32 [B, C, T], rates fp32 [B, T] -> fma(1 - r, x, r v): 1 - r and r v rounded once each, then one fma"""
    x, v = np.asarray(x, F32), np.asarray(v, F32)
    r = np.broadcast_to(np.asarray(rates, F32)[:, None, :], x.shape)
    keep = (F32(1) - r).astype(F32)
    return fma32(keep, x, (r * v).astype(F32))


# ---- the fixture: tone, noise, glide ------------------------------------------------------------------------------------------
SR, HOP, SEG_SECONDS = 44100, 512, 0.4
FIXTURE_W = 4
SEG = int(SR * SEG_SECONDS)                                               # 17640 samples a segment
FIXTURE_CLASSES = (2, 0, 1)                                               # tone: stable, noise: not live, glide: unstable


@functools.lru_cache(maxsize=None)
def fixture_signal():
    """fp32 [3 SEG]: 0.4 s of a 220 Hz tone, 0.4 s of seeded white noise, 0.4 s of a tone gliding 200 -> 400 Hz.  The glide is
    exponential: one octave in 34.45 frames, 34.8 cents a frame everywhere, so the neighbouring frame is 15 cents inside the
    50-cent limit and the next one 20 cents outside it: 3 of 9 frames agree, far from the 7 that make a frame stable."""
    t = np.arange(SEG, dtype=np.float64) / SR
    tone = 0.5 * np.sin(2 * np.pi * 220.0 * t)
    noise = 0.25 * np.random.default_rng(20281).standard_normal(SEG)
    glide = 0.5 * np.sin(2 * np.pi * 200.0 * SEG_SECONDS / np.log(2.0) * (2.0 ** (t / SEG_SECONDS) - 1.0))
    x = np.concatenate([tone, noise, glide]).astype(np.float32)
    x.setflags(write=False)
    return x


def fixture_frames():
    return 1 + 3 * SEG // HOP


def fixture_inner(W=FIXTURE_W):
    """-> segment int [F]: 0, 1, 2 for a frame whose centre (sample t HOP) lies at least W + 2 frames inside that segment
    (two frames: the analysis frame itself; W: the frames its count looks at), -1 for the frames left out"""
    F = fixture_frames()
    seg = np.full(F, -1, np.int64)
    margin = (W + 2) * HOP
    for t in range(F):
        for s in range(3):
            if s * SEG + margin <= t * HOP <= (s + 1) * SEG - margin:
                seg[t] = s
    return seg
