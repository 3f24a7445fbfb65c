"""The fp64 statement of include/jat_hip_harm.h: harmonic analysis, the harmonic template and the harmonic comparison.
Phases are uint32 turns exactly as the header defines them; everything else is fp64.  numpy only.

The error bounds the GPU tests hold the kernels to are derived here from the kernels' summation order; u = 2^-24.
"""
import numpy as np

U = 2.0 ** -24
TURN = 2.0 * np.pi * 2.0 ** -32


def frames_of(L, hop):
    return 1 + L // hop


def window(N):
    """the periodic Hann window as the library rounds it: the fp64 formula of jat_audio_metrics_create, then fp32"""
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N)).astype(np.float32)


def turns(f, sr):
    """uint32(llrint(f / sr * 2^32)), f an fp64 array in [0, sr / 2)"""
    return np.rint(np.asarray(f, np.float64) / float(sr) * 4294967296.0).astype(np.int64).astype(np.uint32)


def angle(p):
    """2 pi float(int32(p)) 2^-32, the float() rounding to nearest even, the product in fp64"""
    return TURN * np.asarray(p, np.uint32).view(np.int32).astype(np.float32).astype(np.float64)


def is_voiced(f0, voiced):
    f0 = np.asarray(f0, np.float32)
    with np.errstate(invalid="ignore"):
        return (np.asarray(voiced) != 0) & (f0 > 0) & np.isfinite(f0)


def framed(x, N, hop):
    """x [L] -> fp64 [frames, N], frame f = x_pad[f hop : f hop + N] with N / 2 zeros a side"""
    L = x.shape[0]
    xp = np.concatenate([np.zeros(N // 2), np.asarray(x, np.float64), np.zeros(N // 2 + N)])
    idx = np.arange(frames_of(L, hop))[:, None] * hop + np.arange(N)[None, :]
    return xp[idx]


def live_mask(f0, voiced, H, sr, N):
    """[frames] -> bool [frames, H]: the frame is voiced and 0 < h f0 < sr / 2 - 2 sr / N"""
    v = is_voiced(f0, voiced)
    hf = np.arange(1, H + 1, dtype=np.float64)[None, :] * np.where(v, f0, 0).astype(np.float64)[:, None]
    return v[:, None] & (hf > 0) & (hf < sr / 2.0 - 2.0 * sr / N)


def analyze(x, f0, voiced, H, sr, N, hop):
    """one row: x fp32 [L], track [frames] -> dict(amp fp64 [frames, H], energy fp64 [frames], live bool [frames, H],
    absum fp64 [frames] = sum_n |w x|, the scale of the error bound)"""
    w = window(N).astype(np.float64)
    fr = framed(x, N, hop) * w[None, :]
    live = live_mask(f0, voiced, H, sr, N)
    amp = np.zeros((fr.shape[0], H))
    n = np.arange(N, dtype=np.uint32)
    for f, h in zip(*np.nonzero(live)):
        s = turns(float(h + 1) * float(f0[f]), sr)
        a = angle(s * n)                                       # uint32 product: modulo 2^32
        c = np.sum(fr[f] * np.cos(a)) - 1j * np.sum(fr[f] * np.sin(a))
        amp[f, h] = 2.0 * abs(c) / w.sum()
    return dict(amp=amp, energy=(fr * fr).sum(1), live=live, absum=np.abs(fr).sum(1))


def analyze_gamma(N):
    """|amp - ref| <= gamma sum_n |w x| / sum w, first order in u (the factor 2 of amp = 2 |c| / sum w is inside gamma).
    A term of Re c or Im c is (w x) cos: the product w x rounded (1 u), the window's fp32 value off by at most one unit from
    this file's where the device's fp64 cosine differs (1 u), the angle float(p) * fl(2 pi 2^-32) with the constant and the
    product rounded (|angle| <= pi: 2 pi u absolute), sincosf within 2 units of 2^-24 absolute (2 u): (4 + 2 pi) u |w x| a
    term.  A lane adds N / 64 terms with one fma each and the butterfly adds 6 times: (N / 64 + 6) u sum |w x|.  Re and Im
    together: sqrt 2.  |c| from re^2 + im^2, the square root, the division by N / 2 and N / 2 against the rounded window's
    sum: 6 u |c| <= 6 u sum |w x|."""
    return 2.0 * (np.sqrt(2.0) * (N / 64.0 + 6.0 + 4.0 + 2.0 * np.pi) + 6.0) * U * 1.01


def energy_gamma(N):
    """|energy - ref| <= gamma ref: each term (w x)^2 carries 2 (1 + 1) u from its two factors, the sum (N / 64 + 6) u"""
    return (N / 64.0 + 6.0 + 4.0) * U * 1.01


def synth_track(f0, voiced, sr, hop, L):
    """one row -> dict(f, u fp64 [L], f0n fp64 [L], inc uint32 [L], phase uint32 [L], va, vb bool [L])"""
    frames = frames_of(L, hop)
    assert len(f0) == frames
    n = np.arange(L)
    f = n // hop
    fb = np.minimum(f + 1, frames - 1)
    u = (n - f * hop).astype(np.float64) / float(hop)
    v = is_voiced(f0, voiced)
    f64 = np.where(v, f0, 0).astype(np.float64)
    va, vb = v[f], v[fb]
    both = (1.0 - u) * f64[f] + u * f64[fb]
    f0n = np.where(va & vb, both, np.where(va, f64[f], np.where(vb, f64[fb], 0.0)))
    below = f0n < sr / 2.0                                                  # at or above Nyquist the phase stands still
    inc = np.where(below, turns(np.where(below, f0n, 0.0), sr), 0).astype(np.uint32)
    phase = np.concatenate([np.zeros(1, np.uint32), np.cumsum(inc, dtype=np.uint32)[:-1]])
    return dict(f=f, fb=fb, u=u, f0n=f0n, inc=inc, phase=phase, va=va, vb=vb)


def synthesize(f0, voiced, amp, sr, hop, L, phase=None):
    """one row: track [frames], amp fp32 [frames, H] -> dict(y fp64 [L], absum fp64 [L] = sum_h over the kept terms of
    (1 - u) |A_f| + u |A_f+1|, phase uint32 [L]).  `phase`: evaluate on these phases instead of the reference's own."""
    t = synth_track(f0, voiced, sr, hop, L)
    ph = t["phase"] if phase is None else np.asarray(phase, np.uint32)
    H = amp.shape[1]
    A = np.asarray(amp, np.float64)
    y, absum = np.zeros(L), np.zeros(L)
    for h in range(1, H + 1):
        a0 = np.where(t["va"], A[t["f"], h - 1], 0.0)
        a1 = np.where(t["vb"], A[t["fb"], h - 1], 0.0)
        keep = (t["f0n"] > 0) & (h * t["f0n"] < sr / 2.0)
        a = (1.0 - t["u"]) * a0 + t["u"] * a1
        y += np.where(keep, a * np.sin(angle(np.uint32(h) * ph)), 0.0)
        absum += np.where(keep, (1.0 - t["u"]) * np.abs(a0) + t["u"] * np.abs(a1), 0.0)
    return dict(y=y, absum=absum, phase=t["phase"], f0n=t["f0n"])


SYNTH_C = 13.0


def synth_bound(H, absum):
    """|y - ref| <= (c + H) u sum_h |a_h(n)| on the same phases.  A term a sin: a_h from u rounded to fp32, 1 - u, two products
    and a sum (3 u |a| where the two amplitudes have one sign), the angle float(int32(p)) * fl(2 pi 2^-32) with the constant and
    the product rounded (2 pi u absolute), sinf within 2 u absolute, the product in the fma: (3 + 2 pi + 2 + 1) u < 13 u a
    term; the H fmas in ascending h add H u."""
    return (SYNTH_C + H) * U * 1.01 * absum


def compare(amp_a, amp_ref, f0_ref, voiced_ref, cutoff_hz, floor):
    """one row: tables [frames, H] -> fp64 [8]: {n, sum e, sum e^2, sum |e|} of the kept band, then of the regenerated band"""
    H = amp_ref.shape[1]
    v = is_voiced(f0_ref, voiced_ref)
    ar, aa = np.asarray(amp_ref, np.float64), np.asarray(amp_a, np.float64)
    cell = v[:, None] & (ar > floor)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = 20.0 * np.log10((aa + floor) / (ar + floor))
    hf = np.arange(1, H + 1, dtype=np.float64)[None, :] * np.where(v, f0_ref, 0).astype(np.float64)[:, None]
    out = []
    for band in (cell & (hf < cutoff_hz), cell & ~(hf < cutoff_hz)):
        eb = e[band]
        out += [float(band.sum()), eb.sum(), (eb * eb).sum(), np.abs(eb).sum()]
    return np.array(out, np.float64)


def band_report(s):
    n = s[0]
    if n <= 0:
        return {"n_cells": 0, "bias_db": 0.0, "rms_db": 0.0, "mean_abs_db": 0.0}
    return {"n_cells": int(n), "bias_db": s[1] / n, "rms_db": float(np.sqrt(s[2] / n)), "mean_abs_db": s[3] / n}


def harmonicity(amp, energy, N):
    w = window(N).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(energy > 0, (amp ** 2).sum(-1) * 0.5 * (w * w).sum() / energy, 0.0)


# ---- fixtures shared by the CPU and the GPU tests ----------------------------------------------------------------------------
SHAPES = ((1, 1, 256, 64, 1), (3, 64 * 3 + 17, 256, 64, 5), (2, 512 * 9 + 100, 2048, 512, 64), (1, 700, 2048, 512, 128))
SR = 44100


def rng(salt):
    return np.random.default_rng(1234 + salt)


def case_track(B, frames, H, sr, N, salt, glide=False):
    """f0 fp32, voiced uint8 [B, frames]: mixed voiced / unvoiced frames, f0 placed so that harmonics cross the guard (and
    Nyquist) inside the table, one voiced frame with f0 = 0 and one with NaN (where there are frames enough)"""
    g = rng(salt)
    top = sr / 2.0 - 2.0 * sr / N
    lo, hi = top / (H + 0.5) * 0.35, top / max(H - 0.5, 0.6) * 1.3        # from "all live" to "the last ones are not"
    if glide:
        f0 = np.exp(np.linspace(np.log(lo), np.log(hi), frames))[None, :] * (1 + 0.1 * g.random((B, 1)))
    else:
        f0 = lo + (hi - lo) * g.random((B, frames))
    f0 = f0.astype(np.float32)
    voiced = (g.random((B, frames)) < 0.7).astype(np.uint8)
    if frames >= 4:
        voiced[:, 0], voiced[:, 1] = 1, 0                                  # a voiced -> unvoiced -> voiced transition
        f0[:, frames // 2] = 0.0
        voiced[:, frames // 2] = 1
        f0[:, frames - 1] = np.nan
        voiced[:, frames - 1] = 1
    else:
        voiced[:] = 1
    return f0, voiced


def case_signal(B, L, salt):
    g = rng(100 + salt)
    t = np.arange(L)[None, :]
    x = 0.4 * np.sin(2 * np.pi * (0.01 + 0.02 * g.random((B, 1))) * t) + 0.2 * g.standard_normal((B, L))
    return x.astype(np.float32)


def case_amp(B, frames, H, salt):
    return (rng(200 + salt).random((B, frames, H)) / H).astype(np.float32)


# the round trip on a constant f0: harmonics at least five bins apart
ROUND_TRIP = ((110.0, 32), (220.0, 16), (440.0, 40), (997.0, 22))


def round_trip(f0_hz, H, sr=SR, N=2048, hop=512, n_frames=12):
    """-> (worst relative error over the live harmonics of the inner frames, amplitudes)"""
    L = (n_frames - 1) * hop
    f0 = np.full(n_frames, f0_hz, np.float32)
    voiced = np.ones(n_frames, np.uint8)
    amp = np.full(H, 1.0 / H, np.float32)                                  # the flat template of generate_harmonics
    y = synthesize(f0, voiced, np.tile(amp, (n_frames, 1)), sr, hop, L)["y"]
    r = analyze(y.astype(np.float32), f0, voiced, H, sr, N, hop)
    inner = slice(3, n_frames - 3)                                         # frames that hold no padding
    live = r["live"][inner]
    rel = np.abs(r["amp"][inner] - amp[None, :]) / amp[None, :]
    return float(rel[live].max()), live
