"""The normative statement of the pYIN tracker (include/jat_hip.h, csrc/pyin.hip): Mauch & Dixon (2014) on YIN's normalised
difference (tests/pitch_ref.py), arranged as librosa.pyin arranges it, in numpy.  dtype=np.float64 is the reference;
dtype=np.float32 is the same statement with the GPU's number formats (fp32 tables, products, sums and Viterbi; the parabolic
shift and the bin position in fp64 on the fp32 cmndf, as the kernel takes them).  Equality with librosa itself is not claimed:
it is not installed where these tests run.  The departures from librosa, marked (D):
  (D1) a trough's bin is clipped to n_bins - 1 (librosa: n_bins, which lands in the unvoiced half and is overwritten)
  (D2) a transition that leaves the band is impossible (librosa: log(tiny))
  (D3) f0 is 0 where unvoiced (librosa: NaN)

The stages are separate functions, so that a test can run each on the GPU's own output of the stage before it:
  stage 1  troughs(y), shifts(y)                 the candidates and their parabolic shifts
  stage 2  probs(c, T)                           the threshold prior spread over the troughs -> prob [F, ny]
  stage 3  bin_positions / bins / scatter / observe   pitch bins, obs [F, n_bins], voiced_prob, log_obs [F, n_bins + 1]
  stage 4  tables(...)                           beta, A, invD, logw, logZ, lk, ls, logpi, freqs
  stage 5  viterbi(log_obs, T, dtype)            state [F]; in fp32 every step is one rounded add, subtract or max
  stage 6  track(state, T)                       (f0, voiced)"""
import functools
import math

import numpy as np

import pitch_ref as P

TINY = P.TINY
DEFAULTS = dict(n_thresholds=100, beta_parameters=(2.0, 18.0), boltzmann_parameter=2.0, resolution=0.1,
                max_transition_rate=35.92, switch_prob=0.01, no_trough_prob=0.01)
OCTAVE = dict(sr=44100, L=22127, seed=2000)


def betainc(a, b, x):
    """the regularised incomplete beta function I_x(a, b) in fp64: the closed binomial sum where a and b are whole numbers,
    else the continued fraction (modified Lentz)"""
    if x <= 0.0:
        return 0.0
    if x >= 1.0:
        return 1.0
    if float(a).is_integer() and float(b).is_integer() and a + b < 400:
        n, a = int(a + b - 1), int(a)
        return math.fsum(math.comb(n, j) * x ** j * (1.0 - x) ** (n - j) for j in range(a, n + 1))
    if x > (a + 1.0) / (a + b + 2.0):
        return 1.0 - betainc(b, a, 1.0 - x)
    front = math.exp(math.lgamma(a + b) - math.lgamma(a) - math.lgamma(b) + a * math.log(x) + b * math.log1p(-x)) / a
    tiny = 1e-300
    c, d = 1.0, 1.0 - (a + b) * x / (a + 1.0)
    d = 1.0 / (d if abs(d) > tiny else tiny)
    f = d
    for m in range(1, 400):
        for num in (m * (b - m) * x / ((a + 2 * m - 1) * (a + 2 * m)), -(a + m) * (a + b + m) * x / ((a + 2 * m) * (a + 2 * m + 1))):
            d = 1.0 + num * d
            d = 1.0 / (d if abs(d) > tiny else tiny)
            c = 1.0 + num / c
            c = c if abs(c) > tiny else tiny
            f *= d * c
        if abs(d * c - 1.0) < 1e-16:
            break
    return front * f


def beta_probs(a, b, n):
    """beta_m, m = 1 .. n: the Beta(a, b) mass on ((m - 1) / n, m / n]"""
    cdf = np.array([betainc(a, b, m / n) for m in range(n + 1)])
    return np.maximum(np.diff(cdf), 0.0)                       # a mass is never negative


def tables(sr=44100, fmin=50.0, fmax=1000.0, frame_length=2048, hop_length=512, n_thresholds=100, beta_parameters=(2.0, 18.0),
           boltzmann_parameter=2.0, resolution=0.1, max_transition_rate=35.92, switch_prob=0.01, no_trough_prob=0.01):
    """every table of the statement in fp64 (theta: the fp32 thresholds, as fp64); made once per parameter set"""
    lo, hi = P.periods(sr, fmin, fmax, frame_length)
    N, lam = int(n_thresholds), float(boltzmann_parameter)
    bps = int(math.ceil(1.0 / resolution))
    n_bins = int(math.floor(12 * bps * math.log2(fmax / fmin))) + 1
    H = int(round(max_transition_rate * 12 * hop_length / sr)) * bps
    nt_max = (hi - lo + 1) // 2 + 1
    beta = beta_probs(beta_parameters[0], beta_parameters[1], N)
    p = np.arange(nt_max + 1, dtype=np.float64)
    A = -np.expm1(-lam) * np.exp(-lam * p)
    invD = np.zeros(nt_max + 1)
    invD[1:] = 1.0 / -np.expm1(-lam * p[1:])
    A[A < TINY] = 0.0
    delta = np.arange(-H, H + 1)
    w = 1.0 - np.abs(delta) / (H + 1.0)
    Z = np.array([w[(delta + r >= 0) & (delta + r < n_bins)].sum() for r in range(n_bins)])
    return dict(sr=sr, fmin=float(fmin), fmax=float(fmax), frame_length=frame_length, hop_length=hop_length, lo=lo, hi=hi, N=N,
                bps=bps, n_bins=n_bins, H=H, theta=(np.arange(1, N + 1) / N).astype(np.float32).astype(np.float64), beta=beta,
                cum_beta=np.concatenate([[0.0], np.cumsum(beta)]), A=A, invD=invD, no_trough_prob=float(no_trough_prob),
                logw=np.log(w), logZ=np.log(Z), lk=math.log(1.0 - switch_prob), ls=math.log(switch_prob),
                logpi=math.log(1.0 / (2 * n_bins)), freqs=(fmin * 2.0 ** (np.arange(n_bins) / (12.0 * bps))).astype(np.float32))


def troughs(y):
    """pitch_ref.select's trough rule: strict on the left, <= on the right, y[0] < y[1] at 0, never the last index"""
    t = np.zeros(y.shape, bool)
    t[:, 1:-1] = (y[:, 1:-1] < y[:, :-2]) & (y[:, 1:-1] <= y[:, 2:])
    t[:, 0] = y[:, 0] < y[:, 1]
    return t


def shifts(y):
    """pitch_ref.shift at every index, in fp64 on y's values"""
    y = y.astype(np.float64)
    s = np.zeros(y.shape)
    ym, y0, yp = y[:, :-2], y[:, 1:-1], y[:, 2:]
    a, b = (yp + ym) - 2.0 * y0, (yp - ym) / 2.0
    ok = np.abs(b) < np.abs(a)
    s[:, 1:-1] = np.where(ok, -b / np.where(ok, a, 1.0), 0.0)
    return s


def probs(c, T, dtype=np.float64):
    """stage 2 on a cmndf c [F, max_period + 1] -> prob [F, ny] in dtype, 0 where there is no trough.  Comparisons of heights
    and thresholds are exact in fp64 whatever dtype c has."""
    y = c[:, T["lo"]:T["hi"] + 1].astype(np.float64)
    tr = troughs(y)
    beta, A, invD = (T[k].astype(dtype) for k in ("beta", "A", "invD"))
    if dtype == np.float32:
        A[A < TINY] = 0
    cum, ntp = T["cum_beta"].astype(dtype), dtype(T["no_trough_prob"])
    out = np.zeros(y.shape, dtype)
    for f in range(y.shape[0]):
        idx = np.flatnonzero(tr[f])
        if not len(idx):
            continue
        h = y[f, idx]
        under = h[:, None] < T["theta"][None, :]
        n = under.sum(axis=0)
        p = np.cumsum(under, axis=0) - under
        term = np.where(under, (beta[None, :] * A[p]) * invD[n][None, :], dtype(0))
        pr = term.sum(axis=1, dtype=dtype)
        g = int(np.argmin(h))
        pr[g] = pr[g] + ntp * cum[int((~under[g]).sum())]
        out[f, idx] = pr
    return out


def bin_positions(c, T):
    """the unrounded fp64 bin position 12 bps log2(f0_i / fmin) of every candidate index [F, ny]"""
    y = c[:, T["lo"]:T["hi"] + 1]
    period = (T["lo"] + np.arange(y.shape[1], dtype=np.float64))[None, :] + shifts(y)
    return 12.0 * T["bps"] * np.log2((T["sr"] / period) / T["fmin"])


def bins(c, T):
    """-> int [F, ny]: the bin of every trough (D1), -1 where there is no trough"""
    y = c[:, T["lo"]:T["hi"] + 1]
    b = np.clip(np.rint(bin_positions(c, T)), 0, T["n_bins"] - 1).astype(np.int64)
    return np.where(troughs(y), b, -1)


def scatter(prob, bin_, n_bins):
    """obs[f, b] = prob of the largest-lag trough of frame f whose bin is b, 0 where there is none; prob's dtype"""
    obs = np.zeros((prob.shape[0], n_bins), prob.dtype)
    for f in range(prob.shape[0]):
        idx = np.flatnonzero(bin_[f] >= 0)
        win = np.full(n_bins, -1, np.int64)
        np.maximum.at(win, bin_[f, idx], idx)
        obs[f] = np.where(win >= 0, prob[f, np.maximum(win, 0)], prob.dtype.type(0))
    return obs


def observe(obs, dtype=np.float64):
    """obs [F, n_bins] -> (voiced_prob [F], log_obs [F, n_bins + 1]); the last entry is every unvoiced state's"""
    o = obs.astype(dtype)
    t = dtype
    vp = np.clip(o.sum(axis=1, dtype=dtype), t(0), t(1))
    unv = (t(1) - vp) / t(o.shape[1]) + t(TINY)
    return vp, np.log(np.concatenate([o + t(TINY), unv[:, None]], axis=1)).astype(dtype)


def viterbi(log_obs, T, dtype=np.float64, tables_=None):
    """stage 5 -> state int [F] in 0 .. 2 n_bins - 1 (the voiced half first).  `tables_`: (logw, logZ, lk, ls, logpi) in
    place of T's (the library's own fp32 tables).  In fp32 this follows the kernel bit for bit: every step is one rounded
    add, subtract or max; arg-max at the lowest source; on a tie between the halves the voiced source wins."""
    logw, logZ, lk, ls, logpi = tables_ if tables_ is not None else (T["logw"], T["logZ"], T["lk"], T["ls"], T["logpi"])
    t = dtype
    logw, logZ, lk, ls, logpi = np.asarray(logw, t), np.asarray(logZ, t), t(lk), t(ls), t(logpi)
    lo = np.asarray(log_obs, t)
    F, nb = lo.shape[0], lo.shape[1] - 1
    H = (len(logw) - 1) // 2
    rev = logw[::-1].copy()                                    # window position j is source r = s - H + j: weight logw[2H - j]
    V = np.stack([lo[0, :nb] + logpi, np.full(nb, lo[0, nb] + logpi, t)])
    back = np.zeros((F, 2, nb), np.int64)
    base = np.arange(nb) - H
    for f in range(1, F):
        M, R = [], []
        for h in range(2):
            U = np.full(nb + 2 * H, -np.inf, t)
            U[H:H + nb] = V[h] - logZ
            cand = np.lib.stride_tricks.sliding_window_view(U, 2 * H + 1) + rev[None, :]
            j = cand.argmax(axis=1)                            # the first maximum: the lowest source
            M.append(cand[np.arange(nb), j])
            R.append(base + j)
        new = np.empty_like(V)
        for h in range(2):
            same, other = M[h] + lk, M[1 - h] + ls
            from_same = (same >= other) if h == 0 else (same > other)     # a tie goes to the voiced source
            new[h] = (lo[f, :nb] if h == 0 else lo[f, nb]) + np.where(from_same, same, other)
            src_h = np.where(from_same, h, 1 - h)
            back[f, h] = src_h * nb + np.where(from_same, R[h], R[1 - h])
        V = new - new.max()
    state = np.zeros(F, np.int64)
    state[F - 1] = int(V.reshape(-1).argmax())
    for f in range(F - 1, 0, -1):
        state[f - 1] = back[f].reshape(-1)[state[f]]
    return state


def track(state, T):
    """-> (f0 fp32, voiced bool, bin int: -1 where unvoiced); f0 = freqs[bin], 0 where unvoiced (D3)"""
    nb = T["n_bins"]
    voiced = state < nb
    b = np.where(voiced, state, -1)
    return np.where(voiced, T["freqs"][np.maximum(b, 0)], np.float32(0)).astype(np.float32), voiced, b


def decode(c, T, dtype=np.float64):
    """stages 2-6 on a cmndf -> dict(prob, bin, obs, voiced_prob, log_obs, state, f0, voiced, track_bin)"""
    pr, b = probs(c, T, dtype), bins(c, T)
    obs = scatter(pr, b, T["n_bins"])
    vp, lo = observe(obs, dtype)
    st = viterbi(lo, T, dtype)
    f0, voiced, tb = track(st, T)
    return dict(prob=pr, bin=b, obs=obs, voiced_prob=vp, log_obs=lo, state=st, f0=f0, voiced=voiced, track_bin=tb)


def params(name):
    sr, fl, hop, fmin, fmax, n, seeds, thr = P.CASES[name]
    return dict(sr=sr, fmin=fmin, fmax=fmax, frame_length=fl, hop_length=hop)


@functools.lru_cache(maxsize=None)
def case_tables(name):
    return tables(**(params(name) if name != "octave" else {}))


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (x fp32 [B, L], [fp64 result per row], [fp32 result per row]) for a row of pitch_ref.CASES or "octave"; computed
    once, never modified"""
    if name == "octave":
        x, r64, r32 = octave_signal()[None, :], None, None
        r64 = [P.yin(x[0], dtype=np.float64)]
        r32 = [P.yin(x[0], dtype=np.float32)]
    else:
        x, r64, r32 = P.case(name)
    T = case_tables(name)
    return x, [decode(r["cmndf"], T, np.float64) for r in r64], [decode(r["cmndf"], T, np.float32) for r in r32]


@functools.lru_cache(maxsize=None)
def octave_signal():
    """0.5 s of a 220 Hz tone whose second partial is the loudest and whose odd partials dip to 0.2 of their level for 60 ms:
    plain YIN drops to half the period in the dip"""
    sr, L = OCTAVE["sr"], OCTAVE["L"]
    phi = 2 * np.pi * 220.0 * np.arange(L) / sr
    a1 = np.ones(L)
    a1[L // 2 - 1323:L // 2 + 1323] = 0.2
    win = np.hanning(513)
    a1 = np.convolve(a1, win / win.sum(), "same")
    x = 0.2 * (0.5 * a1 * np.sin(phi) + np.sin(2 * phi) + 0.3 * a1 * np.sin(3 * phi))
    x = (x + 0.002 * np.random.default_rng(OCTAVE["seed"]).standard_normal(L)).astype(np.float32)
    x.setflags(write=False)
    return x


def same_track(a, b):
    """frames on which two decoded tracks differ in (voiced, bin if voiced)"""
    return int(((a["voiced"] != b["voiced"]) | (a["voiced"] & b["voiced"] & (a["track_bin"] != b["track_bin"]))).sum())
