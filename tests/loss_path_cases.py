"""The cases of the v3mod2 loss launch-path tests, shared by tests/test_loss_paths_cpu.py (which proves that the table reaches
every path of `launch_latent_loss` and that every case's inputs meet the preconditions below) and tests/test_gpu_loss_paths.py
(which runs the kernels on them).  numpy only.

Inputs.  rows = 6 (4 from T = 3000 on), fp32 `recipe.gaussian` draws at the salt recorded with the length:
    row 0   plain                                   row 3   prediction all zeros        (the pm == 0 branches)
    row 1   plain, pred / target / lr x 1000        rows 4, 5  plain
    row 2   pred == target bit for bit              (the e == 0, d == 0, m == 0 branches)
    lr = 0.7 * target + 0.5 * noise

Preconditions.  The loss is not smooth: d loss / d P_k is sign(d) / (|P_k| + 1e-7) per bin and sign(.) per sample, so a
correct fp32 kernel leaves the gate wherever an input sits on a kink or a bin is nearly empty.  The INPUTS keep it inside
(each salt below is the first one of a CPU search, `search_salt`, at which they hold; fp64 numpy only, the kernel is not
consulted):
    min_k |P_k| / rms|P|                               >= 1e-2     rows whose prediction is not zero
    min_k |log(|P_k| + 1e-7) - log(|H_k| + 1e-7)|      >= 2e-5     rows 0, 1, 4, 5
    min_{strict <= k < soft} ||P_k| - |R_k|| / rms|P|  >= 2e-5     rows whose prediction is not zero
    min |pool2(e)|, min |pool4(e)| (and min |e|)       >= 1e-5     rows where pred != target
"""
import math

import numpy as np

import jatsr_amd.recipe as recipe

WEIGHTS = dict(latent_weight=0.3, freq_weight=0.5, ms_weight=0.5, consistency_weight=0.1)
CUTS = dict(low_freq_phase_ratio=0.3, strict_cutoff=0.30, soft_cutoff=0.36)
LDS_LIMIT = 160 * 1024
LOUD, TIE, ZERO = 1, 2, 3          # the special rows

# (T, path, salt) in the order the GPU test runs them.  path: ("fft", N1, N2) or ("direct", FB, NB).
LENGTHS = [
    (4, ("fft", 2, 2), 0), (8, ("fft", 2, 4), 0), (25, ("fft", 5, 5), 0), (35, ("fft", 5, 7), 0), (128, ("fft", 8, 16), 0),
    (346, ("fft", 2, 173), 0), (1377, ("fft", 27, 51), 2), (1722, ("fft", 41, 42), 0), (4096, ("fft", 64, 64), 3),
    (1, ("direct", 1, 2), 0), (2, ("direct", 1, 2), 0), (3, ("direct", 1, 2), 0), (5, ("direct", 1, 2), 0),
    (7, ("direct", 1, 2), 0), (257, ("direct", 1, 2), 0), (431, ("direct", 1, 2), 0), (509, ("direct", 1, 2), 1),
    (521, ("direct", 2, 4), 0), (947, ("direct", 2, 4), 0), (1021, ("direct", 2, 4), 1),
    (1033, ("direct", 3, 6), 1), (1543, ("direct", 3, 6), 3), (2153, ("direct", 3, 6), 2),
    (3418, ("direct", 3, 6), 0),
]
# lengths outside the table that a test runs: the small requests after the largest ones, and the A/B pair
EXTRA = [(23, ("direct", 1, 2), 0), (1378, ("fft", 26, 53), 1)]
SALT = {T: s for T, _, s in LENGTHS + EXTRA}
PATH = {T: p for T, p, _ in LENGTHS + EXTRA}
REJECT_T = 6822
SWEEP_T = (35, 521, 1543)          # the argument sweep: factored, direct, chunked direct


def rows_for(T):
    return 6 if T < 3000 else 4


def width_one_cuts(T):
    """Cut-offs whose transition band is exactly one bin wide (weight torch.linspace(1, 0, 1) = [1])."""
    F = T // 2 + 1
    k = int(F * 0.30)
    cuts = dict(low_freq_phase_ratio=0.3, strict_cutoff=0.30, soft_cutoff=(k + 1.5) / F)
    assert int(F * cuts["soft_cutoff"]) - int(F * cuts["strict_cutoff"]) == 1
    return cuts


def sweep_cuts(T):
    """name -> cut-offs of the argument sweep."""
    return {"band0": dict(low_freq_phase_ratio=0.0, strict_cutoff=0.30, soft_cutoff=0.30),
            "band1": width_one_cuts(T),
            "soft1": dict(low_freq_phase_ratio=0.3, strict_cutoff=0.30, soft_cutoff=1.0)}


def make_inputs(T, salt):
    """-> pred, target, lr as fp32 [1, rows, T]."""
    rows = rows_for(T)
    pred = recipe.gaussian("loss_pred", (1, rows, T), salt + 400)
    target = recipe.gaussian("loss_target", (1, rows, T), salt + 401)
    noise = recipe.gaussian("loss_lr", (1, rows, T), salt + 402)
    for a in (pred, target, noise):
        a[0, LOUD] *= np.float32(1000.0)
    pred[0, TIE] = target[0, TIE]
    pred[0, ZERO] = 0.0
    lr = (0.7 * target + 0.5 * noise).astype(np.float32)
    return pred, target, lr


PRE_BOUNDS = dict(min_mag=1e-2, min_logdiff=2e-5, min_band=2e-5, min_pool=1e-5)


def preconditions(pred, target, lr, cuts=CUTS):
    """The four minima of the module docstring, from fp64 numpy."""
    p, h, r = (np.asarray(a, np.float64)[0] for a in (pred, target, lr))
    rows, T = p.shape
    P, H, R = (np.fft.rfft(a, axis=-1) for a in (p, h, r))
    F = P.shape[-1]
    strict, soft = int(F * cuts["strict_cutoff"]), int(F * cuts["soft_cutoff"])
    nonzero = [i for i in range(rows) if i != ZERO]
    plain = [i for i in range(rows) if i not in (TIE, ZERO)]
    differ = [i for i in range(rows) if i != TIE]
    pm, hm, rm = np.abs(P), np.abs(H), np.abs(R)
    rms = np.sqrt((pm ** 2).mean(-1, keepdims=True))
    rms = np.where(rms > 0, rms, 1.0)                               # the zero row: not indexed below
    out = dict(min_mag=float((pm / rms)[nonzero].min()),
               min_logdiff=float(np.abs(np.log(pm + 1e-7) - np.log(hm + 1e-7))[plain].min()),
               min_band=math.inf, min_pool=math.inf)
    if soft > strict:
        out["min_band"] = float((np.abs(pm - rm) / rms)[nonzero, strict:soft].min())
    e = (p - h)[differ]
    out["min_pool"] = float(np.abs(e).min())
    for s in (2, 4):
        if T // s:
            q = e[:, :T // s * s].reshape(len(differ), T // s, s).mean(-1)
            out["min_pool"] = min(out["min_pool"], float(np.abs(q).min()))
    return out


def preconditions_hold(pre):
    return all(pre[k] >= v for k, v in PRE_BOUNDS.items())


def cuts_of_case(T):
    """Every set of cut-offs a test evaluates length T at."""
    return [CUTS] + (list(sweep_cuts(T).values()) if T in SWEEP_T else [])


def search_salt(T, limit=4096):
    """The first salt at which the inputs of length T meet the preconditions for every set of cut-offs the tests use."""
    for salt in range(limit):
        x = make_inputs(T, salt)
        if all(preconditions_hold(preconditions(*x, cuts=c)) for c in cuts_of_case(T)):
            return salt
    raise AssertionError(f"T = {T}: no salt below {limit} meets the preconditions")


def expected_plan(T, direct_switch=False):
    """Python restatement of `plan_latent_loss` (csrc/train.hip): (kind, a, b, lds_bytes) as jat_k_latent_loss_plan reports
    them."""
    F = T // 2 + 1
    direct = 3 * T * 4 + (T + F) * 8 + 32 * 4                       # three rows, twiddles, g_k, the reduction scratch
    if direct > LDS_LIMIT:
        return 0, 0, 0, direct
    n1 = max(d for d in range(1, math.isqrt(T) + 1) if T % d == 0)  # largest divisor <= sqrt(T)
    if n1 >= 2 and not direct_switch:
        n2 = T // n1
        factored = direct + max(3 * (n1 // 2 + 1) * n2, T) * 8      # + the Y / Z planes
        if factored <= LDS_LIMIT:
            return 2, n1, n2, factored
    if F <= 256 and T <= 512:
        return 1, 1, 2, direct
    if F <= 512 and T <= 1024:
        return 1, 2, 4, direct
    return 1, 3, 6, direct


def is_prime(T):
    return T >= 2 and all(T % d for d in range(2, math.isqrt(T) + 1))


def classes_of(T, plan):
    """The coverage classes (names) a run at length T with plan (kind, a, b, lds) belongs to."""
    kind, a, b, _ = plan
    F = T // 2 + 1
    out = set()
    if kind == 0:
        out.add("rejected")
    elif kind == 1:
        out.add(f"direct<{a},{b}>")
        if (a, b) == (1, 2) and T > 256:
            out.add("direct<1,2> second sample slot")
        if (a, b) == (2, 4) and F > 256:
            out.add("direct<2,4> second bin slot")
        if (a, b) == (3, 6):
            kc, nc = -(-F // (256 * 3)), -(-T // (256 * 6))
            out.add("direct<3,6> one chunk" if (kc, nc) == (1, 1) else "direct<3,6> other")
            if kc >= 2 and nc >= 2:
                out.add("direct<3,6> two or more chunks in both loops")
            if not is_prime(T):
                out.add("direct<3,6> as the LDS fallback of a composite T")
    else:
        out.add("fft N1 == 2" if a == 2 else "fft N1 even > 2" if a % 2 == 0 else "fft N1 odd")
        if a % 2 and b % 2 and a != b:
            out.add("fft odd x odd, N1 != N2")
        if a == 2 and b > 100:
            out.add("fft N1 == 2 with a large N2")
        if T & (T - 1) == 0:
            out.add("fft power of two")
    if kind and int(F * 0.30) == 0 and int(F * 0.36) == 0:
        out.add("empty bands")
    if kind and T // 2 == 0:
        out.add("no pooled samples")
    return out


REQUIRED_CLASSES = {
    "direct<1,2>", "direct<1,2> second sample slot", "direct<2,4>", "direct<2,4> second bin slot", "direct<3,6>",
    "direct<3,6> one chunk", "direct<3,6> two or more chunks in both loops", "direct<3,6> as the LDS fallback of a composite T",
    "rejected", "fft N1 == 2", "fft N1 even > 2", "fft N1 odd", "fft odd x odd, N1 != N2", "fft N1 == 2 with a large N2",
    "fft power of two", "empty bands", "no pooled samples"}
