"""The normative twin of multi-scale latent retrieval (include/jat_hip_ms.h, csrc/retrieval_ms.hip) in numpy.

Every function takes a `dtype`.  With np.float32 each operation below is ONE rounded fp32 numpy operation in the order the
header fixes, so the result is bit-reproducible and the kernels must equal it bit for bit; with np.float64 the same formulas run
in fp64 on the fp32 inputs (the weights a_i and the rate r keep their fp32 values), which is what the error bound is taken from.

    pooling        q_j = (src_j - mean[c]) / std[c];  window (f, s) of a source of length len: cnt = min(s, len - f),
                   p = (((q_f + q_{f+1}) + ...) + q_{f+cnt-1}) / cnt
    interpolation  s = 1: u = v[t];  else p = (t + 0.5) / s - 0.5, j0 = floor(p), w = p - j0,
                   u = (1 - w) v[clamp(j0)] + w v[clamp(j0 + 1)]
    mix            m = -0; m = m + a_i u_i (i ascending);  y = fma(1 - r, x, r m): r m rounded, then one fused multiply-add,
                   which is what jat_bank_blend's last line computes (`fma32` below is exact, so the twin stays bit-reproducible)

Also here: the planted fixture of the end-to-end test (three synthetic files, a bank of 300 windows per scale, queries cut
from the files plus noise) and its fp64 brute force."""
import functools

import numpy as np

import jatsr_amd.recipe as recipe
import retrieval_ref as R

SCALES = (1, 2, 4, 8)


def scale_weights(weights, n):
    """positive numbers -> fp32 a_i: normalised in fp64 to sum 1, each rounded to fp32; None: all equal"""
    w = np.ones(n, np.float64) if weights is None else np.asarray(weights, np.float64)
    assert w.shape == (n,) and (w > 0).all() and np.isfinite(w).all()
    return (w / w.sum()).astype(np.float32)


def normalise(x, mean, std, dtype):
    """(x - mean[c]) / std[c], channels on axis -2; mean None: x as it is"""
    x = np.asarray(x).astype(np.float32).astype(dtype)
    if mean is None:
        return x
    return ((x - np.asarray(mean, np.float32).astype(dtype)[:, None]) / np.asarray(std, np.float32).astype(dtype)[:, None]).astype(dtype)


def pool(q, starts, s, dtype):
    """q [..., len] -> [..., len(starts)]: the windows of s frames that start at `starts`, cut by the end of the axis"""
    q = np.asarray(q, dtype)
    n = q.shape[-1]
    starts = np.asarray(starts, np.int64)
    assert starts.size == 0 or (starts.min() >= 0 and starts.max() < n)
    acc = q[..., starts]
    for j in range(1, s):
        inside = starts + j < n
        acc = np.where(inside, (acc + q[..., np.minimum(starts + j, n - 1)]).astype(dtype), acc)
    cnt = np.minimum(s, n - starts).astype(dtype)
    return (acc / cnt).astype(dtype)


def pool_rows(src, mean, std, first, stride, count, s, dtype=np.float32):
    """the rows jat_bank_add_pooled stores: [count, C]; fp16 for the fp32 twin, unrounded for fp64"""
    q = normalise(src, mean, std, dtype)
    rows = np.ascontiguousarray(pool(q, first + stride * np.arange(count), s, dtype).T)
    return rows.astype(np.float16) if dtype == np.float32 else rows


def pooled_length(T, s):
    return -(-T // s)


def pool_queries(x, s, mean=None, std=None, dtype=np.float32):
    """x [B, C, T] -> [B, C, ceil(T / s)]: windows at t = 0, s, 2 s, ... of each row"""
    q = normalise(x, mean, std, dtype)
    return pool(q, np.arange(0, q.shape[-1], s), s, dtype)


def taps(T, s):
    """-> (ja, jb, w) of every frame t < T for a track of ceil(T / s) frames; w in fp64 (a dyadic fraction, exact in fp32 too)"""
    Ts = pooled_length(T, s)
    p = (np.arange(T, dtype=np.float64) + 0.5) / s - 0.5
    j0 = np.floor(p)
    w = p - j0
    assert (w.astype(np.float32).astype(np.float64) == w).all()
    j0 = j0.astype(np.int64)
    return np.clip(j0, 0, Ts - 1), np.clip(j0 + 1, 0, Ts - 1), w


def interp(v, s, T, dtype=np.float32):
    """v [..., ceil(T / s)] -> [..., T]"""
    v = np.asarray(v, np.float32).astype(dtype)
    assert v.shape[-1] == pooled_length(T, s)
    if s == 1:
        return v
    ja, jb, w = taps(T, s)
    w = w.astype(dtype)
    return (((dtype(1) - w) * v[..., ja]).astype(dtype) + (w * v[..., jb]).astype(dtype)).astype(dtype)


def fma32(a, b, c):
    """round32(a b + c) with ONE rounding, for fp32 a, b, c: the product is exact in fp64, the sum is rounded to odd there
    (TwoSum gives the error of the fp64 sum), and 53 bits rounded to odd round correctly to 24"""
    p = np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
    c = np.asarray(c, np.float32).astype(np.float64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    s = np.where((e != 0) & even, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def mix(x, scales, tracks, weights, rate, dtype=np.float32):
    """-> y [B, C, T] in `dtype`; weights: the fp32 a_i (scale_weights)"""
    x = np.asarray(x, np.float32).astype(dtype)
    T = x.shape[-1]
    a = np.asarray(weights, np.float32)
    r32 = np.float32(rate)
    keep = dtype(np.float32(1) - r32) if dtype == np.float32 else 1.0 - float(r32)
    m = np.full(x.shape, -0.0, dtype)
    for s, v, ai in zip(scales, tracks, a):
        m = (m + (dtype(ai) * interp(v, s, T, dtype)).astype(dtype)).astype(dtype)
    if dtype == np.float32:
        return fma32(np.broadcast_to(keep, x.shape), x, (r32 * m).astype(np.float32))
    return keep * x + float(r32) * m


def mix_bound(x, scales, tracks, weights, rate):
    """(n + 8) 2^-24 S,  S = |(1 - r) x| + r sum_i a_i ((1 - w) |v_a| + w |v_b|): one rounding per operation on the path
    at most (1 - r, the two products and the sum of a tap pair, a_i u_i, the n sums of m, r m, the last fused multiply-add)"""
    x = np.asarray(x, np.float64)
    T = x.shape[-1]
    r = float(np.float32(rate))
    S = np.abs((1.0 - r) * x)
    for s, v, ai in zip(scales, tracks, np.asarray(weights, np.float32)):
        S = S + r * float(ai) * interp(np.abs(np.asarray(v, np.float32)), s, T, np.float64)
    return (len(scales) + 8) * 2.0 ** -24 * S


# ---- the planted fixture of the end-to-end test ----------------------------------------------------------------------------
E2E_C, E2E_SCALES, E2E_SIGMA = 96, (1, 2, 4), 0.05
# three synthetic files [C, len]: (len, first, stride, count); every file's windows run to its last frame, so the last windows
# of the scales 2 and 4 are cut by the end of the file.  300 windows per scale.
E2E_FILES = ((100, 0, 1, 100), (105, 5, 1, 100), (102, 2, 1, 100))
# query sets: name -> (T, [(file, first frame)] per batch row).  "tail": the last 42 frames of each file, whose last window of
# scale 4 holds 2 frames, as the bank's window at that start does.  "mid": stretches inside the files, T a multiple of 4.
E2E_QUERIES = {"tail": (42, ((0, 58), (1, 63), (2, 60))), "mid": (40, ((0, 12), (1, 29), (2, 41)))}


@functools.lru_cache(maxsize=None)
def e2e_fixture():
    """-> dict: stats, files (de-normalised fp32 [C, len]), rows {scale: fp16 [300, C]} as the twin packs them"""
    st = R.stats(E2E_C, 61)
    files = []
    for i, (n, _, _, _) in enumerate(E2E_FILES):
        g = recipe.gaussian("rtms_e2e_file", (E2E_C, n), i)
        files.append((g * st["hr_std"][:, None] + st["hr_mean"][:, None]).astype(np.float32))
    rows = {s: np.concatenate([pool_rows(f, st["hr_mean"], st["hr_std"], first, stride, count, s)
                               for f, (_, first, stride, count) in zip(files, E2E_FILES)]) for s in E2E_SCALES}
    for a in files + list(rows.values()):
        a.setflags(write=False)
    return {"stats": st, "files": files, "rows": rows}


@functools.lru_cache(maxsize=None)
def e2e_queries(name):
    """-> (x fp32 [B, C, T] de-normalised, truth {scale: int [B, Ts]}): stretches of the files plus noise of sigma 0.05 in
    normalised units; truth[s][b, ts] is the bank row whose window starts where the query's window ts starts"""
    fx = e2e_fixture()
    st = fx["stats"]
    T, where = E2E_QUERIES[name]
    x = np.empty((len(where), E2E_C, T), np.float32)
    truth = {s: np.empty((len(where), pooled_length(T, s)), np.int64) for s in E2E_SCALES}
    row0 = np.cumsum([0] + [f[3] for f in E2E_FILES])
    for b, (f, a) in enumerate(where):
        n, first, stride, count = E2E_FILES[f]
        assert stride == 1 and first <= a and a + T <= n
        noise = recipe.gaussian("rtms_e2e_noise_" + name, (E2E_C, T), b) * E2E_SIGMA
        x[b] = fx["files"][f][:, a:a + T] + (noise * st["hr_std"][:, None]).astype(np.float32)
        for s in E2E_SCALES:
            truth[s][b] = row0[f] + (a + s * np.arange(pooled_length(T, s)) - first)
    x.setflags(write=False)
    return x, truth


@functools.lru_cache(maxsize=None)
def e2e_brute_force(name):
    """-> {scale: dict}: d64 [B * Ts, 300], the fp64 distances of the fp32 pooled queries (the search's operands) to the stored
    fp16 rows; order, by (d, index); sorted, d64 in that order; tol = 4 max|d32 - d64| as in retrieval_ref.reference"""
    fx = e2e_fixture()
    x, _ = e2e_queries(name)
    out = {}
    for s in E2E_SCALES:
        q = R.queries(pool_queries(x, s, fx["stats"]["hr_mean"], fx["stats"]["hr_std"]))
        d = R.dist(q, fx["rows"][s], np.float64)
        order = np.argsort(d, axis=1, kind="stable")
        tol = 4.0 * float(np.abs(R.dist(q, fx["rows"][s], np.float32).astype(np.float64) - d).max())
        out[s] = {"d64": d, "order": order, "sorted": np.take_along_axis(d, order, 1), "tol": tol}
    return out
