"""fp64 restatement of top-k latent retrieval (jat_bank_search_topk / jat_bank_blend_topk) in numpy, on top of
tests/retrieval_ref.py: the k nearest rows in (d, index) order, which of their ranks the fp32 arithmetic can decide, the
inverse-square weights in their ratio form and the weighted index-rate blend with its rounding bound."""
import functools

import numpy as np

import retrieval_ref as R

MAX_K = 8
FLOOR = 1e-6


def topk(d, k):
    """d [n, size] -> (idx int32 [n, k], dist2 [n, k]): the first k rows in (d, index) order, dist2 = max(d, 0); size < k
    leaves idx -1 and dist2 +inf behind them"""
    d = np.asarray(d)
    n, size = d.shape
    order = np.argsort(d, axis=1, kind="stable")[:, :k]                  # stable: the lower index first on equal d
    idx = np.full((n, k), -1, np.int32)
    dist2 = np.full((n, k), np.inf, d.dtype)
    m = min(k, size)
    idx[:, :m] = order[:, :m]
    dist2[:, :m] = np.maximum(np.take_along_axis(d, order[:, :m], 1), 0)
    return idx, dist2


def decided(d64, k, tol):
    """-> (sorted d64 [n, min(k + 1, size)], decided bool [n, min(k, size)]): rank j is decided when its fp64 gaps to the
    ranks j - 1 and j + 1 (where they exist) both exceed tol"""
    s = np.sort(np.asarray(d64, np.float64), axis=1)[:, :k + 1]
    m = min(k, s.shape[1])
    gap = np.diff(s, axis=1)                                             # gap[:, j] between ranks j and j + 1
    ok = np.ones((s.shape[0], m), bool)
    for j in range(m):
        if j >= 1:
            ok[:, j] &= gap[:, j - 1] > tol
        if j < gap.shape[1]:
            ok[:, j] &= gap[:, j] > tol
    return s, ok


@functools.lru_cache(maxsize=None)
def topk_case(name):
    """the search case of retrieval_ref with its fp64 top-8 lists and decided ranks; made once"""
    x, keys, ref = R.search_case(name)
    idx, _ = topk(ref["d64"], MAX_K)
    s, ok = decided(ref["d64"], MAX_K, ref["tol"])
    return x, keys, ref, idx, s, ok


def weights(idx, dist2, floor=FLOOR):
    """w [.., k] in fp64 from the fp32 inputs the kernel gets: dt = max(dist2, floor), u = (dt_0 / dt_j)^2 where idx >= 0,
    w = u / sum u; a list without a usable entry has all weights 0"""
    idx = np.asarray(idx)
    dt = np.maximum(np.asarray(dist2, np.float32).astype(np.float64), float(np.float32(floor)))
    with np.errstate(invalid="ignore", divide="ignore"):
        u = np.where(idx >= 0, (dt[..., :1] / dt) ** 2, 0.0)
        S = u.sum(-1, keepdims=True)
        return np.where(S > 0, u / S, 0.0)


def rvc_weights(dist2):
    """square(1 / score) normalised to sum 1, as RVC's index mixes its neighbours"""
    w = np.square(1.0 / np.asarray(dist2, np.float64))
    return w / w.sum(-1, keepdims=True)


# Roundings of the device chain (2^-24 relative each, first order).  A weight: the division dt_0 / dt_j (1), its square (the
# error doubles, 2, and the product rounds, 1), the sum S of k non-negative terms (k - 1 additions, on top of the 3 of each
# term: k + 2), the division by S (1): k + 6.  The value v: the weight (k + 6) and at most k roundings of the fmaf chain, then
# v std (1), + mean (1), rate times that (1), the final sum (1): 2 k + 10 on the sum_j w_j |v_j| |std| term.  mean: its sum,
# the product with the rate, the final sum: 3.  x: 1 - rate (1), the product (1), the final sum (1): 3.  With k <= MAX_K,
# 2 k + 10 <= k + C_BOUND for C_BOUND = MAX_K + 10, and 3 <= k + C_BOUND.
C_WEIGHT = 6
C_BOUND = MAX_K + 10


def blend_topk(x, rows, idx, dist2, rate, mean=None, std=None, floor=FLOOR):
    """y64[b, c, t] = (1 - r) x + r (v std + mean), v = sum_j w_j rows[idx_j] (entries with idx < 0 carry no weight; an
    index >= len(rows) is clamped), in fp64 with r the fp32 rate -> (y64, bound, w) with
    bound = (k + C_BOUND) 2^-24 (sum_j w_j |v_j| |std| + |mean| + |x|)"""
    x64 = np.asarray(x, np.float64)
    idx = np.asarray(idx)
    k = idx.shape[-1]
    w = weights(idx, dist2, floor)                                                            # [B, T, k]
    rows64 = np.asarray(rows, np.float16).astype(np.float64)
    val = rows64[np.clip(idx, 0, len(rows64) - 1)]                                            # [B, T, k, C]
    v = np.einsum("btk,btkc->bct", w, val)
    va = np.einsum("btk,btkc->bct", w, np.abs(val))
    s = np.ones(x64.shape[1]) if std is None else np.asarray(std, np.float64)
    m = np.zeros(x64.shape[1]) if mean is None else np.asarray(mean, np.float64)
    r = float(np.float32(rate))
    y = (1.0 - r) * x64 + r * (v * s[None, :, None] + m[None, :, None])
    bound = (k + C_BOUND) * 2.0 ** -24 * (va * np.abs(s)[None, :, None] + np.abs(m)[None, :, None] + np.abs(x64))
    return y, bound, w
