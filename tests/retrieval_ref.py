"""fp64 brute-force restatement of latent retrieval (jatsr_amd.retrieval, csrc/retrieval.hip) in numpy: the stored fp16 rows,
the squared distances in fp64 and in fp32 (the precision of the `faiss.IndexFlatL2` the reference's roadmap names), the arg-min
with the lowest index on equal distance, and the index-rate blend.  Inputs come from recipe.gaussian."""
import functools

import numpy as np

import jatsr_amd.recipe as recipe

# (channels, keys, B, T): ragged in every dimension; five slabs of 4096 with a ragged last one; the micro width
SEARCH_CASES = {"ragged": (1024, 4099, 2, 345), "slabs": (1024, 20011, 1, 130), "micro": (32, 37, 3, 5)}


def normalise(x, mean, std):
    """(x - mean[c]) / std[c] in fp32, channels on axis -2: the expression of jat_channel_affine"""
    x = np.asarray(x, np.float32)
    return ((x - np.asarray(mean, np.float32)[:, None]) / np.asarray(std, np.float32)[:, None]).astype(np.float32)


def pack_rows(src, mean, std, first=0, stride=1, count=None):
    """frames first, first + stride, ... of src [C, len] (fp16 or fp32) -> the stored fp16 rows [count, C]"""
    src = np.asarray(src)
    n = src.shape[1]
    if count is None:
        count = 0 if first >= n else (n - 1 - first) // stride + 1
    frames = first + stride * np.arange(count)
    return np.ascontiguousarray(normalise(src[:, frames].astype(np.float32), mean, std).T).astype(np.float16)


def stats(C, salt=0):
    """four statistics vectors with means and deviations that differ per channel"""
    return {"hr_mean": recipe.gaussian("rt_hr_mean", (C,), salt) * 0.2, "hr_std": np.abs(recipe.gaussian("rt_hr_std", (C,), salt)) + 0.5,
            "lr_mean": recipe.gaussian("rt_lr_mean", (C,), salt) * 0.2, "lr_std": np.abs(recipe.gaussian("rt_lr_std", (C,), salt)) + 0.5}


def queries(x):
    """x [B, C, T] -> [B * T, C]"""
    x = np.asarray(x)
    return np.ascontiguousarray(x.transpose(0, 2, 1)).reshape(-1, x.shape[1])


def dist(q, keys, dtype):
    """d[n, i] = |q_n|^2 + |k_i|^2 - 2 q_n . k_i in `dtype`, on the stored operands (fp32 queries, fp16 keys)"""
    q = np.asarray(q, np.float32).astype(dtype)
    k = np.asarray(keys, np.float16).astype(dtype)
    return ((q * q).sum(1, dtype=dtype)[:, None] + (k * k).sum(1, dtype=dtype)[None, :] - dtype(2) * (q @ k.T)).astype(dtype)


def reference(q, keys):
    """-> dict: d64, the fp64 arg-min (lowest index on ties), the gap to the second best, and
    tol = 4 max|d32 - d64| (the factor covers a different summation order)"""
    d64 = dist(q, keys, np.float64)
    d32 = dist(q, keys, np.float32)
    err = float(np.abs(d32.astype(np.float64) - d64).max())
    best = d64.argmin(1)
    if d64.shape[1] > 1:
        two = np.partition(d64, 1, axis=1)[:, :2]
        gap = two[:, 1] - two[:, 0]
    else:
        gap = np.full(d64.shape[0], np.inf)
    return {"d64": d64, "argmin": best, "gap": gap, "ref_err": err, "tol": 4.0 * err,
            "mismatch32": int((d32.argmin(1) != best).sum())}


@functools.lru_cache(maxsize=None)
def search_case(name):
    """x fp32 [B, C, T] (already normalised), keys fp16 [N, C] and their reference; made once per case"""
    C, N, B, T = SEARCH_CASES[name]
    salt = sorted(SEARCH_CASES).index(name)
    keys = recipe.gaussian("rt_keys", (N, C), salt).astype(np.float16)
    x = recipe.gaussian("rt_queries", (B, C, T), salt)
    ref = reference(queries(x), keys)
    for a in (keys, x):
        a.setflags(write=False)
    return x, keys, ref


def blend(x, rows, idx, rate, mean=None, std=None):
    """y64[b, c, t] = (1 - r) x + r v in fp64 with r the fp32 rate, v = rows[idx[b, t], c] (* std[c] + mean[c]);
    -> (y64, bound) with bound = 6 * 2^-24 (|x| + |v std| + |mean|): six roundings"""
    x64 = np.asarray(x, np.float64)
    v = np.asarray(rows, np.float16).astype(np.float64)[np.asarray(idx)].transpose(0, 2, 1)      # [B, C, T]
    s = np.ones(x64.shape[1]) if std is None else np.asarray(std, np.float64)
    m = np.zeros(x64.shape[1]) if mean is None else np.asarray(mean, np.float64)
    vs = v * s[None, :, None]
    r = float(np.float32(rate))
    y = (1.0 - r) * x64 + r * (vs + m[None, :, None])
    return y, 6.0 * 2.0 ** -24 * (np.abs(x64) + np.abs(vs) + np.abs(m)[None, :, None])
