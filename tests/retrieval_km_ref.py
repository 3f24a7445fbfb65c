"""numpy twin of k-means compaction (jatsr_amd.retrieval.kmeans, csrc/retrieval_km.hip, include/jat_hip_km.h): the assignment
as an fp64 brute force with the near-tie margin of tests/retrieval_ref.py (gap to the runner-up against tol = 4 max|d32 - d64|),
the update in exact integers as the header defines it, the inertia in fp64, the whole Lloyd loop, and the fixtures the CPU and
GPU tests share.  Inputs come from recipe.gaussian."""
import functools

import numpy as np

import jatsr_amd.recipe as recipe
import retrieval_ref as R

# (N pool rows, K centroids, C): micro; ragged in N and K with more than one centroid tile at the full width; K across
# JAT_BANK_SLAB (4096) and 33 centroid tiles, N = 65 tiles of pool rows and a ragged last one
ASSIGN_CASES = {"micro": (300, 7, 32), "wide": (1031, 130, 1024), "slab": (4200, 4100, 96)}


# ---- assignment -----------------------------------------------------------------------------------------------------------
def assign_reference(pool16, cent16):
    """fp64 brute force over the stored fp16 rows -> the dictionary of retrieval_ref.reference (argmin with the lowest index on
    equal distance, gap to the runner-up, tol) plus `loose`: the rows whose gap is below tol, where either index is allowed"""
    ref = R.reference(np.asarray(pool16, np.float16).astype(np.float32), cent16)
    ref["loose"] = ref["gap"] < ref["tol"]
    return ref


@functools.lru_cache(maxsize=None)
def assign_case(name):
    """pool fp16 [N, C], centroids fp16 [K, C] and their reference; made once per case.  The first centroids are pool rows, as
    in k-means itself (distance 0 to their own row); the rest are independent."""
    N, K, C = ASSIGN_CASES[name]
    salt = sorted(ASSIGN_CASES).index(name)
    pool = recipe.gaussian("km_pool", (N, C), salt).astype(np.float16)
    cent = recipe.gaussian("km_cent", (K, C), salt).astype(np.float16)
    take = min(K, 3)
    cent[:take] = pool[[i * N // take for i in range(take)]]
    ref = assign_reference(pool, cent)
    for a in (pool, cent):
        a.setflags(write=False)
    return pool, cent, ref


# ---- update ---------------------------------------------------------------------------------------------------------------
def units(rows16):
    """finite fp16 values as exact integers in units of 2^-24 (magnitude below 2^40)"""
    v = np.asarray(rows16, np.float16).astype(np.float64) * 2.0 ** 24
    out = v.astype(np.int64)
    assert (out.astype(np.float64) == v).all()
    return out


def mean_row(S, n):
    """fp16_rne(fp32_rne(double_rne(S) / double(n)) 2^-24) per channel, S a sequence of Python integers"""
    q = np.array([float(int(s)) for s in S], np.float64) / np.float64(n)      # int -> float rounds to nearest even
    return (q.astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float16)


def update(cent16, pool16, idx):
    """every centroid with members to the mean of its members; an empty one keeps its row; an idx outside [0, K) joins no
    cluster -> (new rows fp16 [K, C], counts int32 [K])"""
    cent = np.array(cent16, np.float16)
    K = cent.shape[0]
    u = units(pool16)
    idx = np.asarray(idx)
    counts = np.zeros(K, np.int32)
    for i in range(K):
        members = np.nonzero(idx == i)[0]
        counts[i] = len(members)
        if len(members):
            S = [int(v) for v in u[members].sum(0, dtype=np.int64)]          # below 2^62: exact in int64
            assert max(abs(v) for v in S) < 2 ** 62
            cent[i] = mean_row(S, len(members))
    return cent, counts


def seed_positions(N, K):
    return [i * N // K for i in range(K)]


def first_of_equal_rows(rows16):
    """mask [K]: True where no earlier row holds the same bits (a duplicated centroid ties with its first copy by definition)"""
    seen, out = set(), np.zeros(len(rows16), bool)
    for i, r in enumerate(np.asarray(rows16, np.float16)):
        b = r.tobytes()
        out[i] = b not in seen
        seen.add(b)
    return out


def kmeans(pool16, K, iters=10, values16=None, drop_empty=True):
    """the loop of jatsr_amd.retrieval.kmeans with the fp64 assignment -> dict: keys (and values) of the kept centroids, the final
    idx, counts, inertia and changed per iteration, and per iteration the least fp64 gap to a runner-up THAT IS ANOTHER ROW
    (gap) beside the tolerance (tol): where gap > tol in every iteration, an fp32 assignment within tol cannot differ."""
    pool = np.asarray(pool16, np.float16)
    N = pool.shape[0]
    seeds = seed_positions(N, K)
    cent = pool[seeds].copy()
    vals = None if values16 is None else np.asarray(values16, np.float16)[seeds].copy()
    idx = np.full(N, -1, np.int64)
    out = {"inertia": [], "changed": [], "gap": [], "tol": [], "max_abs": []}
    counts = None
    for _ in range(iters):
        ref = R.reference(pool.astype(np.float32), cent)
        d = ref["d64"].copy()
        best = ref["argmin"]
        d[:, ~first_of_equal_rows(cent)] = np.inf
        d[np.arange(N), best] = np.inf
        out["gap"].append(float((d.min(1) - ref["d64"][np.arange(N), best]).min()) if K > 1 else np.inf)
        out["tol"].append(ref["tol"])
        out["max_abs"].append(float(np.abs(cent.astype(np.float64)).max()))
        out["inertia"].append(float(np.maximum(ref["d64"][np.arange(N), best], 0).sum()))
        out["changed"].append(int((best != idx).sum()))
        idx = best.astype(np.int64)
        if out["changed"][-1] == 0:
            break
        cent, counts = update(cent, pool, idx)
        if vals is not None:
            vals, _ = update(vals, values16, idx)
    keep = [i for i in range(K) if counts[i] > 0] if drop_empty else list(range(K))
    out.update(keys=cent[keep], values=None if vals is None else vals[keep], idx=idx, counts=counts, keep=keep)
    return out


# ---- fixtures -------------------------------------------------------------------------------------------------------------
PLANTED = dict(K=24, N=2000, C=96, spread=2.0, noise=0.02)


@functools.lru_cache(maxsize=None)
def planted(duplicates=False):
    """24 well-separated centres, 2000 rows of C = 96: row n belongs to the centre whose seed position i N // K is the last at
    or before n, so every centre is seeded by one of its own rows.  -> (pool fp16, truth [N]).
    duplicates: the rows of centres 0 and 1 are ONE repeated row, so seeds 0 and 1 are equal; the mean of equal rows is that
    row, every one of them ties between centroids 0 and 1 for ever, the lower index takes them and centroid 1 stays empty."""
    K, N, C = PLANTED["K"], PLANTED["N"], PLANTED["C"]
    seeds = np.array(seed_positions(N, K))
    truth = np.searchsorted(seeds, np.arange(N), side="right") - 1
    centres = recipe.gaussian("km_planted_centres", (K, C), 0) * PLANTED["spread"]
    pool = (centres[truth] + recipe.gaussian("km_planted_noise", (N, C), 1) * PLANTED["noise"]).astype(np.float16)
    if duplicates:
        pool[truth <= 1] = pool[0]
        truth = np.where(truth == 1, 0, truth)
    pool.setflags(write=False)
    return pool, truth


def update_case(C, paired, salt=0):
    """a pool of 700 rows of C channels with the edge values of fp16 planted in it, K = 9 and a random idx that leaves
    cluster 4 empty -> (pool keys, pool values or None, centroids, centroid values or None, idx)"""
    N, K = 700, 9
    keys = (recipe.gaussian("km_upd_keys", (N, C), salt + C) * 3.0).astype(np.float16)
    edge = np.array([65504, -65504, 2.0 ** -24, -2.0 ** -24, 0.0, -0.0, 1.0, -1.0], np.float16)
    keys[:64, :8] = edge[(np.arange(64)[:, None] + np.arange(8)[None, :]) % 8]
    keys[5:9, 8:16] = np.float16(-0.0)
    vals = (recipe.gaussian("km_upd_vals", (N, C), salt + C + 1) * 2.0).astype(np.float16) if paired else None
    idx = (np.abs(recipe.gaussian("km_upd_idx", (N,), salt)) * 1000).astype(np.int64) % K
    idx[idx == 4] = 5
    idx[:64] = np.arange(64) % 4                                   # the edge rows spread over clusters 0..3
    idx[5:9] = 8
    cent = recipe.gaussian("km_upd_cent", (K, C), salt).astype(np.float16)
    cvals = recipe.gaussian("km_upd_cvals", (K, C), salt).astype(np.float16) if paired else None
    return keys, vals, cent, cvals, idx.astype(np.int32)
