"""fp64 restatement of the IVF index (include/jat_hip_ivf.h) in numpy, on top of tests/retrieval_ref.py and
tests/retrieval_topk_ref.py: the grouping of rows by list (a stable sort), the probed lists (the nprobe nearest centroids in
(d, index) order), the k nearest rows of the probed lists in (d, position) order, RVC's default number of lists, and the
fixtures the CPU and the GPU tests share."""
import functools
import math

import numpy as np

import jatsr_amd.recipe as recipe
import retrieval_ref as R
import retrieval_topk_ref as TK

MAX_NPROBE = 8


def default_nlist(n):
    """RVC's min(int(16 sqrt(N)), N // 39), floored at 1"""
    return max(1, min(int(16 * math.sqrt(n)), n // 39))


def group(idx, nlist):
    """idx [N] -> (offsets int32 [nlist + 1], order int32 [N]): the stable sort of the rows by list, an idx outside [0, nlist)
    behind all lists; offsets[nlist] is the number of rows that belong to a list"""
    idx = np.asarray(idx).astype(np.int64)
    key = np.where((idx >= 0) & (idx < nlist), idx, nlist)
    order = np.argsort(key, kind="stable").astype(np.int32)
    counts = np.bincount(key, minlength=nlist + 1)[:nlist]
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return offsets, order


def probes(dc, nprobe):
    """dc [n, nlist] (query to centroid) -> int32 [n, nprobe]: the nearest lists in (d, index) order, -1 behind the last list"""
    return TK.topk(dc, nprobe)[0]


def candidates(offsets, probed):
    """the positions of the probed lists of one query, ascending"""
    offsets = np.asarray(offsets)
    pos = [np.arange(offsets[l], offsets[l + 1]) for l in probed if l >= 0]
    return np.sort(np.concatenate(pos)) if pos else np.zeros(0, np.int64)


def search(d, offsets, probed, k):
    """d [n, N] (query to grouped row), probed int32 [n, nprobe] -> (idx int32 [n, k], dist2 [n, k]): per query the first k of
    the probed lists' rows in (d, position) order, dist2 = max(d, 0); beyond the candidates idx -1 and dist2 +inf"""
    d = np.asarray(d)
    idx = np.full((d.shape[0], k), -1, np.int32)
    dist2 = np.full((d.shape[0], k), np.inf, d.dtype)
    for n in range(d.shape[0]):
        pos = candidates(offsets, probed[n])
        if len(pos):
            i, v = TK.topk(d[n:n + 1, pos], k)
            idx[n] = np.where(i[0] >= 0, pos[np.clip(i[0], 0, None)], -1)
            dist2[n] = v[0]
    return idx, dist2


def undecided(d64, offsets, probed, k, tol):
    """bool [n, k]: the ranks of `search` whose fp64 gap to a neighbouring rank among the candidates is within tol (only ranks
    that exist)"""
    out = np.zeros((d64.shape[0], k), bool)
    for n in range(d64.shape[0]):
        pos = candidates(offsets, probed[n])
        if len(pos):
            _, ok = TK.decided(d64[n:n + 1, pos], k, tol)
            out[n, :ok.shape[1]] = ~ok[0]
    return out


# ---- fixtures --------------------------------------------------------------------------------------------------------------
# (channels, lists, rows, B, T, nprobe, k): a mixture with one centre per list; rows and queries scattered around the centres
FP64_CASES = {"wide": (1024, 12, 700, 2, 35, 2, 8), "mid": (96, 51, 2000, 1, 70, 1, 1), "micro": (32, 5, 150, 1, 33, 8, 3)}
FP64_LOOSE = 4      # ranks (lists and rows together) a case may leave inside the near-tie allowance


@functools.lru_cache(maxsize=None)
def fp64_case(name):
    """-> dict: centroids fp16 [nlist, C], rows fp16 [N, C] in their original order, the fp64 assignment, the twin's grouping,
    the grouped rows, x fp32 [B, C, T], and the fp64 results with their tolerances; made once"""
    C, nlist, N, B, T, nprobe, k = FP64_CASES[name]
    salt = sorted(FP64_CASES).index(name)
    cent = (recipe.gaussian("ivf_cent", (nlist, C), salt)).astype(np.float16)
    member = (np.arange(N) * 7919) % nlist
    rows = (cent[member].astype(np.float32) + 0.7 * recipe.gaussian("ivf_rows", (N, C), salt)).astype(np.float16)
    pick = (np.arange(B * T) * 104729) % N
    q = rows[pick].astype(np.float32) + 0.3 * recipe.gaussian("ivf_q", (B * T, C), salt)
    x = np.ascontiguousarray(q.reshape(B, T, C).transpose(0, 2, 1))
    q = R.queries(x)
    aref = R.reference(rows.astype(np.float32), cent)                    # rows to centroids: the assignment
    offsets, order = group(aref["argmin"], nlist)
    grouped = rows[order]
    cref, rref = R.reference(q, cent), R.reference(q, grouped)
    pr = probes(cref["d64"], nprobe)
    idx, dist2 = search(rref["d64"], offsets, pr, k)
    _, pok = TK.decided(cref["d64"], nprobe, cref["tol"])
    loose_rows = undecided(rref["d64"], offsets, pr, k, rref["tol"])
    for a in (cent, rows, x, grouped):
        a.setflags(write=False)
    return {"cent": cent, "rows": rows, "assign": aref["argmin"].astype(np.int32), "assign_gap": aref["gap"], "assign_tol": aref["tol"],
            "offsets": offsets, "order": order, "grouped": grouped, "x": x, "nprobe": nprobe, "k": k, "probes": pr,
            "probes_loose": ~pok, "idx": idx, "dist2": dist2, "loose": loose_rows, "d64": rref["d64"], "tol": rref["tol"]}


# The planted fixture: six centres 16 e_j, rows = centre + 0.25 noise rounded to fp16, the clusters interleaved (row n belongs to
# cluster n mod 6), so the k-means seeds i N // 6 of N = 6 m + 1.. hit clusters that the CPU test checks to be six different ones.
PLANTED = (32, 6, 115)       # channels, clusters, rows: seeds 0, 19, 38, 57, 76, 95 -> clusters 0, 1, 2, 3, 4, 5


@functools.lru_cache(maxsize=None)
def planted():
    C, K, N = PLANTED
    centres = np.zeros((K, C), np.float32)
    centres[np.arange(K), np.arange(K)] = 16.0
    member = np.arange(N) % K
    rows = (centres[member] + 0.25 * recipe.gaussian("ivf_planted", (N, C), 0)).astype(np.float16)
    pick = np.arange(0, N, 3)
    q = rows[pick].astype(np.float32) + 0.01 * recipe.gaussian("ivf_planted_q", (len(pick), C), 0)
    x = np.ascontiguousarray(q.T[None])                                 # [1, C, nq]
    for a in (rows, x):
        a.setflags(write=False)
    return {"centres": centres.astype(np.float16), "member": member.astype(np.int32), "rows": rows, "x": x, "own": pick}


def planted_seeds():
    C, K, N = PLANTED
    return [i * N // K for i in range(K)]
