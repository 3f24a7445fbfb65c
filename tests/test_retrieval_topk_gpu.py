"""Top-k latent retrieval on the GPU (jat_bank_search_topk, jat_bank_blend_topk, LatentBank.search_topk /
blend_topk / retrieve(k=), sample_long(index_k=), infer --index-k) against the fp64 references of tests/retrieval_topk_ref.py.

Search gate.  tol = 4 max|d32 - d64| as in tests/test_gpu_retrieval.py.  For every query and rank: the indexes are distinct rows
of the bank, dist2 does not decrease, |dist2_j - d64[idx_j]| <= tol, |d64[idx_j] - (j-th smallest d64)| <= tol, and wherever the
fp64 gaps of rank j to both neighbouring ranks exceed tol the index is fp64's.  tests/test_retrieval_topk_cpu.py shows from
fp64 alone that at most 1 % of the ranks are left undecided by that rule.

Blend gate.  The inputs are hand-made lists, so the test does not depend on the search.  Weights, read back through a bank
of unit rows, within (k + 6) 2^-24 relative of the fp64 weights; y within (k + 18) 2^-24 (sum_j w_j |v_j| |std| + |mean| + |x|):
the rounding counts are derived next to C_WEIGHT and C_BOUND in tests/retrieval_topk_ref.py."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import retrieval_ref as R  # noqa: E402
import retrieval_topk_ref as K  # noqa: E402
import jatsr_amd  # noqa: E402
import jatsr_amd.io as jio  # noqa: E402
import jatsr_amd.recipe as recipe  # noqa: E402
from jatsr_amd import _lib as L  # noqa: E402
from jatsr_amd.retrieval import LatentBank  # noqa: E402

SLAB = L.BANK_SLAB
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


def cuda(a):
    return torch.from_numpy(np.array(a)).cuda()


def tstats(C_, salt=0):
    return {k: cuda(v) for k, v in R.stats(C_, salt).items()}


def bank_of(rows, capacity=None, values=None):
    """a bank holding exactly these fp16 rows"""
    rows = np.asarray(rows, np.float16)
    b = LatentBank(rows.shape[1], capacity or rows.shape[0], key="hr" if values is None else "lr")
    b.load_rows(cuda(rows), None if values is None else cuda(np.asarray(values, np.float16)))
    return b


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same(a, b):
    """two (idx, dist2) results, bit for bit"""
    return a[0].shape == b[0].shape and torch.equal(a[0], b[0]) and torch.equal(bits(a[1]), bits(b[1]))


@functools.lru_cache(maxsize=None)
def case_bank(case):
    x, keys, _ = R.search_case(case)
    return bank_of(keys), cuda(x)


@functools.lru_cache(maxsize=None)
def gpu_topk(case, k):
    """the kernel's lists for a search case, computed once: (idx [B, T, k], dist2 [B, T, k]) on the device"""
    b, x = case_bank(case)
    return b.search_topk(x, k)


# ---- 1. search against fp64 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 3, 8])
@pytest.mark.parametrize("case", sorted(R.SEARCH_CASES))
def test_search_topk_against_fp64(case, k):
    x, keys, ref, idx64, _, _ = K.topk_case(case)
    C_, N, B, T = R.SEARCH_CASES[case]
    tol, d64 = ref["tol"], ref["d64"]
    s, ok = K.decided(d64, k, tol)
    idx, dist2 = gpu_topk(case, k)
    assert idx.shape == dist2.shape == (B, T, k) and idx.dtype == torch.int32 and dist2.dtype == torch.float32
    idx, dist2 = idx.cpu().numpy().reshape(-1, k), dist2.cpu().numpy().reshape(-1, k).astype(np.float64)
    assert idx.min() >= 0 and idx.max() < N
    srt = np.sort(idx, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all()                                          # distinct rows
    assert (np.diff(dist2, axis=1) >= 0).all() and (dist2 >= 0).all()
    at = np.take_along_axis(d64, idx.astype(np.int64), 1)
    err, rank_err = np.abs(dist2 - at), np.abs(at - s[:, :k])
    wrong = idx != idx64[:, :k]
    print(f"search_topk {case} k={k}: C={C_} keys={N} queries={B}x{T}: tol {tol:.3e}, worst |dist2 - d64[idx]| {err.max():.3e}, "
          f"worst rank-wise |d64[idx_j] - d64 sorted_j| {rank_err.max():.3e}, undecided ranks {int((~ok).sum())} of {ok.size}, "
          f"ranks off fp64's {int(wrong.sum())}")
    assert (err <= tol).all()
    assert (rank_err <= tol).all()
    assert not (wrong & ok).any()


# ---- 2. k = 1, 3. prefixes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(R.SEARCH_CASES))
def test_k1_is_the_search_and_prefixes_are_the_shorter_lists(case):
    b, x = case_bank(case)
    i1, d1 = b.search(x)
    t1 = b.search_topk(x, 1)
    assert t1[0].shape == i1.shape + (1,) and same((t1[0][..., 0], t1[1][..., 0]), (i1, d1))
    i8, d8 = gpu_topk(case, 8)
    assert same((i8[..., :1].contiguous(), d8[..., :1].contiguous()), t1)
    for j in (2, 3, 4):                                                               # list lengths 2, 4 and 4 against 8
        assert same((i8[..., :j].contiguous(), d8[..., :j].contiguous()), b.search_topk(x, j)), j
    for j in (5, 6, 7):                                                               # the same list length, fewer columns
        assert same((i8[..., :j].contiguous(), d8[..., :j].contiguous()), b.search_topk(x, j)), j


# ---- 4. ties --------------------------------------------------------------------------------------------------------------
def test_ties_come_in_index_order():
    C_, N, i = 32, SLAB + 64, 256
    # one lane's consecutive rows, the lane's other half, another wave, another tile, far away, both sides of the slab edge
    planted = [i, i + 1, i + 4, i + 32, i + 128, 1000, SLAB - 1, SLAB, SLAB + 4, SLAB + 34]
    keys = recipe.gaussian("rtk_tie_keys", (N, C_), 0).astype(np.float16)
    for p in planted:
        keys[p] = keys[planted[0]]
    q = np.stack([keys[i].astype(np.float32), keys[7].astype(np.float32)], 1)[None]   # [1, C, 2]: the planted row, a single row
    b = bank_of(keys)
    idx, dist2 = b.search_topk(cuda(q), 8)
    idx, dist2 = idx.cpu().numpy()[0], dist2.cpu().numpy()[0]
    print(f"ties: idx {idx[0].tolist()} dist2 {dist2[0].tolist()}")
    assert idx[0].tolist() == planted[:8]
    assert (dist2[0] == dist2[0, 0]).all() and 0 <= dist2[0, 0] <= R.reference(R.queries(q), keys)["tol"]
    assert idx[1, 0] == 7 and dist2[1, 1] > 1.0
    for k in (2, 4):                                                                  # the shorter lists as well
        ik, _ = b.search_topk(cuda(q), k)
        assert ik.cpu().numpy()[0, 0].tolist() == planted[:k]
    # the last two copies come in once earlier ones are gone: ten equal distances among 4160 rows, the list is the lowest eight
    d64 = R.dist(R.queries(q), keys, np.float64)
    assert np.array_equal(K.topk(d64, 8)[0][0], planted[:8])


# ---- 5. fewer rows than k -------------------------------------------------------------------------------------------------
def test_fewer_rows_than_k():
    C_ = 32
    keys = recipe.gaussian("rtk_few_keys", (3, C_), 0).astype(np.float16)
    x = recipe.gaussian("rtk_few_q", (2, C_, 5), 1)
    b = bank_of(keys, capacity=12)
    idx, dist2 = b.search_topk(cuda(x), 8)
    i_np, d_np = idx.cpu().numpy().reshape(-1, 8), dist2.cpu().numpy().reshape(-1, 8)
    want, _ = K.topk(R.dist(R.queries(x), keys, np.float64), 8)
    assert np.array_equal(i_np, want) and (i_np[:, 3:] == -1).all() and (d_np[:, 3:] == INF).all()
    assert np.isfinite(d_np[:, :3]).all() and (np.diff(d_np[:, :3], axis=1) >= 0).all()
    for k in (2, 3, 5):
        assert same((idx[..., :k].contiguous(), dist2[..., :k].contiguous()), b.search_topk(cuda(x), k))
    y = b.blend_topk(cuda(x), idx, dist2, 0.5).cpu().numpy()
    y64, bound, w = K.blend_topk(x, keys, i_np.reshape(2, 5, 8), d_np.reshape(2, 5, 8), 0.5)
    assert np.isfinite(y).all() and (w[..., 3:] == 0).all() and (np.abs(y - y64) <= bound).all()
    # the tail is not read: the same lists cut to their three valid columns give the same bits
    y3 = b.blend_topk(cuda(x), idx[..., :3].contiguous(), dist2[..., :3].contiguous(), 0.5)
    assert np.array_equal(y3.cpu().numpy().view(np.int32), y.view(np.int32))
    # a bank of one row: the single neighbour has weight 1 and the result is blend's
    one = bank_of(keys[:1], capacity=4)
    st = tstats(C_, 3)
    i8, d8 = one.search_topk(cuda(x), 8)
    assert (i8[..., 0] == 0).all() and (i8[..., 1:] == -1).all() and torch.isinf(d8[..., 1:]).all()
    i1, _ = one.search(cuda(x))
    for m, s in ((None, None), (st["hr_mean"], st["hr_std"])):
        assert torch.equal(bits(one.blend_topk(cuda(x), i8, d8, 0.4, m, s)), bits(one.blend(cuda(x), i1, 0.4, m, s)))


# ---- 6. rows beyond size --------------------------------------------------------------------------------------------------
def test_rows_beyond_size_are_never_returned():
    C_, N, slack = 32, 150, 45
    keys = recipe.gaussian("rt_slack_keys", (N, C_), 0).astype(np.float16)
    q = recipe.gaussian("rt_slack_q", (1, C_, slack), 1).astype(np.float16).astype(np.float32)     # exact in fp16
    b = bank_of(keys, capacity=N + slack)
    full, _ = b.rows("keys", full=True)
    full[N:] = cuda(R.queries(q).astype(np.float16))                   # distance 0 from the queries, if they were ever read
    idx, dist2 = b.search_topk(cuda(q), 8)
    assert int(idx.min()) >= 0 and int(idx.max()) < N and float(dist2.min()) > 1.0
    ref = R.reference(R.queries(q), keys)
    _, ok = K.decided(ref["d64"], 8, ref["tol"])
    want, _ = K.topk(ref["d64"], 8)
    assert not ((idx.cpu().numpy().reshape(-1, 8) != want) & ok).any()
    # the same after clear() and a smaller refill: 5 rows, the lists end there
    b.clear()
    b.load_rows(cuda(keys[:5]))
    q2 = keys[5:45].astype(np.float32).T[None].copy()                  # equal to rows that are no longer part of the bank
    idx2, dist22 = b.search_topk(cuda(q2), 8)
    assert int(idx2[..., :5].min()) >= 0 and int(idx2.max()) < 5 and (idx2[..., 5:] == -1).all()
    assert torch.isinf(dist22[..., 5:]).all() and float(dist22[..., :5].min()) > 1.0


# ---- 7. invariance --------------------------------------------------------------------------------------------------------
def test_invariance():
    C_, N, B, T = 96, SLAB + 517, 3, 77                                # T is no multiple of the query tile
    keys = recipe.gaussian("rt_inv_keys", (N, C_), 0).astype(np.float16)
    st = R.stats(C_, 9)
    raw = cuda(recipe.gaussian("rt_inv_q", (B, C_, T), 1) * st["hr_std"][None, :, None] + st["hr_mean"][None, :, None])
    mean, std = cuda(st["hr_mean"]), cuda(st["hr_std"])
    b = bank_of(keys)
    for k in (4, 8):
        whole = b.search_topk(raw, k, mean, std)
        assert same(b.search_topk(raw, k, mean, std), whole)                                       # two runs
        for row in range(B):                                                                       # alone and inside a batch
            assert same(b.search_topk(raw[row:row + 1].contiguous(), k, mean, std), (whole[0][row:row + 1], whole[1][row:row + 1]))
        shifted = b.search_topk(raw[:, :, 5:].contiguous(), k, mean, std)                          # another place in the tile
        assert same(shifted, (whole[0][:, 5:].contiguous(), whole[1][:, 5:].contiguous()))
        assert same(b.search_topk(jatsr_amd.channel_affine(raw, mean, std), k), whole)             # normalised first
    # the same rows in a bank with more slabs behind them: the split of the key range does not show
    far = recipe.gaussian("rt_inv_far", (2 * SLAB, C_), 2).astype(np.float16) * 4 + 30
    big = bank_of(np.concatenate([keys, far]))
    assert same(big.search_topk(raw, 8, mean, std), b.search_topk(raw, 8, mean, std))


# ---- 8. buffer bounds -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 8])
def test_outputs_stay_inside_their_buffers(k):
    C_, N, B, T = 32, SLAB + 70, 2, 33
    b = bank_of(recipe.gaussian("rt_can_keys", (N, C_), 0).astype(np.float16))
    x = cuda(recipe.gaussian("rt_can_q", (B, C_, T), 1))
    pad, n = 32, B * T * k
    ibuf = torch.full((n + 2 * pad,), -12345, dtype=torch.int32, device="cuda")
    dbuf = torch.full((n + 2 * pad,), float("nan"), device="cuda")
    need = b.topk_workspace_bytes(B * T, k)
    assert need >= 2 * B * T * (4 if k == 3 else 8) * 8 and need % 256 == 0
    assert b.topk_workspace_bytes(B * T, 1) == b.workspace_bytes(B * T)
    work = torch.full((need + 512,), 0x5A, dtype=torch.uint8, device="cuda")
    ip, dp = C.c_void_p(ibuf.data_ptr() + 4 * pad), C.c_void_p(dbuf.data_ptr() + 4 * pad)
    L.check(L.lib().jat_bank_search_topk(b._h, L.ptr(x), None, None, B, T, k, ip, dp, L.ptr(work), need, L.stream_ptr()))
    want_i, want_d = b.search_topk(x, k)
    assert torch.equal(ibuf[pad:pad + n], want_i.view(-1)) and torch.equal(bits(dbuf[pad:pad + n]), bits(want_d.view(-1)))
    assert (ibuf[:pad] == -12345).all() and (ibuf[-pad:] == -12345).all()
    assert torch.isnan(dbuf[:pad]).all() and torch.isnan(dbuf[-pad:]).all()
    assert (work[need:] == 0x5A).all()
    ibuf[pad:pad + n] = -12345                                                         # dist2 may be NULL
    L.check(L.lib().jat_bank_search_topk(b._h, L.ptr(x), None, None, B, T, k, ip, None, L.ptr(work), need, L.stream_ptr()))
    assert torch.equal(ibuf[pad:pad + n], want_i.view(-1))
    # the blend's output inside a larger buffer
    ybuf = torch.full((B * C_ * T + 2 * pad,), float("nan"), device="cuda")
    out = ybuf[pad:pad + B * C_ * T].view(B, C_, T)
    b.blend_topk(x, want_i, want_d, 0.4, out=out)
    assert torch.isnan(ybuf[:pad]).all() and torch.isnan(ybuf[-pad:]).all() and torch.isfinite(out).all()


# ---- 9. blend against fp64 on hand-made lists -----------------------------------------------------------------------------
def hand_lists(N, k, B=2):
    """idx int32 / dist2 fp32 [B, T, k]: the hand-made rows first, then random ascending lists; T = 37"""
    rows = [[0, 1e-9, 1e-6, 1, 2, 3, 4, 5],                    # the floor: the first three count as 1e-6
            [1, 2, 4, 8, 16, 32, 64, 128],
            [1e-3, 1e3, 2e3, 3e3, 4e3, 5e3, 6e3, 7e3],
            [1e30, 1e30, 2e30, 2e30, 3e30, 4e30, 5e30, 6e30],  # a plain 1 / d^2 is 0 / 0 here
            [1, 2, 3, INF, INF, INF, INF, INF],                 # unused places from the fourth on
            [0.5, INF, INF, INF, INF, INF, INF, INF],           # one neighbour
            [0, 0, 0, 0, 0, 0, 0, 0]]                           # exact hits only
    rng = np.random.RandomState(11 + k)
    T = 37
    d = np.empty((B, T, 8), np.float32)
    d[:, :len(rows)] = np.array(rows, np.float32)[None]
    d[:, len(rows):] = np.sort(rng.uniform(900, 1200, size=(B, T - len(rows), 8)), axis=-1)
    idx = np.stack([np.stack([rng.permutation(N)[:8] for _ in range(T)]) for _ in range(B)]).astype(np.int32)
    idx[np.isinf(d)] = -1
    return idx[..., :k].copy(), d[..., :k].copy()


@pytest.mark.parametrize("k", [2, 5, 8])
def test_blend_topk_weights(k):
    """a bank of unit rows at rate 1 returns the weights themselves: y[b, idx_j, t] = w_j"""
    C_ = 32
    b = bank_of(np.eye(C_, dtype=np.float16))
    idx, d = hand_lists(C_, k)
    B, T = idx.shape[:2]
    y = b.blend_topk(torch.zeros(B, C_, T, device="cuda"), cuda(idx), cuda(d), 1.0).cpu().numpy().astype(np.float64)
    w64 = K.weights(idx, d)
    got = np.take_along_axis(y.transpose(0, 2, 1), np.clip(idx, 0, None).astype(np.int64), 2)          # [B, T, k]
    got = np.where(idx >= 0, got, 0.0)
    assert np.abs(w64.sum(-1) - 1).max() < 1e-12
    assert np.abs(y.sum(1) - 1).max() <= (2 * k + K.C_WEIGHT) * 2.0 ** -24            # nothing lands anywhere else
    rel = np.abs(got - w64) / np.maximum(w64, 1e-300)
    print(f"blend_topk weights k={k}: worst |w - w64| / w64 = {rel.max() / 2.0 ** -24:.2f} x 2^-24 (bound {k + K.C_WEIGHT})")
    assert (np.abs(got - w64) <= (k + K.C_WEIGHT) * 2.0 ** -24 * w64 + 1e-45).all()
    assert np.allclose(got[:, 0, :min(k, 3)], 1.0 / min(k, 3), rtol=1e-6)             # the floor row
    assert (got[:, 5, 0] == 1.0).all()                                                # one neighbour: exactly 1


@pytest.mark.parametrize("denorm", [False, True], ids=["plain", "denorm"])
@pytest.mark.parametrize("k", [2, 5, 8])
@pytest.mark.parametrize("C_", [32, 1024])
def test_blend_topk_against_fp64(C_, k, denorm):
    N = 53
    rows = recipe.gaussian("rtk_blend_rows", (N, C_), C_).astype(np.float16)
    st = R.stats(C_, 3)
    idx, d = hand_lists(N, k)
    idx[1, 10, 0] = N + 5                                                             # clamped into the bank
    B, T = idx.shape[:2]
    x = recipe.gaussian("rtk_blend_x", (B, C_, T), 1) * 2.0
    b = bank_of(rows)
    xt, it, dt = cuda(x), cuda(idx), cuda(d)
    m, s = (cuda(st["hr_mean"]), cuda(st["hr_std"])) if denorm else (None, None)
    assert torch.equal(bits(b.blend_topk(xt, it, dt, 0.0, m, s)), bits(xt))            # rate 0: x bit for bit
    for rate in (0.4, 1.0):
        y64, bound, _ = K.blend_topk(x, rows, idx, d, rate, st["hr_mean"] if denorm else None, st["hr_std"] if denorm else None)
        y = b.blend_topk(xt, it, dt, rate, m, s)
        err = np.abs(y.cpu().numpy().astype(np.float64) - y64)
        print(f"blend_topk C={C_} k={k} denorm={denorm} r={rate}: worst error / bound {(err / bound).max():.3f}")
        assert np.isfinite(y64).all() and (err <= bound).all()
        inplace = xt.clone()
        assert b.blend_topk(inplace, it, dt, rate, m, s, out=inplace) is inplace and torch.equal(bits(inplace), bits(y))
    # another floor: every hand-made distance below it counts as it
    y64, bound, _ = K.blend_topk(x, rows, idx, d, 0.4, st["hr_mean"] if denorm else None, st["hr_std"] if denorm else None, floor=2.5)
    y = b.blend_topk(xt, it, dt, 0.4, m, s, dist2_floor=2.5)
    assert (np.abs(y.cpu().numpy().astype(np.float64) - y64) <= bound).all()


# ---- 10. k = 1 is the blend -----------------------------------------------------------------------------------------------
def test_blend_topk_k1_is_the_blend():
    C_, N, B, T = 96, 211, 2, 45
    rows = recipe.gaussian("rt_blend_rows", (N, C_), 0).astype(np.float16)
    rows[3, :7] = np.float16(-0.0)                                                    # the sign of a zero is kept too
    st = tstats(C_, 3)
    x = cuda(recipe.gaussian("rt_blend_x", (B, C_, T), 1) * 2.0)
    x[0, :7, 3] = -0.0
    idx = (np.arange(B * T).reshape(B, T) * 37 % N).astype(np.int32)
    idx[0, 0], idx[1, -1], idx[0, 3] = N - 1, 0, 3
    d = np.abs(recipe.gaussian("rtk_k1_d", (B, T, 1), 2)).astype(np.float32) * 1e3
    d[0, 1], d[0, 2] = 0.0, 1e30
    b = bank_of(rows)
    for rate in (0.0, 0.3, 1.0):
        for m, s in ((None, None), (st["hr_mean"], st["hr_std"])):
            want = b.blend(x, cuda(idx), rate, m, s)
            assert torch.equal(bits(b.blend_topk(x, cuda(idx[..., None]), cuda(d), rate, m, s)), bits(want)), (rate, m is None)


# ---- 11. wrappers ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["hr", "lr"])
def test_retrieve_is_search_topk_then_blend_topk(key):
    C_, n, B, T = 64, 230, 2, 19
    ts = tstats(C_, 11)
    hr = cuda(recipe.gaussian("rt_pair_hr", (C_, n), 0).astype(np.float16))
    lr = cuda(recipe.gaussian("rt_pair_lr", (C_, n), 1).astype(np.float16))
    b = LatentBank(C_, n, key=key)
    b.add(hr, ts, lr_latent=lr if key == "lr" else None)
    pred = cuda(recipe.gaussian("rt_pair_pred", (B, C_, T), 2))
    query = cuda(recipe.gaussian("rt_pair_query", (B, C_, T), 3)) * ts["lr_std"][None, :, None] + ts["lr_mean"][None, :, None]
    q, qm, qs = (query, ts["lr_mean"], ts["lr_std"]) if key == "lr" else (pred, ts["hr_mean"], ts["hr_std"])
    idx, dist2 = b.search_topk(q, 8, qm, qs)
    want = b.blend_topk(pred, idx, dist2, 0.4, ts["hr_mean"], ts["hr_std"])
    got, gi, gd = b.retrieve(pred, 0.4, stats=ts, query=query if key == "lr" else None, k=8, neighbours=True)
    assert torch.equal(bits(got), bits(want)) and same((gi, gd), (idx, dist2))
    assert torch.equal(bits(b.retrieve(pred, 0.4, stats=ts, query=query if key == "lr" else None, k=8)), bits(want))
    # k = 1: the calls of before
    i1, _ = b.search(q, qm, qs)
    old = b.blend(pred, i1, 0.4, ts["hr_mean"], ts["hr_std"])
    assert torch.equal(bits(b.retrieve(pred, 0.4, stats=ts, query=query if key == "lr" else None)), bits(old))
    assert torch.equal(bits(b.retrieve(pred, 0.4, stats=ts, query=query if key == "lr" else None, k=1)), bits(old))
    assert not torch.equal(bits(old), bits(want))
    with pytest.raises(ValueError, match="index_k"):
        b.retrieve(pred, 0.4, stats=ts, query=query, k=9)
    with pytest.raises(ValueError, match="dist2_floor"):
        b.retrieve(pred, 0.4, stats=ts, query=query, k=4, dist2_floor=0.0)


def micro_model():
    cfg = recipe.CONFIGS["micro"]
    m = jatsr_amd.JaT_AudioSR_V3(**cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in recipe.make_state_dict(cfg).items()}, strict=False)
    return m.cuda().eval()


def test_sample_long_with_index_k():
    m = micro_model()
    Cc, total, chunk, ov = 32, 70, 40, 8
    plan = jatsr_amd.chunk_plan(total, chunk, ov)
    st = tstats(Cc, 21)
    lr = cuda(recipe.gaussian("rt_e2e_lr", (Cc, total), 1) * 1.3 + 0.2)
    noise = [cuda(recipe.gaussian("rt_e2e_noise", (1, Cc, e - s), i)) for i, (s, e) in enumerate(plan)]
    args = (m, lr, st["hr_mean"], st["hr_std"], st["lr_mean"], st["lr_std"])
    kw = dict(num_steps=3, cfg_scale=2.0, chunk_frames=chunk, overlap_frames=ov, noise=noise)
    bank = LatentBank(Cc, 300)
    bank.add(cuda(recipe.gaussian("rt_e2e_bank_hr", (Cc, 300), 2)), st)
    plain = jatsr_amd.sample_long(*args, **kw)
    got = jatsr_amd.sample_long(*args, bank=bank, index_rate=0.4, index_k=4, **kw)
    assert torch.equal(bits(got), bits(bank.retrieve(plain, 0.4, stats=st, k=4)))
    one = jatsr_amd.sample_long(*args, bank=bank, index_rate=0.4, index_k=1, **kw)
    assert torch.equal(bits(one), bits(jatsr_amd.sample_long(*args, bank=bank, index_rate=0.4, **kw)))
    assert torch.equal(bits(one), bits(bank.retrieve(plain, 0.4, stats=st))) and not torch.equal(bits(one), bits(got))
    assert torch.equal(bits(jatsr_amd.sample_long(*args, bank=bank, index_rate=0.0, index_k=4, **kw)), bits(plain))


def test_infer_with_index_k(tmp_path):
    from jatsr_amd.infer import main as infer_main
    cfg = recipe.CONFIGS["micro"]
    Cc, T = cfg["input_channels"], 200
    torch.save({"model_state_dict": {k: torch.from_numpy(v) for k, v in recipe.make_state_dict(cfg).items()},
                "config": dict(cfg)}, tmp_path / "last.pt")
    jio.save_latent_file(tmp_path / "clip.pt", hr_latent=torch.from_numpy(recipe.gaussian("rt_inf_hr", (Cc, T), 1)),
                         lr_latent=torch.from_numpy(recipe.gaussian("rt_inf_lr", (Cc, T), 2)))
    st = R.stats(Cc, 31)
    (tmp_path / "stats.json").write_text(json.dumps({k: [float(v) for v in a] for k, a in st.items()}))
    stats = jio.load_stats(tmp_path / "stats.json", channels=Cc)
    bank = LatentBank(Cc, 120)
    bank.add(cuda(recipe.gaussian("rt_inf_bank", (Cc, 120), 3)), stats)
    bank.save(tmp_path / "bank.pt")
    base = ["--checkpoint", str(tmp_path / "last.pt"), "--input-file", str(tmp_path / "clip.pt"), "--stats-file",
            str(tmp_path / "stats.json"), "--steps", "2", "--cfg-scale", "2.0", "--seed", "3", "--index-bank",
            str(tmp_path / "bank.pt"), "--index-rate", "0.5"]
    infer_main(base + ["--output-dir", str(tmp_path / "k1")])
    infer_main(base + ["--output-dir", str(tmp_path / "k4"), "--index-k", "4"])
    name = "clip_generated_cfg2.0_idx.pt"
    assert sorted(os.listdir(tmp_path / "k4")) == ["clip_generated_cfg2.0.pt", name]
    one = torch.load(tmp_path / "k1" / name, weights_only=False)
    four = torch.load(tmp_path / "k4" / name, weights_only=False)
    assert one["metadata"]["index_k"] == 1 and "idx" not in one and "dist2" not in one
    assert four["metadata"]["index_k"] == 4 and four["metadata"]["index_rate"] == 0.5
    assert four["idx"].shape == four["dist2"].shape == (T, 4) and four["idx"].dtype == torch.int32
    assert four["dist2"].dtype == torch.float32 and int(four["idx"].min()) >= 0 and int(four["idx"].max()) < 120
    assert four["generated_latent"].shape == one["generated_latent"].shape == (Cc, T)
    assert not torch.equal(four["generated_latent"], one["generated_latent"])
    # the file is retrieve(k=4) of the generated latent the other file holds, up to its fp16 storage
    gen = torch.load(tmp_path / "k4" / "clip_generated_cfg2.0.pt", weights_only=False)["generated_latent"]
    assert torch.equal(gen, torch.load(tmp_path / "k1" / "clip_generated_cfg2.0.pt", weights_only=False)["generated_latent"])


# ---- 12. argument errors --------------------------------------------------------------------------------------------------
def test_argument_errors():
    C_, N = 32, 20
    b = bank_of(recipe.gaussian("rt_err_keys", (N, C_), 0).astype(np.float16))
    x = cuda(recipe.gaussian("rt_err_q", (1, C_, 8), 1))
    k = 4
    idx = torch.full((8, k), -7, dtype=torch.int32, device="cuda")
    d = torch.ones(8, k, device="cuda")
    y = torch.full_like(x, 7.0)
    need = b.topk_workspace_bytes(8, k)
    work = torch.zeros(need + 8, dtype=torch.uint8, device="cuda")
    lib, h, s = L.lib(), b._h, L.stream_ptr()
    INV = L.JAT_E_INVALID
    X, I, D, W, Y = L.ptr(x), L.ptr(idx), L.ptr(d), L.ptr(work), L.ptr(y)
    n = C.c_size_t()
    for bad_k in (0, 9, -1):
        assert lib.jat_bank_topk_workspace_bytes(h, 8, bad_k, C.byref(n)) == INV
        assert lib.jat_bank_search_topk(h, X, None, None, 1, 8, bad_k, I, None, W, need, s) == INV
        assert lib.jat_bank_blend_topk(h, X, I, D, bad_k, None, None, 0.5, 1e-6, Y, 1, 8, s) == INV
    assert lib.jat_bank_topk_workspace_bytes(h, 0, k, C.byref(n)) == INV
    assert lib.jat_bank_topk_workspace_bytes(h, 8, k, None) == INV
    assert lib.jat_bank_search_topk(h, None, None, None, 1, 8, k, I, None, W, need, s) == INV                # null x
    assert lib.jat_bank_search_topk(h, X, None, None, 1, 8, k, None, None, W, need, s) == INV                # null idx
    assert lib.jat_bank_search_topk(h, X, None, None, 1, 8, k, I, None, None, need, s) == INV                # null workspace
    assert lib.jat_bank_search_topk(h, X, X, None, 1, 8, k, I, None, W, need, s) == INV                      # mean without std
    assert lib.jat_bank_search_topk(h, X, None, None, 1, 0, k, I, None, W, need, s) == INV                   # T = 0
    assert lib.jat_bank_search_topk(h, X, None, None, 0, 8, k, I, None, W, need, s) == INV
    assert lib.jat_bank_search_topk(h, X, None, None, 1, 8, k, I, None, W, need - 1, s) == INV               # workspace too small
    assert lib.jat_bank_search_topk(h, X, None, None, 1, 8, k, I, None, C.c_void_p(work.data_ptr() + 4), need, s) == INV
    # the workspace follows the list length: 1, 2, 4, 4, 8 for k = 1, 2, 3, 4, 5
    sizes = [b.topk_workspace_bytes(1000, kk) for kk in (1, 2, 3, 4, 5, 8)]
    assert sizes == [8192, 16128, 32000, 32000, 64000, 64000] and sizes[0] == b.workspace_bytes(1000)
    assert lib.jat_bank_blend_topk(h, None, I, D, k, None, None, 0.5, 1e-6, Y, 1, 8, s) == INV
    assert lib.jat_bank_blend_topk(h, X, None, D, k, None, None, 0.5, 1e-6, Y, 1, 8, s) == INV
    assert lib.jat_bank_blend_topk(h, X, I, None, k, None, None, 0.5, 1e-6, Y, 1, 8, s) == INV               # null dist2
    assert lib.jat_bank_blend_topk(h, X, I, D, k, None, None, 0.5, 1e-6, None, 1, 8, s) == INV
    assert lib.jat_bank_blend_topk(h, X, I, D, k, X, None, 0.5, 1e-6, Y, 1, 8, s) == INV                     # mean without std
    assert lib.jat_bank_blend_topk(h, X, I, D, k, None, None, 1.5, 1e-6, Y, 1, 8, s) == INV
    assert lib.jat_bank_blend_topk(h, X, I, D, k, None, None, 0.5, 1e-6, Y, 1, 0, s) == INV
    for floor in (0.0, -1.0, float("nan")):
        assert lib.jat_bank_blend_topk(h, X, I, D, k, None, None, 0.5, floor, Y, 1, 8, s) == INV
    empty = LatentBank(C_, 4)
    assert lib.jat_bank_search_topk(empty._h, X, None, None, 1, 8, k, I, None, W, need, s) == L.JAT_E_STATE
    assert lib.jat_bank_blend_topk(empty._h, X, I, D, k, None, None, 0.5, 1e-6, Y, 1, 8, s) == L.JAT_E_STATE
    torch.cuda.synchronize()
    assert (idx == -7).all() and (y == 7.0).all()                              # nothing was launched
    with pytest.raises(ValueError, match="index_k"):
        b.search_topk(x, 0)
    with pytest.raises(ValueError, match="index_k"):
        b.search_topk(x, 9)
    with pytest.raises(ValueError):
        b.search_topk(x[:, :16].contiguous(), 4)                               # another channel count
    good_i, good_d = b.search_topk(x, k)
    with pytest.raises(ValueError, match="dist2_floor"):
        b.blend_topk(x, good_i, good_d, 0.4, dist2_floor=float("nan"))
    with pytest.raises(ValueError, match="index_rate"):
        b.blend_topk(x, good_i, good_d, -0.1)
    with pytest.raises(ValueError):
        b.blend_topk(x, good_i[..., 0], good_d[..., 0], 0.4)                   # lists without their k axis
    with pytest.raises(ValueError):
        b.blend_topk(x, good_i, good_d[..., :2], 0.4)                          # dist2 of another shape


# ---- 13. the fp16-operand library -----------------------------------------------------------------------------------------
def small_run():
    """search_topk at every list length with the normalisation in the loader, the de-normalising blend_topk: C = 96, a bank
    across a slab edge"""
    C_, n, B, T = 96, SLAB + 300, 2, 41
    st = tstats(C_, 51)
    b = LatentBank(C_, n)
    b.add(cuda(recipe.gaussian("rtk_lib_bank", (C_, n), 0)), st)
    x = cuda(recipe.gaussian("rtk_lib_x", (B, C_, T), 1))
    out = {}
    for k in (2, 3, 8):
        idx, dist2 = b.search_topk(x, k, st["hr_mean"], st["hr_std"])
        y = b.blend_topk(x, idx, dist2, 0.4, st["hr_mean"], st["hr_std"])
        out.update({f"idx{k}": idx.cpu().numpy(), f"dist2{k}": dist2.cpu().numpy(), f"y{k}": y.cpu().numpy()})
    return out


def test_fp16_library_gives_the_same_bits(tmp_path):
    """retrieval.hip uses fp16 MFMA in both builds: libjat_hip_fp16.so (a child process) computes what this process computes"""
    code = ("import sys, numpy as np\n"
            "sys.path.insert(0, 'tests')\n"
            "import jatsr_amd._lib as L\n"
            "from test_retrieval_topk_gpu import small_run\n"
            "assert L.operand_dtype() == 'fp16'\n"
            "np.savez(sys.argv[1], **small_run())\n")
    env = dict(os.environ, JAT_OPERAND_DTYPE="fp16")
    env.pop("JAT_LIB_PATH", None)
    path = str(tmp_path / "fp16.npz")
    out = subprocess.run([sys.executable, "-c", code, path], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
    other, here = dict(np.load(path)), small_run()
    assert sorted(other) == sorted(here) and len(here) == 9
    for k, v in here.items():
        assert v.tobytes() == other[k].tobytes(), k
