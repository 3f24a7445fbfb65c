"""Multi-scale latent retrieval on the GPU (jat_bank_add_pooled, jat_bank_pool_frames, jat_bank_mix_scales,
MultiScaleBank, load_bank, sample_long(bank=MultiScaleBank), infer with a format-2 bank file) against the numpy twin of
tests/retrieval_ms_ref.py.

The three kernels are fp32 with one rounding per operation in a fixed order, so every comparison with the fp32 twin is bit for
bit.  The mix is also held against the fp64 evaluation of the same formulas within (n + 8) 2^-24 S (retrieval_ms_ref.mix_bound).
The end-to-end test uses the planted fixture whose margins tests/test_retrieval_ms_cpu.py asserts from fp64 alone: the nearest
row of every pooled query is decided (no query is excused), at k = 1 and as the first column at k = 4; the later ranks of a
k = 4 list carry no planted margin and follow the rule of tests/test_retrieval_topk_gpu.py (a rank whose fp64 gaps to both
neighbours exceed tol = 4 max|d32 - d64| must be fp64's).  The three entries and MultiScaleBank.retrieve also run on a delayed
side stream (tests/stream_check.py), as tests/test_gpu_streams.py does for the entries of include/jat_hip.h."""
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

import retrieval_ms_ref as M  # noqa: E402
import retrieval_ref as R  # noqa: E402
import retrieval_topk_ref as K  # noqa: E402
import jatsr_amd  # noqa: E402
import jatsr_amd.io as jio  # noqa: E402
import jatsr_amd.recipe as recipe  # noqa: E402
from jatsr_amd import _lib as L  # noqa: E402
from jatsr_amd import retrieval as RT  # noqa: E402
from jatsr_amd.retrieval import LatentBank, MultiScaleBank  # noqa: E402
from stream_check import Case, check_case  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV = L.JAT_E_INVALID


def cuda(a):
    return torch.from_numpy(np.array(a)).cuda()


def tstats(C_, salt=0):
    return {k: cuda(v) for k, v in R.stats(C_, salt).items()}


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(t, a):
    """a device tensor against a numpy array of the same dtype, bit for bit"""
    got = t.detach().cpu().numpy()
    return got.shape == a.shape and got.dtype == a.dtype and got.tobytes() == np.ascontiguousarray(a).tobytes()


def raw_add_pooled(bank, key_src, value_src, window, first, stride, count, key_stats, value_stats=(None, None)):
    return L.lib().jat_bank_add_pooled(bank._h, L.ptr(key_src), L.ptr(value_src), int(key_src.dtype == torch.float16),
                                       key_src.shape[1], first, stride, count, window, L.ptr(key_stats[0]), L.ptr(key_stats[1]),
                                       L.ptr(value_stats[0]), L.ptr(value_stats[1]), L.stream_ptr())


def norms_of(rows16):
    """the norms the existing bank_norms_kernel gives these fp16 rows"""
    b = LatentBank(rows16.shape[1], rows16.shape[0])
    b.load_rows(rows16)
    return b.rows("keys")[1].clone()


# ---- 1. the pooled pack ---------------------------------------------------------------------------------------------------
# len = 37.  (first, stride, count): starts 1, 6, .., 36 (the window at 36 is cut to one frame at s = 2, 4, 8; the one at 31 to
# six frames at s = 8), then starts 30 .. 36, appended behind them (rows land at row0 + i; every count from 7 down to 1 at s = 8)
PACK_ADDS = ((1, 5, 8), (30, 1, 7))


@pytest.mark.parametrize("dtype", [np.float16, np.float32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("C_", [32, 96])
def test_pooled_pack_equals_the_twin(C_, dtype):
    n = 37
    st, ts = R.stats(C_, 5), tstats(C_, 5)
    src = (recipe.gaussian("rtms_pack_src", (C_, n), C_) * 2.0).astype(dtype)
    for s in (1, 2, 4, 8):
        b = LatentBank(C_, 40)
        b.load_rows(cuda(np.zeros((3, C_), np.float16)))                              # the first add does not start at row 0
        want = [np.zeros((3, C_), np.float16)]
        for first, stride, count in PACK_ADDS:
            assert first + (count - 1) * stride == n - 1
            assert raw_add_pooled(b, cuda(src), None, s, first, stride, count, (ts["hr_mean"], ts["hr_std"])) == 0
            want.append(M.pool_rows(src, st["hr_mean"], st["hr_std"], first, stride, count, s))
        want = np.concatenate(want)
        rows, norms = b.rows("keys")
        assert len(b) == 18 and same_bits(rows, want), s
        assert torch.equal(bits(norms), bits(norms_of(cuda(want)))), s
    # window = 1 writes what jat_bank_add writes, norms included
    old, new = LatentBank(C_, 20), LatentBank(C_, 20)
    for first, stride, count in PACK_ADDS:
        old.add(cuda(src), ts, first=first, stride=stride, count=count)
        assert raw_add_pooled(new, cuda(src), None, 1, first, stride, count, (ts["hr_mean"], ts["hr_std"])) == 0
    assert torch.equal(bits(old.rows("keys")[0]), bits(new.rows("keys")[0]))
    assert torch.equal(bits(old.rows("keys")[1]), bits(new.rows("keys")[1]))
    assert same_bits(old.rows("keys")[0], np.concatenate([R.pack_rows(src, st["hr_mean"], st["hr_std"], *a) for a in PACK_ADDS]))


@pytest.mark.parametrize("dtype", [np.float16, np.float32], ids=["fp16", "fp32"])
def test_pooled_pack_of_a_paired_bank(dtype):
    C_, n = 96, 37
    st, ts = R.stats(C_, 6), tstats(C_, 6)
    hr = (recipe.gaussian("rtms_pair_hr", (C_, n), 0) * 1.5).astype(dtype)
    lr = (recipe.gaussian("rtms_pair_lr", (C_, n), 1) * 0.7).astype(dtype)
    for s in (2, 4, 8):
        b = LatentBank(C_, 16, key="lr")
        want_k, want_v = [], []
        for first, stride, count in PACK_ADDS:
            b.add(cuda(hr), ts, lr_latent=cuda(lr), first=first, stride=stride, count=count, window=s)       # the wrapper
            want_k.append(M.pool_rows(lr, st["lr_mean"], st["lr_std"], first, stride, count, s))
            want_v.append(M.pool_rows(hr, st["hr_mean"], st["hr_std"], first, stride, count, s))
        assert same_bits(b.rows("keys")[0], np.concatenate(want_k)), s
        assert same_bits(b.rows("values")[0], np.concatenate(want_v)), s
        assert torch.equal(bits(b.rows("keys")[1]), bits(norms_of(cuda(np.concatenate(want_k))))), s


# ---- 2. the pooled queries ------------------------------------------------------------------------------------------------
# T1, T3 (below s = 4 and 8), T33 = 8 * 4 + 1, T = 64; T = 300: a second tile of the kernel, and a partial one
@pytest.mark.parametrize("norm", [False, True], ids=["plain", "stats"])
@pytest.mark.parametrize("C_,T", [(32, 1), (32, 3), (32, 33), (1024, 33), (32, 64), (64, 300)])
def test_pool_frames_equals_the_twin(C_, T, norm):
    B, pad = 2, 64
    st = R.stats(C_, 7)
    x = recipe.gaussian("rtms_pool_x", (B, C_, T), C_ + T) * 1.7 + 0.3
    mean, std = (st["hr_mean"], st["hr_std"]) if norm else (None, None)
    dm, ds = (cuda(mean), cuda(std)) if norm else (None, None)
    xt = cuda(x)
    for scales in ((2, 4, 8), (4,), (2,), (8,), (2, 8)):
        sizes = [B * C_ * M.pooled_length(T, s) for s in scales]
        buf = torch.full((sum(sizes) + pad * (len(sizes) + 1),), float("nan"), device="cuda")
        outs, at = [], pad
        for s, n in zip(scales, sizes):
            outs.append(buf[at:at + n].view(B, C_, M.pooled_length(T, s)))
            at += n + pad
        got = RT.pool_frames(xt, scales, dm, ds, outs=outs)
        assert all(g is o for g, o in zip(got, outs))
        guard = torch.ones_like(buf, dtype=torch.bool)
        for s, o in zip(scales, outs):
            assert same_bits(o, M.pool_queries(x, s, mean, std)), (scales, s)
            lo = (o.data_ptr() - buf.data_ptr()) // 4
            guard[lo:lo + o.numel()] = False
        assert int(guard.sum()) == pad * (len(sizes) + 1) and torch.isnan(buf[guard]).all(), scales
    assert torch.equal(bits(xt), bits(cuda(x)))                                       # x is only read
    fresh = RT.pool_frames(xt, (2, 4, 8), dm, ds)                                     # the wrapper's own buffers
    assert [tuple(f.shape) for f in fresh] == [(B, C_, M.pooled_length(T, s)) for s in (2, 4, 8)]
    assert all(same_bits(f, M.pool_queries(x, s, mean, std)) for f, s in zip(fresh, (2, 4, 8)))


# ---- 3. the mix -----------------------------------------------------------------------------------------------------------
MIX_SCALES = ((1,), (4,), (1, 2), (2, 8), (1, 2, 4), (1, 2, 4, 8))


def mix_inputs(B, C_, T, scales, salt=0):
    x = recipe.gaussian("rtms_mix_x", (B, C_, T), salt) * 2.0
    tracks = [recipe.gaussian(f"rtms_mix_v{s}", (B, C_, M.pooled_length(T, s)), salt) * 1.5 + 0.1 for s in scales]
    return x, tracks, M.scale_weights([3, 1, 2, 5][:len(scales)], len(scales))


# T = 300: a second block along t; (65, 1024, 3): more (b, c) rows than the grid's 65535, the row loop
@pytest.mark.parametrize("B,C_,T", [(2, 33, 1), (2, 33, 3), (2, 33, 33), (1, 32, 300), (65, 1024, 3)])
def test_mix_equals_the_twin_and_stays_within_the_fp64_bound(B, C_, T):
    for scales in (MIX_SCALES if B < 65 else ((1, 2), (4, 8))):
        x, tracks, a = mix_inputs(B, C_, T, scales, T)
        xt, tt = cuda(x), [cuda(v) for v in tracks]
        for rate in (0.0, 0.4, 1.0):
            y = RT.mix_scales(xt, scales, tt, a, rate)
            assert same_bits(y, M.mix(x, scales, tracks, a, rate)), (scales, rate)
            err = np.abs(y.cpu().numpy().astype(np.float64) - M.mix(x, scales, tracks, a, rate, np.float64))
            bound = M.mix_bound(x, scales, tracks, a, rate)
            if B < 65:
                print(f"mix B={B} C={C_} T={T} scales={scales} r={rate}: worst error / bound "
                      f"{(err / np.maximum(bound, 1e-300)).max():.3f}")
            assert (err <= bound).all(), (scales, rate)
            if rate == 0.0:
                assert torch.equal(bits(y), bits(xt))                                  # rate 0: x's bits
            inplace = xt.clone()
            assert RT.mix_scales(inplace, scales, tt, a, rate, out=inplace) is inplace
            assert torch.equal(bits(inplace), bits(y)), (scales, rate)                 # y = x in place
        assert all(torch.equal(bits(t), bits(cuda(v))) for t, v in zip(tt, tracks))    # the tracks are only read


def test_mix_output_stays_inside_its_buffer_and_a_track_may_not_be_y():
    B, C_, T, scales, pad = 2, 32, 33, (1, 2, 4, 8), 64
    x, tracks, a = mix_inputs(B, C_, T, scales, 9)
    xt, tt = cuda(x), [cuda(v) for v in tracks]
    buf = torch.full((B * C_ * T + 2 * pad,), float("nan"), device="cuda")
    out = buf[pad:pad + B * C_ * T].view(B, C_, T)
    RT.mix_scales(xt, scales, tt, a, 0.4, out=out)
    assert same_bits(out, M.mix(x, scales, tracks, a, 0.4)) and torch.isnan(buf[:pad]).all() and torch.isnan(buf[-pad:]).all()
    # a track aliasing y is refused, whole or in part, and nothing is launched
    y = tt[0]
    keep = y.clone()
    with pytest.raises(ValueError, match="overlaps y"):
        RT.mix_scales(xt, scales, tt, a, 0.4, out=y)
    big = torch.zeros(2 * B * C_ * T, device="cuda")
    part_y, part_v = big[:B * C_ * T].view(B, C_, T), big[B * C_ * T - 8:B * C_ * T - 8 + tt[3].numel()].view(tt[3].shape)
    with pytest.raises(ValueError, match="overlaps y"):
        RT.mix_scales(xt, scales, tt[:3] + [part_v], a, 0.4, out=part_y)
    torch.cuda.synchronize()
    assert torch.equal(bits(y), bits(keep)) and (big == 0).all()
    assert RT.mix_scales(xt, scales, [xt] + tt[1:], a, 0.4).shape == xt.shape          # a track may be x: both are only read


@pytest.mark.parametrize("denorm", [False, True], ids=["plain", "denorm"])
def test_mix_of_scale_1_alone_is_the_blend(denorm):
    C_, N, B, T = 96, 211, 2, 45
    rows = recipe.gaussian("rt_blend_rows", (N, C_), 0).astype(np.float16)
    rows[3, :7] = np.float16(-0.0)
    st = R.stats(C_, 3)
    x = recipe.gaussian("rt_blend_x", (B, C_, T), 1) * 2.0
    idx = (np.arange(B * T).reshape(B, T) * 37 % N).astype(np.int32)
    idx[0, 3] = 3
    b = LatentBank(C_, N)
    b.load_rows(cuda(rows))
    v = rows.astype(np.float32)[idx].transpose(0, 2, 1)                                 # [B, C, T], exact
    m, s = (cuda(st["hr_mean"]), cuda(st["hr_std"])) if denorm else (None, None)
    if denorm:
        # the de-normalised value as the blend itself forms it, read out at rate 1 over x = -1: 0 * -1 = -0 and -0 + v = v, every
        # bit of v kept (how the kernel rounds v std + mean is its own affair; the mix takes the track as it comes)
        v = b.blend(torch.full((B, C_, T), -1.0, device="cuda"), cuda(idx), 1.0, m, s).cpu().numpy()
    for rate in (0.0, 0.3, 1.0):
        want = b.blend(cuda(x), cuda(idx), rate, m, s)
        got = RT.mix_scales(cuda(x), (1,), [cuda(np.ascontiguousarray(v))], RT.check_scale_weights(None, 1), rate)
        assert torch.equal(bits(got), bits(want)), rate


# ---- 4. end to end on the planted fixture ---------------------------------------------------------------------------------
E2E_WEIGHTS = [3, 2, 1]


@functools.lru_cache(maxsize=None)
def e2e_bank(key="hr"):
    fx = M.e2e_fixture()
    ts = {k: cuda(v) for k, v in fx["stats"].items()}
    bank = MultiScaleBank(M.E2E_C, 300, scales=M.E2E_SCALES, weights=E2E_WEIGHTS)
    for f, (_, first, stride, count) in zip(fx["files"], M.E2E_FILES):
        assert bank.add(cuda(f), ts, first=first, stride=stride, count=count) == count
    return bank, ts


def composed(bank, x, q, qmean, qstd, ts, k, rate, floor=1e-6):
    """the same retrieval from the EXISTING calls (search / blend, search_topk / blend_topk per scale at rate 1, on twin-pooled
    queries) and the twin's mix -> (y numpy, [idx], [dist2], [track numpy])"""
    qn, xn = q.cpu().numpy(), x.cpu().numpy()
    m, s = (None, None) if qmean is None else (qmean.cpu().numpy(), qstd.cpu().numpy())
    tracks, idxs, dists = [], [], []
    for scale, b in zip(bank.scales, bank.banks):
        if scale == 1:
            qs, mm, ss, base = q, qmean, qstd, x
        else:
            qs, mm, ss = cuda(M.pool_queries(qn, scale, m, s)), None, None
            base = qs
        if k == 1:
            idx, d2 = b.search(qs, mm, ss)
            tr = b.blend(base, idx, 1.0, ts["hr_mean"], ts["hr_std"])
        else:
            idx, d2 = b.search_topk(qs, k, mm, ss)
            tr = b.blend_topk(base, idx, d2, 1.0, ts["hr_mean"], ts["hr_std"], dist2_floor=floor)
        tracks.append(tr.cpu().numpy())
        idxs.append(idx)
        dists.append(d2)
    return M.mix(xn, bank.scales, tracks, np.array(bank.weights, np.float32), rate), idxs, dists, tracks


def test_e2e_bank_rows_are_the_twins():
    bank, _ = e2e_bank()
    fx = M.e2e_fixture()
    assert len(bank) == 300 and bank.scales == (1, 2, 4) and bank.weights == (0.5, float(np.float32(1 / 3)), float(np.float32(1 / 6)))
    for s, b in zip(bank.scales, bank.banks):
        assert len(b) == 300 and same_bits(b.rows("keys")[0], fx["rows"][s]), s


@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("name", sorted(M.E2E_QUERIES))
def test_end_to_end_on_planted_queries(name, k):
    bank, ts = e2e_bank()
    x_np, truth = M.e2e_queries(name)
    ref = M.e2e_brute_force(name)
    x = cuda(x_np)
    y, idxs, dists = bank.retrieve(x, 0.4, stats=ts, k=k, neighbours=True)
    assert len(idxs) == len(dists) == 3 and y.shape == x.shape
    for s, idx, d2 in zip(bank.scales, idxs, dists):
        Ts = M.pooled_length(x.shape[2], s)
        assert tuple(idx.shape) == ((3, Ts) if k == 1 else (3, Ts, 4)) and idx.dtype == torch.int32 and d2.shape == idx.shape
        got = idx.cpu().numpy().reshape(-1, k)
        want = ref[s]["order"][:, :k]
        assert np.array_equal(got[:, 0], truth[s].reshape(-1)) and np.array_equal(got[:, 0], want[:, 0]), s   # every query
        _, ok = K.decided(ref[s]["d64"], k, ref[s]["tol"])
        print(f"{name} k={k} scale {s}: ranks off fp64's {int((got != want).sum())}, undecided {int((~ok).sum())} of {ok.size}")
        assert ok[:, 0].all() and not ((got != want) & ok).any(), s
        at = np.take_along_axis(ref[s]["d64"], got.astype(np.int64), 1)
        assert (np.abs(d2.cpu().numpy().reshape(-1, k) - np.maximum(at, 0)) <= ref[s]["tol"]).all(), s
    want_y, want_i, want_d, _ = composed(bank, x, x, ts["hr_mean"], ts["hr_std"], ts, k, 0.4)
    assert same_bits(y, want_y)
    assert all(torch.equal(a, b) for a, b in zip(idxs, want_i)) and all(torch.equal(bits(a), bits(b)) for a, b in zip(dists, want_d))
    assert torch.equal(bits(bank.retrieve(x, 0.4, stats=ts, k=k)), bits(y))             # without the lists; statistics default
    assert torch.equal(bits(bank.retrieve(x, 0.4, k=k)), bits(y))
    assert torch.equal(bits(bank.retrieve(x, 0.0, k=k)), bits(x))                       # rate 0: x
    assert torch.equal(bits(x), bits(cuda(x_np)))


def test_other_weights_and_the_roadmap_rate():
    bank, ts = e2e_bank()
    x = cuda(M.e2e_queries("tail")[0])
    y = bank.retrieve(x, 0.4, stats=ts)
    try:
        bank.set_weights(None)                                                          # equal weights: the roadmap's form
        r = 0.2
        rate = MultiScaleBank.roadmap_rate(r, 3)
        got = bank.retrieve(x, rate, stats=ts)
        want, _, _, tracks = composed(bank, x, x, ts["hr_mean"], ts["hr_std"], ts, 1, rate)
        assert same_bits(got, want) and not torch.equal(bits(got), bits(y))
        # (x + r sum_s up_s) / (1 + 3 r) from the same tracks, in fp64
        x64 = x.cpu().numpy().astype(np.float64)
        road = (x64 + r * sum(M.interp(v, s, x64.shape[-1], np.float64) for s, v in zip(bank.scales, tracks))) / (1 + 3 * r)
        bound = M.mix_bound(x64, bank.scales, tracks, np.array(bank.weights, np.float32), rate)
        assert (np.abs(got.cpu().numpy() - road) <= bound + 2.0 ** -22 * np.abs(road)).all()      # the weights' and the rate's fp32 rounding
    finally:
        bank.set_weights(E2E_WEIGHTS)
    assert torch.equal(bits(bank.retrieve(x, 0.4, stats=ts)), bits(y))


# ---- 5. key = "lr" --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3])
def test_lr_keys_hr_values(k):
    C_, n, B, T = 32, 150, 2, 27
    st, ts = R.stats(C_, 13), tstats(C_, 13)
    hr = recipe.gaussian("rtms_lr_hr", (C_, n), 0).astype(np.float16)
    lr = recipe.gaussian("rtms_lr_lr", (C_, n), 1).astype(np.float16)
    bank = MultiScaleBank(C_, n, scales=(1, 2, 8), key="lr")
    assert bank.add(cuda(hr), ts, lr_latent=cuda(lr)) == n and len(bank) == n
    for s, b in zip(bank.scales, bank.banks):
        assert same_bits(b.rows("keys")[0], M.pool_rows(lr, st["lr_mean"], st["lr_std"], 0, 1, n, s)), s
        assert same_bits(b.rows("values")[0], M.pool_rows(hr, st["hr_mean"], st["hr_std"], 0, 1, n, s)), s
    pred = cuda(recipe.gaussian("rtms_lr_pred", (B, C_, T), 2))
    query = cuda(lr[:, 40:40 + T].astype(np.float32)[None].repeat(B, 0) + recipe.gaussian("rtms_lr_noise", (B, C_, T), 3) * 0.02)
    y, idxs, dists = bank.retrieve(pred, 0.4, stats=ts, query=query, k=k, neighbours=True)
    want_y, want_i, want_d, _ = composed(bank, pred, query, ts["lr_mean"], ts["lr_std"], ts, k, 0.4)
    assert same_bits(y, want_y) and all(torch.equal(a, b) for a, b in zip(idxs, want_i))
    # the LR stretch is found at every scale: windows 40, 40 + s, ...
    for s, idx in zip(bank.scales, idxs):
        first = idx.reshape(B, -1, k)[..., 0].cpu().numpy()
        full = T // s                                                                    # the cut last window is not planted
        assert np.array_equal(first[:, :full], np.broadcast_to(40 + s * np.arange(full), (B, full))), s
    with pytest.raises(ValueError, match="query"):
        bank.retrieve(pred, 0.4, stats=ts)
    with pytest.raises(ValueError, match="query"):
        bank.retrieve(pred, 0.4, stats=ts, query=query[:, :, :5])
    with pytest.raises(ValueError, match="lr_latent"):
        bank.add(cuda(hr), ts)


# ---- 6. invariance --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 4])
def test_invariance(k):
    bank, ts = e2e_bank()
    x = cuda(M.e2e_queries("tail")[0])
    whole = bank.retrieve(x, 0.4, stats=ts, k=k, neighbours=True)
    again = bank.retrieve(x, 0.4, stats=ts, k=k, neighbours=True)
    assert torch.equal(bits(whole[0]), bits(again[0]))                                  # two runs
    assert all(torch.equal(a, b) for a, b in zip(whole[1], again[1]))
    for row in range(3):                                                                # alone and inside a batch of 3
        alone = bank.retrieve(x[row:row + 1].contiguous(), 0.4, stats=ts, k=k, neighbours=True)
        assert torch.equal(bits(alone[0]), bits(whole[0][row:row + 1])), row
        assert all(torch.equal(a, b[row:row + 1]) for a, b in zip(alone[1], whole[1])), row


# ---- 7. the entries on a delayed side stream ------------------------------------------------------------------------------
def gen(shape, salt, scale=1.0):
    return cuda(recipe.gaussian("rtms_stream", tuple(shape), salt) * scale)


def stream_cases():
    Cc, n, B, T = 32, 120, 2, 37

    def stat_inputs(salt):
        return {k: gen((Cc,), salt + j).abs() * 0.5 + 0.5 for j, k in enumerate(("k_mean", "k_std", "v_mean", "v_std"))}

    def add_pooled():
        inputs = dict(stat_inputs(10), lr_src=gen((Cc, n), 1), hr_src=gen((Cc, n), 2))

        def call(bank, i, o):
            for w in (4, 1):
                rc = raw_add_pooled(bank, i["lr_src"], i["hr_src"], w, 3, 2, 50, (i["k_mean"], i["k_std"]), (i["v_mean"], i["v_std"]))
                assert rc == 0
            assert len(bank) == 100
            return {"rows": bank.rows("keys")[0].clone(), "norms": bank.rows("keys")[1].clone(),
                    "vrows": bank.rows("values")[0].clone()}
        return Case(inputs, call, state=lambda live, outs: LatentBank(Cc, 128, key="lr"))

    def pool():
        inputs = dict(x=gen((B, Cc, 300), 3), mean=gen((Cc,), 4), std=gen((Cc,), 5).abs() + 0.5)
        outs = {f"p{s}": torch.empty(B, Cc, M.pooled_length(300, s), device="cuda") for s in (2, 4, 8)}

        def call(_, i, o):
            RT.pool_frames(i["x"], (2, 4, 8), i["mean"], i["std"], outs=[o["p2"], o["p4"], o["p8"]])
            return {"alone": RT.pool_frames(i["x"], (4,))[0]}
        return Case(inputs, call, outputs=outs)

    def mix():
        scales = (1, 2, 4, 8)
        inputs = {"x": gen((B, Cc, T), 6)}
        inputs.update({f"v{s}": gen((B, Cc, M.pooled_length(T, s)), 7 + s) for s in scales})
        a = RT.check_scale_weights([1, 2, 3, 4], 4)

        def call(_, i, o):
            RT.mix_scales(i["x"], scales, [i[f"v{s}"] for s in scales], a, 0.4, out=o["y"])
            return {"fresh": RT.mix_scales(i["x"], (2, 8), [i["v2"], i["v8"]], a[:2], 0.7)}
        return Case(inputs, call, outputs={"y": torch.empty(B, Cc, T, device="cuda")})

    def retrieve(key, k):
        def state(live, outs):
            st = {k_: gen((Cc,), 20 + j).abs() * 0.5 + 0.5 for j, k_ in enumerate(RT.STAT_KEYS)}
            bank = MultiScaleBank(Cc, n, scales=(1, 2, 4), key=key, weights=[1, 2, 3])
            bank.add(gen((Cc, n), 30), st, lr_latent=gen((Cc, n), 31) if key == "lr" else None)
            return bank

        def call(bank, i, o):
            y, idxs, dists = bank.retrieve(i["x"], 0.4, query=i["query"] if key == "lr" else None, k=k, neighbours=True)
            out = {"y": y}
            out.update({f"idx{j}": v for j, v in enumerate(idxs)})
            out.update({f"dist2{j}": v for j, v in enumerate(dists)})
            return out
        return Case({"x": gen((B, Cc, T), 40), "query": gen((B, Cc, T), 41)}, call, state=state)

    return {"jat_bank_add_pooled": add_pooled, "jat_bank_pool_frames": pool, "jat_bank_mix_scales": mix,
            "MultiScaleBank.retrieve": lambda: retrieve("hr", 1), "MultiScaleBank.retrieve lr k=3": lambda: retrieve("lr", 3)}


def test_every_new_entry_has_a_side_stream_case():
    assert set(L.MS_SIGNATURES) <= set(stream_cases())


@pytest.mark.parametrize("name", ["jat_bank_add_pooled", "jat_bank_pool_frames", "jat_bank_mix_scales", "MultiScaleBank.retrieve",
                                  "MultiScaleBank.retrieve lr k=3"])
def test_side_stream(name):
    """none of the three entries synchronises, and retrieve as a whole keeps the delay pending"""
    check_case(stream_cases()[name](), name, synchronises=False)


# ---- 8. integration -------------------------------------------------------------------------------------------------------
def micro_model():
    cfg = recipe.CONFIGS["micro"]
    m = jatsr_amd.JaT_AudioSR_V3(**cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in recipe.make_state_dict(cfg).items()}, strict=False)
    return m.cuda().eval()


def test_sample_long_with_a_multi_scale_bank():
    m = micro_model()
    Cc, total, chunk, ov = 32, 70, 40, 8
    plan = jatsr_amd.chunk_plan(total, chunk, ov)
    st = tstats(Cc, 21)
    lr = cuda(recipe.gaussian("rt_e2e_lr", (Cc, total), 1) * 1.3 + 0.2)
    noise = [cuda(recipe.gaussian("rt_e2e_noise", (1, Cc, e - s), i)) for i, (s, e) in enumerate(plan)]
    args = (m, lr, st["hr_mean"], st["hr_std"], st["lr_mean"], st["lr_std"])
    kw = dict(num_steps=3, cfg_scale=2.0, chunk_frames=chunk, overlap_frames=ov, noise=noise)
    src = cuda(recipe.gaussian("rt_e2e_bank_hr", (Cc, 300), 2))
    bank = MultiScaleBank(Cc, 300, scales=(1, 2, 4))
    bank.add(src, st)
    plain = jatsr_amd.sample_long(*args, **kw)
    got = jatsr_amd.sample_long(*args, bank=bank, index_rate=0.4, **kw)
    assert torch.equal(bits(got), bits(bank.retrieve(plain, 0.4, stats=st))) and not torch.equal(bits(got), bits(plain))
    got4 = jatsr_amd.sample_long(*args, bank=bank, index_rate=0.4, index_k=4, **kw)
    assert torch.equal(bits(got4), bits(bank.retrieve(plain, 0.4, stats=st, k=4))) and not torch.equal(bits(got4), bits(got))
    assert torch.equal(bits(jatsr_amd.sample_long(*args, bank=bank, index_rate=0.0, **kw)), bits(plain))
    # a bank keyed by LR frames is looked up by the LR input
    lrb = MultiScaleBank(Cc, 300, scales=(2, 4), key="lr")
    lrb.add(src, st, lr_latent=cuda(recipe.gaussian("rt_e2e_bank_lr", (Cc, 300), 3)))
    got_lr = jatsr_amd.sample_long(*args, bank=lrb, index_rate=0.4, **kw)
    assert torch.equal(bits(got_lr), bits(lrb.retrieve(plain, 0.4, stats=st, query=lr[None].float())))
    # a single bank goes the way it always went
    single = LatentBank(Cc, 300)
    single.add(src, st)
    assert torch.equal(bits(jatsr_amd.sample_long(*args, bank=single, index_rate=0.4, **kw)), bits(single.retrieve(plain, 0.4, stats=st)))


def test_scale_1_alone_is_the_single_bank():
    C_, n, B, T = 64, 230, 2, 19
    ts = tstats(C_, 11)
    hr = cuda(recipe.gaussian("rt_pair_hr", (C_, n), 0).astype(np.float16))
    lr = cuda(recipe.gaussian("rt_pair_lr", (C_, n), 1).astype(np.float16))
    pred = cuda(recipe.gaussian("rt_pair_pred", (B, C_, T), 2))
    query = cuda(recipe.gaussian("rt_pair_query", (B, C_, T), 3)) * ts["lr_std"][None, :, None] + ts["lr_mean"][None, :, None]
    for key in ("hr", "lr"):
        single, multi = LatentBank(C_, n, key=key), MultiScaleBank(C_, n, scales=(1,), key=key, weights=[7.0])
        for b in (single, multi):
            b.add(hr, ts, lr_latent=lr if key == "lr" else None, first=2, stride=3)
        assert multi.weights == (1.0,) and len(multi) == len(single) == 76
        assert torch.equal(bits(multi.banks[0].rows("keys")[0]), bits(single.rows("keys")[0]))
        q = query if key == "lr" else None
        for k in (1, 8):
            want = single.retrieve(pred, 0.4, stats=ts, query=q, k=k, neighbours=True)
            got = multi.retrieve(pred, 0.4, stats=ts, query=q, k=k, neighbours=True)
            assert torch.equal(bits(got[0]), bits(want[0])) and torch.equal(got[1][0], want[1])
            assert torch.equal(bits(multi.retrieve(pred, 0.4, stats=ts, query=q, k=k)), bits(want[0]))
        # the single bank itself: search + blend, as ever
        qq, qm, qs = (query, ts["lr_mean"], ts["lr_std"]) if key == "lr" else (pred, ts["hr_mean"], ts["hr_std"])
        i1, _ = single.search(qq, qm, qs)
        assert torch.equal(bits(single.retrieve(pred, 0.4, stats=ts, query=q)), bits(single.blend(pred, i1, 0.4, ts["hr_mean"], ts["hr_std"])))


def test_save_and_load(tmp_path):
    bank, ts = e2e_bank()
    bank.save(tmp_path / "ms.pt")
    d = torch.load(tmp_path / "ms.pt", weights_only=False)
    assert d["format"] == 2 and d["scales"] == [1, 2, 4] and d["weights"] == list(bank.weights) and len(d["banks"]) == 3
    back = RT.load_bank(tmp_path / "ms.pt")
    assert isinstance(back, MultiScaleBank) and back.scales == bank.scales and back.weights == bank.weights
    assert len(back) == 300 and back.key == "hr" and back.channels == M.E2E_C
    for a, b in zip(back.banks, bank.banks):
        assert torch.equal(bits(a.rows("keys")[0]), bits(b.rows("keys")[0]))
        assert torch.equal(bits(a.rows("keys")[1]), bits(b.rows("keys")[1]))            # the norms
    x = cuda(M.e2e_queries("mid")[0])
    assert torch.equal(bits(back.retrieve(x, 0.4, stats=ts, k=4)), bits(bank.retrieve(x, 0.4, stats=ts, k=4)))
    assert isinstance(MultiScaleBank.load(tmp_path / "ms.pt"), MultiScaleBank)
    with pytest.raises(ValueError, match="load_bank"):
        LatentBank.load(tmp_path / "ms.pt")
    bank.banks[0].save(tmp_path / "one.pt")                                              # format 1 loads as a LatentBank
    one = RT.load_bank(tmp_path / "one.pt")
    assert isinstance(one, LatentBank) and len(one) == 300
    with pytest.raises(ValueError, match="format 2"):
        MultiScaleBank.load(tmp_path / "one.pt")
    other = {k: v + 1 for k, v in ts.items()}
    with pytest.raises(ValueError, match="statistics"):
        back.retrieve(x, 0.4, stats=other)
    # a paired bank keeps keys and values
    C_, n = 32, 40
    st = tstats(C_, 3)
    pair = MultiScaleBank(C_, n, scales=(2, 4), key="lr")
    pair.add(gen((C_, n), 50), st, lr_latent=gen((C_, n), 51))
    pair.save(tmp_path / "pair.pt")
    p2 = RT.load_bank(tmp_path / "pair.pt")
    for a, b in zip(p2.banks, pair.banks):
        assert a.key == "lr" and torch.equal(bits(a.rows("keys")[0]), bits(b.rows("keys")[0]))
        assert torch.equal(bits(a.rows("values")[0]), bits(b.rows("values")[0]))


def write_data_dir(root, Cc, lengths):
    os.makedirs(root / "train")
    for i, n in enumerate(lengths):
        jio.save_latent_file(root / "train" / f"f{i}.pt", hr_latent=torch.from_numpy(recipe.gaussian("rtms_dir_hr", (Cc, n), i)),
                             lr_latent=torch.from_numpy(recipe.gaussian("rtms_dir_lr", (Cc, n), i)))
    st = R.stats(Cc, 31)
    (root / "global_stats_separated.json").write_text(json.dumps({k: [float(v) for v in a] for k, a in st.items()}))
    return jio.load_stats(root / "global_stats_separated.json", channels=Cc)


def test_build_command_and_infer_with_a_format_2_file(tmp_path):
    from jatsr_amd.infer import main as infer_main
    cfg = recipe.CONFIGS["micro"]
    Cc, T = cfg["input_channels"], 200
    lengths = [90, 50, 77]
    stats = write_data_dir(tmp_path / "data", Cc, lengths)
    base = ["build", "--data-dir", str(tmp_path / "data"), "--max-frames", "100"]
    RT.main(base + ["--out", str(tmp_path / "ms.pt"), "--scales", "1,2,4"])
    RT.main(base + ["--out", str(tmp_path / "one.pt")])
    ms, one = RT.load_bank(tmp_path / "ms.pt"), RT.load_bank(tmp_path / "one.pt")
    plan = RT.frame_plan(lengths, 100)
    rows = sum(c for _, _, c in plan)
    assert isinstance(ms, MultiScaleBank) and isinstance(one, LatentBank) and len(ms) == len(one) == rows <= 100
    assert torch.load(tmp_path / "one.pt", weights_only=False)["format"] == 1
    assert torch.equal(bits(ms.banks[0].rows("keys")[0]), bits(one.rows("keys")[0]))     # scale 1 is the single bank's file
    want4 = []
    for i, (n, (first, stride, count)) in enumerate(zip(lengths, plan)):                 # one frame_plan for every scale
        hr = recipe.gaussian("rtms_dir_hr", (Cc, n), i).astype(np.float16)
        want4.append(M.pool_rows(hr, stats["hr_mean"].numpy(), stats["hr_std"].numpy(), first, stride, count, 4))
    assert same_bits(ms.banks[2].rows("keys")[0], np.concatenate(want4))
    with pytest.raises(SystemExit):
        RT.main(base + ["--out", str(tmp_path / "bad.pt"), "--scale-weights", "1,2"])    # weights without scales
    with pytest.raises(SystemExit):
        RT.main(base + ["--out", str(tmp_path / "bad.pt"), "--scales", "1,2", "--scale-weights", "1,2,3"])
    assert not os.path.exists(tmp_path / "bad.pt")
    # inference
    torch.save({"model_state_dict": {k: torch.from_numpy(v) for k, v in recipe.make_state_dict(cfg).items()},
                "config": dict(cfg)}, tmp_path / "last.pt")
    jio.save_latent_file(tmp_path / "clip.pt", hr_latent=torch.from_numpy(recipe.gaussian("rt_inf_hr", (Cc, T), 1)),
                         lr_latent=torch.from_numpy(recipe.gaussian("rt_inf_lr", (Cc, T), 2)))
    common = ["--checkpoint", str(tmp_path / "last.pt"), "--input-file", str(tmp_path / "clip.pt"), "--stats-file",
              str(tmp_path / "data" / "global_stats_separated.json"), "--steps", "2", "--cfg-scale", "2.0", "--seed", "3",
              "--index-rate", "0.5"]
    infer_main(common + ["--index-bank", str(tmp_path / "ms.pt"), "--output-dir", str(tmp_path / "ms")])
    infer_main(common + ["--index-bank", str(tmp_path / "ms.pt"), "--output-dir", str(tmp_path / "msw"), "--index-scale-weights",
                         "2,1,1", "--index-k", "4"])
    infer_main(common + ["--index-bank", str(tmp_path / "one.pt"), "--output-dir", str(tmp_path / "one")])
    name = "clip_generated_cfg2.0_idx.pt"
    for d in ("ms", "msw", "one"):
        assert sorted(os.listdir(tmp_path / d)) == ["clip_generated_cfg2.0.pt", name]
    f_ms = torch.load(tmp_path / "ms" / name, weights_only=False)
    f_w = torch.load(tmp_path / "msw" / name, weights_only=False)
    f_one = torch.load(tmp_path / "one" / name, weights_only=False)
    third = float(np.float32(1 / 3))
    assert f_ms["metadata"]["index_scales"] == [1, 2, 4] and f_ms["metadata"]["index_scale_weights"] == [third] * 3
    assert f_ms["metadata"]["index_k"] == 1 and f_ms["metadata"]["bank_rows"] == rows and f_ms["metadata"]["index_rate"] == 0.5
    assert f_w["metadata"]["index_scale_weights"] == [0.5, 0.25, 0.25] and f_w["metadata"]["index_k"] == 4
    assert [tuple(f_w[f"idx_s{s}"].shape) for s in (1, 2, 4)] == [(200, 4), (100, 4), (50, 4)] and "idx" not in f_w
    assert "idx_s1" not in f_ms and f_w["dist2_s4"].dtype == torch.float32
    # with a single bank every file is written as before
    assert sorted(f_one["metadata"]) == ["bank_key", "bank_rows", "index_bank", "index_k", "index_rate", "source"]
    assert sorted(f_one) == ["generated_latent", "metadata"]
    gen_ = torch.load(tmp_path / "ms" / "clip_generated_cfg2.0.pt", weights_only=False)["generated_latent"]
    assert torch.equal(gen_, torch.load(tmp_path / "one" / "clip_generated_cfg2.0.pt", weights_only=False)["generated_latent"])
    assert not torch.equal(f_ms["generated_latent"], f_one["generated_latent"])
    assert not torch.equal(f_ms["generated_latent"], f_w["generated_latent"])
    with pytest.raises(SystemExit, match="multi-scale"):
        infer_main(common + ["--index-bank", str(tmp_path / "one.pt"), "--output-dir", str(tmp_path / "x"), "--index-scale-weights", "1,1"])
    with pytest.raises(SystemExit, match="index-scale-weights"):
        infer_main(common + ["--index-bank", str(tmp_path / "ms.pt"), "--output-dir", str(tmp_path / "x"), "--index-scale-weights", "1,1"])


# ---- 9. the fp16-operand library ------------------------------------------------------------------------------------------
def small_run():
    """the pooled pack (fp16 and fp32 sources), the pooled queries, the mix and retrieve at k = 1 and 3: C = 96"""
    C_, n, B, T = 96, 200, 2, 41
    st = tstats(C_, 51)
    bank = MultiScaleBank(C_, n, scales=(1, 2, 4, 8), weights=[4, 3, 2, 1])
    bank.add(cuda(recipe.gaussian("rtms_lib_bank", (C_, 120), 0)), st)
    bank.add(cuda(recipe.gaussian("rtms_lib_bank", (C_, 80), 1).astype(np.float16)), st)
    x = cuda(recipe.gaussian("rtms_lib_x", (B, C_, T), 1))
    out = {f"rows{s}": b.rows("keys")[0].cpu().numpy() for s, b in zip(bank.scales, bank.banks)}
    out.update({f"norms{s}": b.rows("keys")[1].cpu().numpy() for s, b in zip(bank.scales, bank.banks)})
    out.update({f"pool{s}": p.cpu().numpy() for s, p in zip((2, 4, 8), RT.pool_frames(x, (2, 4, 8), st["hr_mean"], st["hr_std"]))})
    for k in (1, 3):
        y, idxs, dists = bank.retrieve(x, 0.4, stats=st, k=k, neighbours=True)
        out[f"y{k}"] = y.cpu().numpy()
        out.update({f"idx{k}_{s}": i.cpu().numpy() for s, i in zip(bank.scales, idxs)})
        out.update({f"dist2{k}_{s}": d.cpu().numpy() for s, d in zip(bank.scales, dists)})
    return out


def test_fp16_library_gives_the_same_bits(tmp_path):
    """retrieval_ms.hip is fp32 in both builds: libjat_hip_fp16.so (a child process) computes what this process computes"""
    code = ("import sys, numpy as np\n"
            "sys.path.insert(0, 'tests')\n"
            "import jatsr_amd._lib as L\n"
            "from test_retrieval_ms_gpu import small_run\n"
            "assert L.operand_dtype() == 'fp16'\n"
            "np.savez(sys.argv[1], **small_run())\n")
    env = dict(os.environ, JAT_OPERAND_DTYPE="fp16")
    env.pop("JAT_LIB_PATH", None)
    path = str(tmp_path / "fp16.npz")
    out = subprocess.run([sys.executable, "-c", code, path], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
    other, here = dict(np.load(path)), small_run()
    assert sorted(other) == sorted(here) and len(here) == 8 + 3 + 2 * 9
    for k, v in here.items():
        assert v.tobytes() == other[k].tobytes(), k


# ---- 10. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_in_python():
    for bad in ((1, 3), (3,), (1, 1), (2, 2), (4, 2), (1, 2, 4, 8, 8), (), (0,), (16,)):
        with pytest.raises(ValueError, match="scales"):
            MultiScaleBank(32, 10, scales=bad)
    for scales, w in (((1, 2), [1.0]), ((1, 2), [1.0, 1.0, 1.0]), ((1, 2), [1.0, 0.0]), ((1, 2), [1.0, -2.0]), ((1,), [float("nan")]),
                      ((1, 2), [1.0, float("inf")])):
        with pytest.raises(ValueError, match="weights"):
            MultiScaleBank(32, 10, scales=scales, weights=w)
    with pytest.raises(ValueError, match="key"):
        MultiScaleBank(32, 10, key="xx")
    x = gen((1, 32, 9), 60)
    with pytest.raises(ValueError, match="scales"):
        RT.pool_frames(x, (1, 2))                                                       # scale 1 takes no buffer
    with pytest.raises(ValueError, match="scales"):
        RT.pool_frames(x, (3,))
    with pytest.raises(ValueError):
        RT.pool_frames(x, (2,), mean=torch.zeros(32, device="cuda"))                    # mean without std
    with pytest.raises(ValueError, match="outs"):
        RT.pool_frames(x, (2,), outs=[torch.empty(1, 32, 4, device="cuda")])            # ceil(9 / 2) = 5
    with pytest.raises(ValueError):
        RT.pool_frames(x[:, :16].contiguous(), (2,))                                    # 16 channels: refused by the library
    v2 = gen((1, 32, 5), 61)
    with pytest.raises(ValueError, match="tracks"):
        RT.mix_scales(x, (2,), [gen((1, 32, 4), 62)], [1.0], 0.4)
    with pytest.raises(ValueError, match="index_rate"):
        RT.mix_scales(x, (2,), [v2], [1.0], 1.5)
    with pytest.raises(ValueError, match="weights"):
        RT.mix_scales(x, (2,), [v2], [0.0], 0.4)
    with pytest.raises(ValueError):
        RT.mix_scales(x, (2, 4), [v2], [1.0], 0.4)
    b = LatentBank(32, 10)
    with pytest.raises(ValueError, match="window"):
        b.add(gen((32, 20), 63), tstats(32, 1), window=3)
    bank, ts = e2e_bank()
    xq = cuda(M.e2e_queries("mid")[0])
    with pytest.raises(ValueError, match="index_k"):
        bank.retrieve(xq, 0.4, k=9)
    with pytest.raises(ValueError, match="index_rate"):
        bank.retrieve(xq, 1.4)
    with pytest.raises(ValueError, match="dist2_floor"):
        bank.retrieve(xq, 0.4, k=2, dist2_floor=0.0)
    with pytest.raises(ValueError):
        bank.retrieve(xq[:, :32].contiguous(), 0.4)                                     # another channel count
    with pytest.raises(ValueError, match="nothing was added"):
        MultiScaleBank(32, 10).retrieve(gen((1, 32, 9), 64), 0.4)


def test_refusals_through_the_raw_abi():
    lib, s = L.lib(), L.stream_ptr()
    B, C_, T = 1, 32, 9
    x = gen((B, C_, T), 70)
    y = torch.full_like(x, 7.0)
    v = [torch.full((B, C_, M.pooled_length(T, sc)), 5.0, device="cuda") for sc in (1, 2, 4, 8)]
    mean = torch.zeros(C_, device="cuda")

    def ints(*a):
        return (C.c_int32 * len(a))(*a)

    def ptrs(*t):
        return (C.c_void_p * len(t))(*[None if u is None else u.data_ptr() for u in t])

    def floats(*a):
        return (C.c_float * len(a))(*a)

    X, Y = L.ptr(x), L.ptr(y)
    pool = lib.jat_bank_pool_frames
    assert pool(X, None, None, B, C_, T, 1, ints(2), ptrs(v[1]), s) == 0                                  # the good call
    for scales in ((1,), (3,), (16,), (0,), (2, 2), (4, 2), (2, 4, 8, 8)):
        outs = ptrs(*[v[1]] * len(scales))
        assert pool(X, None, None, B, C_, T, len(scales), ints(*scales), outs, s) == INV, scales
    assert pool(X, None, None, B, C_, T, 4, ints(2, 4, 8, 8), ptrs(v[1], v[2], v[3], v[3]), s) == INV       # n > 3 for pooling
    assert pool(X, None, None, B, C_, T, 0, ints(2), ptrs(v[1]), s) == INV
    assert pool(X, None, None, B, C_, T, 1, None, ptrs(v[1]), s) == INV
    assert pool(X, None, None, B, C_, T, 1, ints(2), None, s) == INV
    assert pool(X, None, None, B, C_, T, 1, ints(2), ptrs(None), s) == INV
    assert pool(None, None, None, B, C_, T, 1, ints(2), ptrs(v[1]), s) == INV
    assert pool(X, L.ptr(mean), None, B, C_, T, 1, ints(2), ptrs(v[1]), s) == INV
    assert pool(X, None, None, B, C_, T, 1, ints(2), ptrs(x), s) == INV                                   # an output over x
    for bad in (dict(B=0), dict(T=0), dict(C_=48), dict(C_=16), dict(C_=2048)):
        a = dict(B=B, C_=C_, T=T)
        a.update(bad)
        assert pool(X, None, None, a["B"], a["C_"], a["T"], 1, ints(2), ptrs(v[1]), s) == INV, bad
    mix = lib.jat_bank_mix_scales
    assert mix(X, 2, ints(1, 2), ptrs(v[0], v[1]), floats(0.5, 0.5), 0.4, Y, B, C_, T, s) == 0             # the good call
    torch.cuda.synchronize()
    assert not (y == 7.0).any()
    y.fill_(7.0)
    for scales in ((3,), (0,), (16,), (1, 1), (2, 1), (1, 2, 4, 8, 8)):
        n = len(scales)
        assert mix(X, n, ints(*scales), ptrs(*[v[0]] * n), floats(*[1.0] * n), 0.4, Y, B, C_, T, s) == INV, scales
    assert mix(X, 0, ints(1), ptrs(v[0]), floats(1.0), 0.4, Y, B, C_, T, s) == INV
    for w in (0.0, -1.0, float("nan"), float("inf")):
        assert mix(X, 2, ints(1, 2), ptrs(v[0], v[1]), floats(0.5, w), 0.4, Y, B, C_, T, s) == INV, w
    for rate in (-0.1, 1.5, float("nan")):
        assert mix(X, 1, ints(1), ptrs(v[0]), floats(1.0), rate, Y, B, C_, T, s) == INV, rate
    assert mix(X, 1, ints(1), ptrs(y), floats(1.0), 0.4, Y, B, C_, T, s) == INV                            # a track that is y
    assert mix(X, 1, ints(1), ptrs(None), floats(1.0), 0.4, Y, B, C_, T, s) == INV
    assert mix(X, 1, None, ptrs(v[0]), floats(1.0), 0.4, Y, B, C_, T, s) == INV
    assert mix(X, 1, ints(1), None, floats(1.0), 0.4, Y, B, C_, T, s) == INV
    assert mix(X, 1, ints(1), ptrs(v[0]), None, 0.4, Y, B, C_, T, s) == INV
    assert mix(None, 1, ints(1), ptrs(v[0]), floats(1.0), 0.4, Y, B, C_, T, s) == INV
    assert mix(X, 1, ints(1), ptrs(v[0]), floats(1.0), 0.4, None, B, C_, T, s) == INV
    assert mix(X, 1, ints(1), ptrs(v[0]), floats(1.0), 0.4, Y, B, C_, 0, s) == INV
    assert mix(X, 1, ints(1), ptrs(v[0]), floats(1.0), 0.4, Y, 0, C_, T, s) == INV
    # the pooled add: the checks of jat_bank_add and the window
    b = LatentBank(C_, 8)
    src = gen((C_, 20), 71)
    st = (mean, torch.ones(C_, device="cuda"))
    for window in (0, 3, 16, -2):
        assert raw_add_pooled(b, src, None, window, 0, 1, 4, st) == INV, window
    assert raw_add_pooled(b, src, None, 4, 0, 1, 0, st) == INV                                             # count 0
    assert raw_add_pooled(b, src, None, 4, 20, 1, 1, st) == INV                                            # the start leaves the source
    assert raw_add_pooled(b, src, None, 4, 17, 1, 4, st) == INV
    assert raw_add_pooled(b, src, src, 4, 0, 1, 4, st) == INV                                              # values for an unpaired bank
    assert raw_add_pooled(b, src, None, 4, 0, 1, 4, (None, None)) == INV
    assert raw_add_pooled(b, src, None, 4, 0, 1, 9, st) == L.JAT_E_STATE and len(b) == 0                   # beyond the capacity
    torch.cuda.synchronize()
    assert (y == 7.0).all() and all((t == 5.0).all() for t in v[2:])                                       # nothing was launched
    assert raw_add_pooled(b, src, None, 4, 17, 1, 3, st) == 0 and len(b) == 3                              # starts 17, 18, 19: cut
