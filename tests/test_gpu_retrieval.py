"""Latent retrieval on the GPU (csrc/retrieval.hip behind the jat_bank_* entry points; jatsr_amd.retrieval) against the fp64
brute force of tests/retrieval_ref.py.

Search gate.  tol = 4 max|d32 - d64| over the case's whole distance matrix, d32 the same formula in numpy fp32 on the same
stored operands: measured from the two references inside the test.  Required: |dist2 - d64[idx]| <= tol for every query,
idx == argmin d64 wherever the fp64 gap between best and second best exceeds 2 tol, and at most 1 % of all queries off the
fp64 arg-min.  Measured on MI355X (the kernel's worst |dist2 - d64[idx]| / tol): see DESIGN 19."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import retrieval_ref as R  # noqa: E402
import jatsr_amd  # noqa: E402
import jatsr_amd.io as jio  # noqa: E402
import jatsr_amd.recipe as recipe  # noqa: E402
from jatsr_amd import _lib as L  # noqa: E402
from jatsr_amd.retrieval import LatentBank, frame_plan  # noqa: E402

SLAB = L.BANK_SLAB
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


# ---- pack ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float16, np.float32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("C_,n,first,stride,count", [(1024, 97, 3, 2, 45), (32, 70, 0, 1, 70), (96, 333, 5, 7, 33), (64, 1, 0, 1, 1),
                                                    (32, 40, 39, 5, 1)])
def test_pack_rows_and_norms(dtype, C_, n, first, stride, count):
    st = R.stats(C_, C_ + n)
    src = (recipe.gaussian("rt_pack", (C_, n), n) * 1.5 + 0.1).astype(dtype)
    CANARY = 0x7BCD
    b = LatentBank(C_, count + 9, key="hr")
    full, _ = b.rows("keys", full=True)
    full.view(torch.int16).fill_(CANARY)
    pre = b.add(cuda(recipe.gaussian("rt_pack0", (C_, 4), 1).astype(dtype)), tstats(C_, C_ + n))       # rows 0..3: an offset start
    assert pre == 4 and len(b) == 4
    assert b.add(cuda(src), tstats(C_, C_ + n), first=first, stride=stride, count=count) == count
    assert len(b) == 4 + count
    want = R.pack_rows(src, st["hr_mean"], st["hr_std"], first, stride, count)
    rows, norms = b.rows("keys")
    got = rows.cpu().numpy()
    assert got.shape == (4 + count, C_) and got.dtype == np.float16
    assert np.array_equal(got[4:].view(np.uint16), want.view(np.uint16))                  # bit for bit
    n64 = (want.astype(np.float64) ** 2).sum(1)
    err = np.abs(norms.cpu().numpy()[4:].astype(np.float64) - n64)
    print(f"pack C={C_} count={count}: worst norm error / (C 2^-24 |row|^2) = {(err / (C_ * 2.0 ** -24 * n64)).max():.3f}")
    assert (err <= C_ * 2.0 ** -24 * n64).all()
    # overflow is refused and leaves the bank as it was; the slack rows keep their canaries
    with pytest.raises(L.JatError):
        b.add(cuda(src[:, :1].repeat(6, axis=1)), tstats(C_, C_ + n), count=6)
    assert len(b) == 4 + count
    full, _ = b.rows("keys", full=True)
    after = full.cpu().numpy()
    assert np.array_equal(after[4:4 + count].view(np.uint16), want.view(np.uint16))
    assert (after[4 + count:].view(np.uint16) == CANARY).all()
    with pytest.raises(ValueError):
        b.add(cuda(src), tstats(C_, C_ + n), first=first, stride=stride, count=count + (n - 1 - first) // stride + 1)   # past the source


def test_load_rows_recomputes_the_same_norms():
    C_ = 96
    st = tstats(C_, 5)
    a = LatentBank(C_, 50)
    a.add(cuda(recipe.gaussian("rt_load", (C_, 50), 0)), st)
    rows, norms = a.rows()
    b = LatentBank(C_, 60)
    b.load_rows(rows[:7])
    b.load_rows(rows[7:])
    r2, n2 = b.rows()
    assert torch.equal(bits(r2), bits(rows)) and torch.equal(bits(n2), bits(norms))


# ---- search against fp64 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(R.SEARCH_CASES))
def test_search_against_fp64(case):
    x, keys, ref = R.search_case(case)
    C_, N, B, T = R.SEARCH_CASES[case]
    if case == "slabs":
        assert N > 4 * SLAB and N % SLAB not in (0,) and N % 128 != 0        # five slabs, the last one ragged
    assert ref["mismatch32"] == 0                                            # the fp32 reference alone finds every arg-min
    idx, dist2 = bank_of(keys).search(cuda(x))
    idx, dist2 = idx.cpu().numpy().reshape(-1), dist2.cpu().numpy().reshape(-1).astype(np.float64)
    assert idx.min() >= 0 and idx.max() < N
    tol = ref["tol"]
    err = np.abs(dist2 - ref["d64"][np.arange(idx.size), idx])
    close = ref["gap"] <= 2 * tol
    wrong = idx != ref["argmin"]
    print(f"search {case}: C={C_} keys={N} queries={B}x{T}: reference error {ref['ref_err']:.3e}, tol {tol:.3e}, kernel worst "
          f"|dist2 - d64[idx]| {err.max():.3e}, queries with gap <= 2 tol {close.mean() * 100:.2f} % (smallest gap "
          f"{ref['gap'].min():.3e}), off the fp64 arg-min {int(wrong.sum())}")
    assert (err <= tol).all()
    assert not (wrong & ~close).any()
    assert wrong.mean() <= 0.01


def test_exact_integer_rows_and_an_asymmetric_operand():
    """The fp16 operand lane map on exact data: small integers (every product and sum exact in fp32), rows that differ in one
    channel each, so a swapped or permuted operand element would move the arg-min and the distance."""
    C_, N = 64, 300
    rng = np.random.RandomState(7)
    keys = rng.randint(-3, 4, size=(N, C_)).astype(np.float16)
    q = rng.randint(-3, 4, size=(2, C_, 37)).astype(np.float32)
    q[1] += (np.arange(C_, dtype=np.float32) % 5)[:, None]                   # asymmetric in the channel index
    d64 = R.dist(R.queries(q), keys, np.float64)
    idx, dist2 = bank_of(keys).search(cuda(q))
    idx, dist2 = idx.cpu().numpy().reshape(-1), dist2.cpu().numpy().reshape(-1)
    assert np.array_equal(idx, d64.argmin(1))                                # ties included: numpy's argmin is the lowest index
    assert np.array_equal(dist2.astype(np.float64), d64.min(1))              # exact


# ---- ties and bounds ----------------------------------------------------------------------------------------------------
def test_ties_return_the_lowest_index():
    C_, N = 64, 2 * SLAB + 300
    keys = recipe.gaussian("rt_tie_keys", (N, C_), 0).astype(np.float16)
    groups = [[5, 200, SLAB + 77, 2 * SLAB + 150],       # tiles and slabs apart
              [SLAB + 130, 2 * SLAB + 3],                # first copy in the second slab
              [2 * SLAB + 3 + 32, 2 * SLAB + 3 + 70],    # one tile, two waves
              [301, 305, 333],                           # one wave: the two lane halves, two register groups
              [N - 1, 4]]                                # the very last row of the ragged slab and an early one
    for g in groups:
        for i in g[1:]:
            keys[i] = keys[g[0]]
    q = np.stack([keys[g[0]].astype(np.float32) for g in groups], 1)[None]          # [1, C, 5]
    ref = R.reference(R.queries(q), keys)
    idx, dist2 = bank_of(keys).search(cuda(q))
    idx, dist2 = idx.cpu().numpy().reshape(-1), dist2.cpu().numpy().reshape(-1)
    want = [min(i for i in range(N) if np.array_equal(keys[i], keys[g[0]])) for g in groups]
    print(f"ties: idx {idx.tolist()} want {want}, dist2 {dist2.tolist()}, tol {ref['tol']:.3e}")
    assert idx.tolist() == want
    assert (dist2 >= 0).all() and (dist2 <= ref["tol"]).all()


def test_rows_beyond_size_are_never_returned():
    C_, N, slack = 32, 150, 45
    keys = recipe.gaussian("rt_slack_keys", (N, C_), 0).astype(np.float16)
    q = recipe.gaussian("rt_slack_q", (1, C_, slack), 1).astype(np.float16).astype(np.float32)     # exact in fp16
    b = bank_of(keys, capacity=N + slack)
    full, _ = b.rows("keys", full=True)
    full[N:] = cuda(R.queries(q).astype(np.float16))                   # distance 0 from the queries, if they were ever read
    idx, dist2 = b.search(cuda(q))
    ref = R.reference(R.queries(q), keys)
    assert int(idx.max()) < N and np.array_equal(idx.cpu().numpy().reshape(-1), ref["argmin"])
    assert float(dist2.min()) > 1.0
    # the same after clear() and a smaller refill: the rows of the first fill lie behind the new size
    b.clear()
    assert len(b) == 0
    b.load_rows(cuda(keys[:20]))
    assert len(b) == 20
    q2 = keys[20:60].astype(np.float32).T[None].copy()                 # equal to rows that are no longer part of the bank
    idx2, _ = b.search(cuda(q2))
    assert int(idx2.max()) < 20
    assert np.array_equal(idx2.cpu().numpy().reshape(-1), R.reference(R.queries(q2), keys[:20])["argmin"])


def test_bank_of_one_row():
    C_ = 32
    key = recipe.gaussian("rt_one", (1, C_), 0).astype(np.float16)
    q = recipe.gaussian("rt_one_q", (2, C_, 3), 1)
    qs = R.queries(q).astype(np.float64)
    k = key.astype(np.float64)[0]
    d64 = ((qs - k) ** 2).sum(1)
    # three fp32 sums of C terms each (|q|^2, |k|^2, q.k): at most C 2^-24 of the sum of their magnitudes, whatever the order
    bound = C_ * 2.0 ** -24 * ((qs ** 2).sum(1) + (k ** 2).sum() + 2 * np.abs(qs * k).sum(1))
    idx, dist2 = bank_of(key).search(cuda(q))
    assert int(idx.abs().max()) == 0
    assert (np.abs(dist2.cpu().numpy().reshape(-1) - d64) <= bound).all()


# ---- invariance ---------------------------------------------------------------------------------------------------------
def test_invariance_and_loader_normalisation():
    C_, N, B, T = 96, SLAB + 517, 3, 77
    keys = recipe.gaussian("rt_inv_keys", (N, C_), 0).astype(np.float16)
    st = R.stats(C_, 9)
    raw = cuda(recipe.gaussian("rt_inv_q", (B, C_, T), 1) * st["hr_std"][None, :, None] + st["hr_mean"][None, :, None])
    mean, std = cuda(st["hr_mean"]), cuda(st["hr_std"])
    b = bank_of(keys)
    idx, d = b.search(raw, mean, std)
    idx_again, d_again = b.search(raw, mean, std)
    assert torch.equal(idx, idx_again) and torch.equal(bits(d), bits(d_again))                 # two runs
    for row in range(B):                                                                       # alone and inside a batch
        i1, d1 = b.search(raw[row:row + 1].contiguous(), mean, std)
        assert torch.equal(i1[0], idx[row]) and torch.equal(bits(d1[0]), bits(d[row]))
    i2, d2 = b.search(jatsr_amd.channel_affine(raw, mean, std))                                # normalised first, plain search
    assert torch.equal(i2, idx) and torch.equal(bits(d2), bits(d))
    ref = R.reference(R.queries(R.normalise(raw.cpu().numpy(), st["hr_mean"], st["hr_std"])), keys)
    wrong = idx.cpu().numpy().reshape(-1) != ref["argmin"]
    assert not (wrong & (ref["gap"] > 2 * ref["tol"])).any()


# ---- blend --------------------------------------------------------------------------------------------------------------
def test_blend():
    C_, N, B, T = 96, 211, 2, 45
    rows = recipe.gaussian("rt_blend_rows", (N, C_), 0).astype(np.float16)
    st = R.stats(C_, 3)
    mean, std = cuda(st["hr_mean"]), cuda(st["hr_std"])
    x = recipe.gaussian("rt_blend_x", (B, C_, T), 1) * 2.0
    idx = (np.arange(B * T).reshape(B, T) * 37 % N).astype(np.int32)
    idx[0, 0], idx[1, -1] = N - 1, 0
    b = bank_of(rows)
    xt, it = cuda(x), cuda(idx)
    # r = 0: x bit for bit, also in place; r = 1: the stored value exactly
    assert torch.equal(bits(b.blend(xt, it, 0.0)), bits(xt))
    assert torch.equal(bits(b.blend(xt, it, 0.0, mean, std)), bits(xt))
    alias = xt.clone()
    assert b.blend(alias, it, 0.0, out=alias) is alias and torch.equal(bits(alias), bits(xt))
    v = rows.astype(np.float32)[idx].transpose(0, 2, 1)
    assert np.array_equal(b.blend(xt, it, 1.0).cpu().numpy(), v)
    for rate in (0.3, 0.5):
        for m, s in ((None, None), (mean, std)):
            y64, bound = R.blend(x, rows, idx, rate, None if m is None else st["hr_mean"], None if s is None else st["hr_std"])
            # canaries around y: the output sits inside a larger buffer
            pad = 64
            buf = torch.full((B * C_ * T + 2 * pad,), float("nan"), device="cuda")
            out = buf[pad:pad + B * C_ * T].view(B, C_, T)
            y = b.blend(xt, it, rate, m, s, out=out)
            assert torch.isnan(buf[:pad]).all() and torch.isnan(buf[-pad:]).all()
            err = np.abs(y.cpu().numpy().astype(np.float64) - y64)
            print(f"blend r={rate} denorm={m is not None}: worst error / bound {(err / bound).max():.3f}")
            assert (err <= bound).all()
            inplace = xt.clone()
            b.blend(inplace, it, rate, m, s, out=inplace)
            assert torch.equal(bits(inplace), bits(y))


def test_search_outputs_stay_inside_their_buffers():
    C_, N, B, T = 32, 70, 2, 33
    b = bank_of(recipe.gaussian("rt_can_keys", (N, C_), 0).astype(np.float16))
    x = cuda(recipe.gaussian("rt_can_q", (B, C_, T), 1))
    pad, n = 32, B * T
    ibuf = torch.full((n + 2 * pad,), -12345, dtype=torch.int32, device="cuda")
    dbuf = torch.full((n + 2 * pad,), float("nan"), device="cuda")
    need = b.workspace_bytes(n)
    work = torch.full((need + 512,), 0x5A, dtype=torch.uint8, device="cuda")
    L.check(L.lib().jat_bank_search(b._h, L.ptr(x), None, None, B, T, C.c_void_p(ibuf.data_ptr() + 4 * pad),
                                    C.c_void_p(dbuf.data_ptr() + 4 * pad), L.ptr(work), need, L.stream_ptr()))
    want_i, want_d = b.search(x)
    assert torch.equal(ibuf[pad:pad + n], want_i.view(-1)) and torch.equal(bits(dbuf[pad:pad + n]), bits(want_d.view(-1)))
    assert (ibuf[:pad] == -12345).all() and (ibuf[-pad:] == -12345).all()
    assert torch.isnan(dbuf[:pad]).all() and torch.isnan(dbuf[-pad:]).all()
    assert (work[need:] == 0x5A).all()
    # dist2 may be NULL
    L.check(L.lib().jat_bank_search(b._h, L.ptr(x), None, None, B, T, C.c_void_p(ibuf.data_ptr() + 4 * pad), None, L.ptr(work),
                                    need, L.stream_ptr()))
    assert torch.equal(ibuf[pad:pad + n], want_i.view(-1))


# ---- key = "lr" ---------------------------------------------------------------------------------------------------------
def test_lr_keys_return_hr_values():
    C_, n, B, T = 64, 230, 2, 19
    st = R.stats(C_, 11)
    ts = tstats(C_, 11)
    hr = recipe.gaussian("rt_pair_hr", (C_, n), 0).astype(np.float16)
    lr = recipe.gaussian("rt_pair_lr", (C_, n), 1).astype(np.float16)
    b = LatentBank(C_, 200, key="lr")
    count = b.add(cuda(hr), ts, lr_latent=cuda(lr), first=1, stride=2, count=100)
    assert count == 100 == len(b)
    krows = R.pack_rows(lr, st["lr_mean"], st["lr_std"], 1, 2, 100)
    vrows = R.pack_rows(hr, st["hr_mean"], st["hr_std"], 1, 2, 100)
    assert np.array_equal(b.rows("keys")[0].cpu().numpy().view(np.uint16), krows.view(np.uint16))
    assert np.array_equal(b.rows("values")[0].cpu().numpy().view(np.uint16), vrows.view(np.uint16))
    pred = recipe.gaussian("rt_pair_pred", (B, C_, T), 2)
    query = recipe.gaussian("rt_pair_query", (B, C_, T), 3) * st["lr_std"][None, :, None] + st["lr_mean"][None, :, None]
    ref = R.reference(R.queries(R.normalise(query, st["lr_mean"], st["lr_std"])), krows)
    assert (ref["gap"] > 2 * ref["tol"]).all()
    idx, _ = b.search(cuda(query), ts["lr_mean"], ts["lr_std"])
    assert np.array_equal(idx.cpu().numpy().reshape(-1), ref["argmin"])
    y = b.retrieve(cuda(pred), 0.4, stats=ts, query=cuda(query))
    y64, bound = R.blend(pred, vrows, ref["argmin"].reshape(B, T), 0.4, st["hr_mean"], st["hr_std"])
    assert (np.abs(y.cpu().numpy() - y64) <= bound).all()
    with pytest.raises(ValueError):
        b.retrieve(cuda(pred), 0.4, stats=ts)                                  # no LR query
    with pytest.raises(ValueError):
        b.retrieve(cuda(pred), 0.4, stats=dict(ts, lr_std=ts["lr_std"] * 2), query=cuda(query))    # other statistics
    with pytest.raises(ValueError):
        b.add(cuda(hr), ts)                                                    # a paired bank needs both arrays


# ---- end to end on the micro model --------------------------------------------------------------------------------------
def micro_model():
    cfg = recipe.CONFIGS["micro"]
    m = jatsr_amd.JaT_AudioSR_V3(**cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in recipe.make_state_dict(cfg).items()}, strict=False)
    return m.cuda().eval()


@pytest.mark.parametrize("key", ["hr", "lr"])
def test_sample_long_with_a_bank(key):
    m = micro_model()
    Cc, total, chunk, ov = 32, 70, 40, 8
    plan = jatsr_amd.chunk_plan(total, chunk, ov)
    assert [e - s for s, e in plan] == [40, 38]                                # two chunks, the second padded into the first's bucket
    st = tstats(Cc, 21)
    lr = cuda(recipe.gaussian("rt_e2e_lr", (Cc, total), 1) * 1.3 + 0.2)
    noise = [cuda(recipe.gaussian("rt_e2e_noise", (1, Cc, e - s), i)) for i, (s, e) in enumerate(plan)]
    args = (m, lr, st["hr_mean"], st["hr_std"], st["lr_mean"], st["lr_std"])
    kw = dict(num_steps=3, cfg_scale=2.0, chunk_frames=chunk, overlap_frames=ov, noise=noise)
    bank = LatentBank(Cc, 300, key=key)
    hr_train = cuda(recipe.gaussian("rt_e2e_bank_hr", (Cc, 300), 2))
    lr_train = cuda(recipe.gaussian("rt_e2e_bank_lr", (Cc, 300), 3))
    bank.add(hr_train, st, lr_latent=lr_train if key == "lr" else None)
    plain = jatsr_amd.sample_long(*args, **kw)
    assert torch.equal(bits(jatsr_amd.sample_long(*args, bank=None, index_rate=0.4, **kw)), bits(plain))
    assert torch.equal(bits(jatsr_amd.sample_long(*args, bank=bank, index_rate=0.0, **kw)), bits(plain))
    got = jatsr_amd.sample_long(*args, bank=bank, index_rate=0.4, **kw)
    want = bank.retrieve(plain, 0.4, stats=st, query=lr[None] if key == "lr" else None)
    assert got.shape == plain.shape == (1, Cc, total)
    assert torch.equal(bits(got), bits(want)) and not torch.equal(bits(got), bits(plain))
    with pytest.raises(ValueError):
        jatsr_amd.sample_long(*args, bank=bank, index_rate=1.5, **kw)
    with pytest.raises(ValueError):                                             # a bank built with other statistics
        jatsr_amd.sample_long(m, lr, st["hr_mean"] + 1, st["hr_std"], st["lr_mean"], st["lr_std"], bank=bank, index_rate=0.4, **kw)


def test_infer_with_an_index_bank(tmp_path):
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
            str(tmp_path / "stats.json"), "--steps", "2", "--cfg-scale", "2.0", "--seed", "3"]
    infer_main(base + ["--output-dir", str(tmp_path / "plain")])
    infer_main(base + ["--output-dir", str(tmp_path / "idx"), "--index-bank", str(tmp_path / "bank.pt"), "--index-rate", "0.5"])
    assert sorted(os.listdir(tmp_path / "plain")) == ["clip_generated_cfg2.0.pt"]
    assert sorted(os.listdir(tmp_path / "idx")) == ["clip_generated_cfg2.0.pt", "clip_generated_cfg2.0_idx.pt"]
    a = torch.load(tmp_path / "plain" / "clip_generated_cfg2.0.pt", weights_only=False)
    b = torch.load(tmp_path / "idx" / "clip_generated_cfg2.0.pt", weights_only=False)
    for k in ("generated_latent", "hr_latent", "lr_latent"):
        assert torch.equal(a[k], b[k])
    e = torch.load(tmp_path / "idx" / "clip_generated_cfg2.0_idx.pt", weights_only=False)
    assert e["generated_latent"].shape == a["generated_latent"].shape and e["generated_latent"].dtype == torch.float16
    assert not torch.equal(e["generated_latent"], a["generated_latent"])
    assert e["metadata"]["index_rate"] == 0.5 and e["metadata"]["bank_rows"] == 120
    # the loaded bank is the saved one, bit for bit; other statistics at inference are refused
    again = LatentBank.load(tmp_path / "bank.pt")
    assert torch.equal(bits(again.rows()[0]), bits(bank.rows()[0])) and torch.equal(bits(again.rows()[1]), bits(bank.rows()[1]))
    (tmp_path / "other.json").write_text(json.dumps({k: [float(v) + (k == "hr_mean") for v in a_] for k, a_ in st.items()}))
    with pytest.raises(ValueError):
        infer_main(base[:4] + ["--stats-file", str(tmp_path / "other.json")] + base[6:] +
                   ["--output-dir", str(tmp_path / "bad"), "--index-bank", str(tmp_path / "bank.pt")])


@pytest.mark.parametrize("key", ["hr", "lr"])
def test_from_data_dir_holds_the_planned_frames(tmp_path, key):
    Cc, lengths, max_frames = 32, [50, 1, 37], 30
    os.makedirs(tmp_path / "train")
    files = []
    for i, n in enumerate(lengths):
        hr = recipe.gaussian("rt_dir_hr", (Cc, n), i).astype(np.float16)
        lr = recipe.gaussian("rt_dir_lr", (Cc, n), i).astype(np.float16)
        jio.save_latent_file(tmp_path / "train" / f"f{i:02d}.pt", hr_latent=torch.from_numpy(hr), lr_latent=torch.from_numpy(lr))
        files.append((hr, lr))
    st = R.stats(Cc, 41)
    bank = LatentBank.from_data_dir(tmp_path, tstats(Cc, 41), max_frames=max_frames, key=key)
    plan = frame_plan(lengths, max_frames)
    assert plan == [(0, 3, 17), (1, 3, 0), (0, 3, 13)] and len(bank) == 30 == bank.capacity
    kcat, vcat = [], []
    for (hr, lr), (first, stride, count) in zip(files, plan):
        vcat.append(R.pack_rows(hr, st["hr_mean"], st["hr_std"], first, stride, count))
        kcat.append(R.pack_rows(lr, st["lr_mean"], st["lr_std"], first, stride, count) if key == "lr" else vcat[-1])
    assert np.array_equal(bank.rows("keys")[0].cpu().numpy().view(np.uint16), np.concatenate(kcat).view(np.uint16))
    assert np.array_equal(bank.rows("values")[0].cpu().numpy().view(np.uint16), np.concatenate(vcat).view(np.uint16))


# ---- argument errors ----------------------------------------------------------------------------------------------------
def test_argument_errors():
    with pytest.raises(ValueError):
        LatentBank(48, 10)
    C_, N = 32, 20
    b = bank_of(recipe.gaussian("rt_err_keys", (N, C_), 0).astype(np.float16))
    x = cuda(recipe.gaussian("rt_err_q", (1, C_, 8), 1))
    idx = torch.full((8,), -7, dtype=torch.int32, device="cuda")
    need = b.workspace_bytes(8)
    work = torch.zeros(need, dtype=torch.uint8, device="cuda")
    lib, h, s = L.lib(), b._h, L.stream_ptr()
    INV = L.JAT_E_INVALID
    assert lib.jat_bank_search(h, None, None, None, 1, 8, L.ptr(idx), None, L.ptr(work), need, s) == INV          # null x
    assert lib.jat_bank_search(h, L.ptr(x), None, None, 1, 8, None, None, L.ptr(work), need, s) == INV            # null idx
    assert lib.jat_bank_search(h, L.ptr(x), None, None, 1, 8, L.ptr(idx), None, None, need, s) == INV             # null workspace
    assert lib.jat_bank_search(h, L.ptr(x), L.ptr(x), None, 1, 8, L.ptr(idx), None, L.ptr(work), need, s) == INV  # mean without std
    assert lib.jat_bank_search(h, L.ptr(x), None, None, 1, 0, L.ptr(idx), None, L.ptr(work), need, s) == INV      # T = 0
    assert lib.jat_bank_search(h, L.ptr(x), None, None, 1, -3, L.ptr(idx), None, L.ptr(work), need, s) == INV
    assert lib.jat_bank_search(h, L.ptr(x), None, None, 0, 8, L.ptr(idx), None, L.ptr(work), need, s) == INV
    assert lib.jat_bank_search(h, L.ptr(x), None, None, 1, 8, L.ptr(idx), None, L.ptr(work), need - 1, s) == INV  # workspace too small
    assert lib.jat_bank_blend(h, None, L.ptr(idx), None, None, 0.5, L.ptr(x), 1, 8, s) == INV
    assert lib.jat_bank_blend(h, L.ptr(x), L.ptr(idx), None, None, 1.5, L.ptr(x), 1, 8, s) == INV
    assert lib.jat_bank_blend(h, L.ptr(x), L.ptr(idx), None, None, 0.5, L.ptr(x), 1, 0, s) == INV
    n = C.c_size_t()
    assert lib.jat_bank_search_workspace_bytes(h, 0, C.byref(n)) == INV
    torch.cuda.synchronize()
    assert (idx == -7).all()                                                   # nothing was launched
    with pytest.raises(ValueError):
        b.search(x[:, :16].contiguous())                                       # another channel count
    with pytest.raises(ValueError):
        b.blend(x, idx.view(1, 8), -0.1)
    empty = LatentBank(C_, 4)
    assert lib.jat_bank_search(empty._h, L.ptr(x), None, None, 1, 8, L.ptr(idx), None, L.ptr(work), need, s) == L.JAT_E_STATE


# ---- the fp16-operand library ---------------------------------------------------------------------------------------------
def small_run():
    """pack, search with the normalisation in the loader, de-normalising blend: every kernel once at C = 96"""
    C_, n, B, T = 96, 300, 2, 41
    st = tstats(C_, 51)
    b = LatentBank(C_, n)
    b.add(cuda(recipe.gaussian("rt_lib_bank", (C_, n), 0)), st)
    x = cuda(recipe.gaussian("rt_lib_x", (B, C_, T), 1))
    idx, dist2 = b.search(x, st["hr_mean"], st["hr_std"])
    y = b.blend(x, idx, 0.4, st["hr_mean"], st["hr_std"])
    rows, norms = b.rows()
    return {"rows": rows.cpu().numpy(), "norms": norms.cpu().numpy(), "idx": idx.cpu().numpy(), "dist2": dist2.cpu().numpy(),
            "y": y.cpu().numpy()}


def test_fp16_library_gives_the_same_bits(tmp_path):
    """retrieval.hip uses fp16 MFMA in both builds: libjat_hip_fp16.so (a child process) computes what this process computes"""
    code = ("import sys, numpy as np\n"
            "sys.path.insert(0, 'tests')\n"
            "import jatsr_amd._lib as L\n"
            "from test_gpu_retrieval import small_run\n"
            "assert L.operand_dtype() == 'fp16'\n"
            "np.savez(sys.argv[1], **small_run())\n")
    env = dict(os.environ, JAT_OPERAND_DTYPE="fp16")
    env.pop("JAT_LIB_PATH", None)
    path = str(tmp_path / "fp16.npz")
    out = subprocess.run([sys.executable, "-c", code, path], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
    other, here = dict(np.load(path)), small_run()
    assert sorted(other) == sorted(here)
    for k, v in here.items():
        assert v.tobytes() == other[k].tobytes(), k
