"""The IVF index on the GPU (jat_bank_group, jat_ivf_search, IVFBank, load_bank with format 3, sample_long(bank=IVFBank),
infer --index-nprobe) against the twins of tests/retrieval_ivf_ref.py and against the exact search itself.

The grouping is integer work: offsets, order and every copied row are compared bit for bit with the stable sort of the twin.
The search's contract is bit equality with `LatentBank.search_topk` restricted to the probed lists: the probed lists are taken
from the `probes` output, exactly their rows are loaded (positions ascending) into a temporary bank, the exact search runs there
and its indices are mapped back; idx and the bits of dist2 must be equal.  Against fp64 the rule is that of
tests/test_retrieval_topk_gpu.py (tol = 4 max|d32 - d64|, a rank is held to fp64 wherever its gaps to both neighbours exceed
tol); tests/test_retrieval_ivf_cpu.py shows from fp64 alone that at most FP64_LOOSE ranks of a case are excused."""
import ctypes as C
import functools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import retrieval_ivf_ref as IVF  # noqa: E402
import retrieval_ref as R  # noqa: E402
import jatsr_amd  # noqa: E402
import jatsr_amd.io as jio  # noqa: E402
import jatsr_amd.recipe as recipe  # noqa: E402
from jatsr_amd import _lib as L  # noqa: E402
from jatsr_amd import retrieval as RT  # noqa: E402
from jatsr_amd.retrieval import IVFBank, LatentBank  # noqa: E402
from stream_check import Case, check_case  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV, STATE = L.JAT_E_INVALID, L.JAT_E_STATE


def cuda(a):
    return torch.from_numpy(np.array(a)).cuda()


def tstats(C_, salt=0):
    return {k: cuda(v) for k, v in R.stats(C_, salt).items()}


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(t, a):
    got = t.detach().cpu().numpy()
    return got.shape == a.shape and got.dtype == a.dtype and got.tobytes() == np.ascontiguousarray(a).tobytes()


def bank_of(keys16, values16=None, capacity=None, stats=None):
    b = LatentBank(keys16.shape[1], capacity or keys16.shape[0], key="hr" if values16 is None else "lr")
    if stats is not None:
        b._set_stats(stats)
    b.load_rows(cuda(keys16), None if values16 is None else cuda(values16))
    return b


# ---- the layout fixture: lists of chosen sizes, rows interleaved -------------------------------------------------------------
# an empty list, one row, one row short of a tile, a tile, a tile and a row, more than the 128 rows the four waves take at once
SIZES = (0, 1, 31, 32, 33, 300, 64, 129)


@functools.lru_cache(maxsize=None)
def layout(C_, sizes=SIZES, salt=0):
    """-> rows fp16 [N, C] and values fp16 [N, C] in their original order, idx int32 [N], centres fp16 [nlist, C]: row n lies
    around the centre of its list, the lists interleaved"""
    nlist, N = len(sizes), sum(sizes)
    labels = np.repeat(np.arange(nlist), sizes)
    step = next(s for s in (257, 263, 269, 271) if np.gcd(s, N) == 1)
    idx = labels[(np.arange(N) * step) % N].astype(np.int32)
    centres = recipe.gaussian("ivf_layout_centres", (nlist, C_), salt).astype(np.float16)
    rows = (centres[idx].astype(np.float32) + 0.5 * recipe.gaussian("ivf_layout_rows", (N, C_), salt)).astype(np.float16)
    values = recipe.gaussian("ivf_layout_values", (N, C_), salt).astype(np.float16)
    return rows, values, idx, centres


def layout_queries(C_, B, T, centres, salt=0, mean=None, std=None):
    """x fp32 [B, C, T]: query n lies around centre n mod nlist (so every list, the empty one too, is some query's nearest);
    with statistics it does so once it is normalised with them"""
    n = B * T
    q = centres[np.arange(n) % len(centres)].astype(np.float32) + 0.6 * recipe.gaussian("ivf_layout_q", (n, C_), salt)
    if mean is not None:
        q = q * np.asarray(std, np.float32)[None] + np.asarray(mean, np.float32)[None]
    return cuda(np.ascontiguousarray(q.reshape(B, T, C_).transpose(0, 2, 1)).astype(np.float32))


def make_ivf(C_, sizes=SIZES, paired=False, nprobe=1, stats=None, salt=0):
    rows, values, idx, centres = layout(C_, sizes, salt)
    bank = bank_of(rows, values if paired else None, stats=stats)
    grouped, offsets, order = RT.group_rows(bank, cuda(idx), len(sizes))
    return IVFBank(grouped, bank_of(centres, centres if paired else None), offsets, order, nprobe)


def restricted(ivf, x, k, mean, std, probes):
    """`LatentBank.search_topk` over exactly the rows of the probed lists of every query, mapped back to positions.  Queries
    that probe the same lists share one temporary bank."""
    B, C_, T = x.shape
    offsets = ivf.offsets.cpu().numpy()
    keys = ivf.bank.rows("keys")[0]
    q = x.permute(0, 2, 1).reshape(B * T, C_)
    pr = probes.cpu().numpy().reshape(B * T, -1)
    idx = np.full((B * T, k), -1, np.int32)
    dist2 = np.full((B * T, k), np.inf, np.float32)
    groups = {}
    for n in range(B * T):
        groups.setdefault(tuple(pr[n]), []).append(n)
    for lists, ns in groups.items():
        pos = IVF.candidates(offsets, lists)
        if len(pos) == 0:
            continue
        tmp = LatentBank(C_, len(pos))
        tmp.load_rows(keys[torch.from_numpy(pos).cuda()])
        i, d = tmp.search_topk(q[ns].t()[None].contiguous(), k, mean, std)
        i = i[0].cpu().numpy()
        idx[ns] = np.where(i >= 0, pos[np.clip(i, 0, None)], -1)
        dist2[ns] = d[0].cpu().numpy()
    return idx.reshape(B, T, k), dist2.reshape(B, T, k)


# ---- 1. the grouping ------------------------------------------------------------------------------------------------------------
GROUP_SIZES = (0, 1, 31, 32, 33, 1500, 2)       # one list holds most of the bank


@pytest.mark.parametrize("paired", [False, True], ids=["keys", "paired"])
@pytest.mark.parametrize("C_", [32, 96, 1024])
def test_grouping_equals_the_twin(C_, paired):
    rows, values, idx, _ = layout(C_, GROUP_SIZES, 1)
    nlist, N = len(GROUP_SIZES), len(rows)
    bank = bank_of(rows, values if paired else None)
    norms = bank.rows("keys")[1].cpu().numpy()
    offsets, order = IVF.group(idx, nlist)
    assert np.diff(offsets).tolist() == list(GROUP_SIZES)
    runs = [RT.group_rows(bank, cuda(idx), nlist) for _ in range(2)]
    for g, o, r in runs:
        assert len(g) == N and same_bits(o, offsets) and same_bits(r, order)
        assert same_bits(g.rows("keys")[0], rows[order]) and same_bits(g.rows("keys")[1], norms[order])
        if paired:
            assert same_bits(g.rows("values")[0], values[order])
    assert same_bits(bank.rows("keys")[0], rows)                         # the source is left as it was


def test_grouping_with_indices_outside_the_lists():
    rows, _, idx, _ = layout(96, GROUP_SIZES, 1)
    nlist, N = len(GROUP_SIZES), len(rows)
    bad = idx.copy()
    bad[[3, 700, N - 1]] = [-1, nlist, 2 ** 31 - 1]
    bad[10] = -2 ** 31
    offsets, order = IVF.group(bad, nlist)
    assert offsets[-1] == N - 4 and order[-4:].tolist() == [3, 10, 700, N - 1]
    bank = bank_of(rows)
    g, o, r = RT.group_rows(bank, cuda(bad), nlist, check=False)
    assert same_bits(o, offsets) and same_bits(r, order) and same_bits(g.rows("keys")[0], rows[order])
    with pytest.raises(ValueError, match="4 entries of idx lie outside"):
        RT.group_rows(bank, cuda(bad), nlist)
    # such rows belong to no list: a search over every list never returns them
    ivf = IVFBank(g, bank_of(layout(96, GROUP_SIZES, 1)[3]), o, r, 8)
    i, _ = ivf.search_topk(layout_queries(96, 1, 33, layout(96, GROUP_SIZES, 1)[3]), 8)
    assert int(i.max()) < N - 4 and int(i.min()) >= 0


# ---- 2. the search equals the exact search restricted to the probed lists ------------------------------------------------------------
# (channels, k, nprobe, B, T, statistics given)
SEARCH_CASES = [(32, 1, 1, 1, 1, False), (96, 3, 2, 1, 33, True), (1024, 8, 8, 2, 35, False), (1024, 1, 2, 1, 70, True),
                (96, 8, 1, 1, 70, False), (32, 3, 8, 1, 33, True), (1024, 3, 1, 1, 33, False), (96, 1, 8, 1, 70, False),
                (32, 8, 2, 3, 11, False)]


@pytest.mark.parametrize("C_,k,nprobe,B,T,norm", SEARCH_CASES)
def test_search_equals_the_restricted_exact_search(C_, k, nprobe, B, T, norm):
    ivf = make_ivf(C_)
    ts = tstats(C_, 3)
    mean, std = (ts["hr_mean"], ts["hr_std"]) if norm else (None, None)
    centres = layout(C_)[3]
    x = layout_queries(C_, B, T, centres, **(dict(mean=R.stats(C_, 3)["hr_mean"], std=R.stats(C_, 3)["hr_std"]) if norm else {}))
    idx, dist2, pr = ivf.search_topk(x, k, mean, std, nprobe=nprobe, probes=True)
    assert idx.shape == dist2.shape == (B, T, k) and pr.shape == (B, T, nprobe)
    ci, _ = ivf.centroids.search_topk(x, nprobe, mean, std)
    assert torch.equal(pr, ci)                                           # stage 1 is the exact search over the centroids
    want_i, want_d = restricted(ivf, x, k, mean, std, pr)
    assert same_bits(idx, want_i)
    assert same_bits(bits(dist2), want_d.view(np.int32))
    sizes = np.diff(ivf.offsets.cpu().numpy())
    first = pr.cpu().numpy().reshape(B * T, nprobe)[:, 0]
    print(f"first probes cover lists of {sorted(set(sizes[first].tolist()))} rows; {int((idx < 0).sum())} places without a candidate")
    if B * T >= 33:
        assert set(sizes[first].tolist()) == set(SIZES)                  # every list size was somebody's nearest list


def test_fewer_lists_than_probes_and_fewer_candidates_than_k():
    sizes = (1, 0, 2)
    ivf = make_ivf(96, sizes)
    x = layout_queries(96, 1, 33, layout(96, sizes)[3])
    idx, dist2, pr = ivf.search_topk(x, 8, nprobe=8, probes=True)
    assert (pr[..., 3:] == -1).all() and (pr[..., :3] >= 0).all()
    assert (idx[..., 3:] == -1).all() and torch.isinf(dist2[..., 3:]).all() and (idx[..., :3] >= 0).all()
    flat = ivf.bank.search_topk(x, 8)
    assert torch.equal(idx, flat[0]) and torch.equal(bits(dist2), bits(flat[1]))
    idx, dist2, pr = ivf.search_topk(x, 3, nprobe=1, probes=True)
    want_i, want_d = restricted(ivf, x, 3, None, None, pr)
    assert same_bits(idx, want_i) and same_bits(bits(dist2), want_d.view(np.int32))
    empty = (pr[0, :, 0] == 1).cpu().numpy()                             # the queries whose nearest list is the empty one
    assert empty.any() and (idx[0, empty] == -1).all() and torch.isinf(dist2[0, empty]).all()


# ---- 3. every list probed: the exact search on the grouped bank -------------------------------------------------------------------
@pytest.mark.parametrize("nlist", [1, 4, 8])
def test_all_lists_probed_is_the_exact_search(nlist):
    sizes = {1: (333,), 4: (0, 33, 200, 31), 8: SIZES}[nlist]
    for C_, k in ((96, 8), (1024, 3)):
        ivf = make_ivf(C_, sizes, paired=(C_ == 96))
        ts = tstats(C_, 4)
        x = layout_queries(C_, 2, 35, layout(C_, sizes)[3])
        got = ivf.search_topk(x, k, ts["hr_mean"], ts["hr_std"], nprobe=8)
        want = ivf.bank.search_topk(x, k, ts["hr_mean"], ts["hr_std"])
        assert torch.equal(got[0], want[0]) and torch.equal(bits(got[1]), bits(want[1]))


# ---- 4. against fp64 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(IVF.FP64_CASES))
def test_against_fp64(name):
    c = IVF.fp64_case(name)
    nprobe, k = c["nprobe"], c["k"]
    ivf = IVFBank.from_centroids(bank_of(c["rows"]), bank_of(c["cent"]), nprobe)
    assert same_bits(ivf.offsets, c["offsets"]) and same_bits(ivf.order, c["order"])      # margins: test_fixture_margins
    idx, dist2, pr = ivf.search_topk(cuda(c["x"]), k, probes=True)
    idx, dist2 = idx.reshape(-1, k).cpu().numpy(), dist2.reshape(-1, k).cpu().numpy().astype(np.float64)
    pr = pr.reshape(-1, nprobe).cpu().numpy()
    lists_loose = np.zeros(pr.shape, bool)                               # ranks behind the last list are -1 on both sides
    lists_loose[:, :c["probes_loose"].shape[1]] = c["probes_loose"]
    assert not ((pr != c["probes"]) & ~lists_loose).any()
    loose = IVF.undecided(c["d64"], c["offsets"], pr, k, c["tol"])
    want_i, want_d = IVF.search(c["d64"], c["offsets"], pr, k)
    n_loose = int(loose.sum()) + int(c["probes_loose"].sum())
    print(f"{name}: {n_loose} ranks inside the near-tie allowance, {int((idx != want_i).sum())} differ from fp64")
    assert n_loose <= IVF.FP64_LOOSE
    assert not ((idx != want_i) & ~loose).any()
    live = idx >= 0
    assert (live == (want_i >= 0)).all() and np.isinf(dist2[~live]).all()
    rows = np.arange(len(idx))[:, None].repeat(k, 1)
    err = np.abs(dist2[live] - np.maximum(c["d64"][rows[live], idx[live]], 0))
    print(f"{name}: worst dist2 error {err.max():.3g}, tol {c['tol']:.3g}")
    assert (err <= c["tol"]).all()


# ---- 5. ties ------------------------------------------------------------------------------------------------------------------------
def test_tie_rules():
    C_ = 96
    rows, _, idx, centres = (a.copy() for a in layout(C_, (40, 50, 60, 45), 2))
    a = (rows[7].astype(np.float32) * 0.5 + 0.25).astype(np.float16)      # a row the bank does not hold yet
    in0, in2 = np.flatnonzero(idx == 0), np.flatnonzero(idx == 2)
    rows[in0[[3, 20, 38]]] = a                                            # three copies inside list 0 ...
    rows[in2[[0, 33, 59]]] = a                                            # ... and three more in list 2: tiles 0 and 1 of that list
    bank = bank_of(rows)
    grouped, offsets, order = RT.group_rows(bank, cuda(idx), 4)
    x = cuda(np.ascontiguousarray(a.astype(np.float32)[None, :, None]))
    off = offsets.cpu().numpy()
    want0 = [int(off[0]) + v for v in (3, 20, 38)]
    want2 = [int(off[2]) + v for v in (0, 33, 59)]
    # inside one list: only list 0 is probed (its centroid is made the query's nearest), the lower position first
    cent = centres.copy()
    cent[0] = a
    ivf = IVFBank(grouped, bank_of(cent), offsets, order, 1)
    i, d, pr = ivf.search_topk(x, 4, probes=True)
    assert pr.flatten().tolist() == [0] and i.flatten().tolist()[:3] == want0
    assert len(set(bits(d).flatten().tolist()[:3])) == 1 and float(d.flatten()[3]) > float(d.flatten()[0])
    # across two probed lists
    i, d = ivf.search_topk(x, 8, nprobe=8)
    assert i.flatten().tolist()[:6] == want0 + want2 and len(set(bits(d).flatten().tolist()[:6])) == 1
    flat = ivf.bank.search_topk(x, 8)
    assert torch.equal(i, flat[0]) and torch.equal(bits(d), bits(flat[1]))
    # duplicated centroids: the lower list is the probed one
    cent[2] = a
    ivf = IVFBank(grouped, bank_of(cent), offsets, order, 1)
    i, d, pr = ivf.search_topk(x, 4, probes=True)
    assert pr.flatten().tolist() == [0] and i.flatten().tolist()[:3] == want0
    _, _, pr = ivf.search_topk(x, 2, nprobe=2, probes=True)
    assert pr.flatten().tolist() == [0, 2]


# ---- 6. the planted fixture -----------------------------------------------------------------------------------------------------------
def test_planted_fixture():
    p = IVF.planted()
    C_, K, N = IVF.PLANTED
    x = cuda(p["x"])
    bank = bank_of(p["rows"])
    ivf = IVFBank.from_centroids(bank, bank_of(p["centres"]), 1)
    offsets, order = IVF.group(p["member"], K)
    assert same_bits(ivf.offsets, offsets) and same_bits(ivf.order, order)
    idx, _ = ivf.search(x)
    assert (ivf.order.cpu().numpy()[idx.cpu().numpy()[0]] == p["own"]).all()
    built, report = IVFBank.build(bank, nlist=K, iters=10)
    assert report["lists"] == report["kept"] == K and report["list_min"] >= N // K and report["list_max"] <= N // K + 1
    assert report["nprobe"] == built.nprobe == 1 and len(built) == N
    got = built.order.cpu().numpy()
    assert sorted(got.tolist()) == list(range(N))
    for l in range(K):                                                    # a list is one planted cluster
        assert len(set(p["member"][got[int(built.offsets[l]):int(built.offsets[l + 1])]].tolist())) == 1
    idx, _ = built.search(x)
    assert (got[idx.cpu().numpy()[0]] == p["own"]).all()
    assert RT.default_nlist(N) == 2 and IVFBank.build(bank)[1]["clusters"] == 2


# ---- 7. independence ---------------------------------------------------------------------------------------------------------------
def test_independence_of_batch_k_and_run():
    ivf = make_ivf(1024, nprobe=2)
    x = layout_queries(1024, 2, 35, layout(1024)[3])
    i8, d8 = ivf.search_topk(x, 8)
    again = ivf.search_topk(x, 8)
    assert torch.equal(i8, again[0]) and torch.equal(bits(d8), bits(again[1]))
    i3, d3 = ivf.search_topk(x, 3)
    assert torch.equal(i3, i8[..., :3]) and torch.equal(bits(d3), bits(d8[..., :3]))
    i1, d1 = ivf.search(x)
    assert torch.equal(i1, i8[..., 0]) and torch.equal(bits(d1), bits(d8[..., 0]))
    for b, t in ((0, 0), (1, 17), (1, 34)):
        one = ivf.search_topk(x[b:b + 1, :, t:t + 1].contiguous(), 8)
        assert torch.equal(one[0][0, 0], i8[b, t]) and torch.equal(bits(one[1][0, 0]), bits(d8[b, t]))
    flip = ivf.search_topk(x.flip(2).contiguous(), 8)                    # other neighbours, another place in the grid
    assert torch.equal(flip[0].flip(1), i8) and torch.equal(bits(flip[1].flip(1)), bits(d8))


# ---- 8. streams and graphs ---------------------------------------------------------------------------------------------------------
def group_work(bank, nlist):
    n = C.c_size_t()
    assert L.lib().jat_bank_group_workspace_bytes(bank._h, nlist, C.byref(n)) == 0
    return torch.empty(n.value, dtype=torch.uint8, device="cuda")


def search_work(bank, cent, nq, k, nprobe):
    n = C.c_size_t()
    assert L.lib().jat_ivf_search_workspace_bytes(bank._h, cent._h, nq, k, nprobe, C.byref(n)) == 0
    return torch.empty(n.value, dtype=torch.uint8, device="cuda")


def raw_group(src, idx, nlist, dst, offsets, order, work):
    return L.lib().jat_bank_group(src._h, L.ptr(idx), nlist, dst._h, L.ptr(offsets), L.ptr(order), L.ptr(work),
                                  0 if work is None else work.numel(), L.stream_ptr())


def raw_search(bank, cent, offsets, x, mean, std, k, nprobe, idx, dist2, probes, work):
    B, _, T = x.shape
    return L.lib().jat_ivf_search(bank._h, cent._h, L.ptr(offsets), L.ptr(x), L.ptr(mean), L.ptr(std), B, T, k, nprobe,
                                  L.ptr(idx), L.ptr(dist2), L.ptr(probes), L.ptr(work), 0 if work is None else work.numel(),
                                  L.stream_ptr())


STREAM_C, STREAM_SIZES = 96, (40, 0, 33, 130, 1)


def stream_cases():
    Cc, sizes = STREAM_C, STREAM_SIZES
    nlist, N = len(sizes), sum(sizes)
    rows, _, idx, centres = layout(Cc, sizes, 5)
    other = np.roll(idx, 7)                                               # a decoy assignment: in range, other lists

    def group():
        def fresh(live, outs):
            return LatentBank(Cc, N), LatentBank(Cc, N)                   # created before the delay starts; filled on the stream

        def call(st, i, o):
            src, dst = st
            src.load_rows(i["rows"])
            assert raw_group(src, i["idx"], nlist, dst, o["offsets"], o["order"], group_work(src, nlist)) == 0
            return {"keys": dst.rows("keys")[0].clone(), "norms": dst.rows("keys")[1].clone()}
        return Case({"rows": cuda(rows), "idx": cuda(idx)}, call,
                    outputs={"offsets": torch.empty(nlist + 1, dtype=torch.int32, device="cuda"),
                             "order": torch.empty(N, dtype=torch.int32, device="cuda")}, decoys={"idx": cuda(other)}, state=fresh)

    def search():
        B, T, k, nprobe = 2, 17, 3, 2
        offsets, order = IVF.group(idx, nlist)
        decoy_offsets = np.minimum(offsets + np.arange(nlist + 1), N).astype(np.int32)
        ts = tstats(Cc, 6)

        def fresh(live, outs):
            return LatentBank(Cc, N), LatentBank(Cc, nlist)

        def call(st, i, o):
            bank, cent = st
            bank.load_rows(i["rows"])
            cent.load_rows(i["cent"])
            work = search_work(bank, cent, B * T, k, nprobe)
            assert raw_search(bank, cent, i["offsets"], i["x"], i["mean"], i["std"], k, nprobe, o["idx"], o["dist2"], o["probes"],
                              work) == 0
            ivf = IVFBank(bank, cent, i["offsets"], torch.zeros(N, dtype=torch.int32, device="cuda"), nprobe)
            wi, wd = ivf.search_topk(i["x"], k, i["mean"], i["std"])
            return {"w_idx": wi, "w_dist2": wd}
        return Case({"rows": cuda(rows[order]), "cent": cuda(centres), "offsets": cuda(offsets),
                     "x": layout_queries(Cc, B, T, centres, 5), "mean": ts["hr_mean"], "std": ts["hr_std"]}, call,
                    outputs={"idx": torch.empty(B, T, k, dtype=torch.int32, device="cuda"), "dist2": torch.empty(B, T, k, device="cuda"),
                             "probes": torch.empty(B, T, nprobe, dtype=torch.int32, device="cuda")},
                    decoys={"offsets": cuda(decoy_offsets)}, state=fresh)

    return {"jat_bank_group": group, "jat_ivf_search": search}


def test_every_stream_taking_entry_has_a_case():
    header = open(os.path.join(ROOT, "include", "jat_hip_ivf.h")).read()
    takes = set(re.findall(r"\bint (jat_[a-z0-9_]+)\([^;]*void\* stream\)", header))
    assert takes == set(stream_cases()) and len(takes) == 2
    assert takes | {"jat_bank_group_workspace_bytes", "jat_ivf_search_workspace_bytes"} == set(L.IVF_SIGNATURES)


@pytest.mark.parametrize("name", ["jat_bank_group", "jat_ivf_search"])
def test_side_stream(name):
    check_case(stream_cases()[name](), name, synchronises=False)


def test_graph_capture():
    """grouping and search captured into one graph and replayed after the assignment and the queries changed: no allocation,
    synchronisation or copy in either entry"""
    Cc, sizes = STREAM_C, STREAM_SIZES
    nlist, N = len(sizes), sum(sizes)
    rows, _, idx0, centres = layout(Cc, sizes, 5)
    idx1 = np.roll(idx0, 11)
    B, T, k, nprobe = 2, 17, 8, 2
    x0, x1 = layout_queries(Cc, B, T, centres, 5), layout_queries(Cc, B, T, centres, 6)
    src, cent = bank_of(rows), bank_of(centres)
    idx, x = cuda(idx0), x0.clone()
    offsets, order = torch.zeros(nlist + 1, dtype=torch.int32, device="cuda"), torch.zeros(N, dtype=torch.int32, device="cuda")
    out_i = torch.zeros(B, T, k, dtype=torch.int32, device="cuda")
    out_d, out_p = torch.zeros(B, T, k, device="cuda"), torch.zeros(B, T, nprobe, dtype=torch.int32, device="cuda")
    gwork, swork = group_work(src, nlist), search_work(src, cent, B * T, k, nprobe)

    def run(dst):
        assert raw_group(src, idx, nlist, dst, offsets, order, gwork) == 0
        assert raw_search(dst, cent, offsets, x, None, None, k, nprobe, out_i, out_d, out_p, swork) == 0
    run(LatentBank(Cc, N))                                                # eagerly once: what the first launch of a kernel sets up
    torch.cuda.synchronize()
    dst = LatentBank(Cc, N)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run(dst)
    idx.copy_(cuda(idx1))
    x.copy_(x1)
    g.replay()
    torch.cuda.synchronize()
    want_g, want_o, want_r = RT.group_rows(src, cuda(idx1), nlist)
    want = IVFBank(want_g, cent, want_o, want_r, nprobe).search_topk(x1, k, probes=True)
    assert torch.equal(offsets, want_o) and torch.equal(order, want_r) and torch.equal(dst.rows("keys")[0], want_g.rows("keys")[0])
    assert torch.equal(out_i, want[0]) and torch.equal(bits(out_d), bits(want[1])) and torch.equal(out_p, want[2])
    assert not torch.equal(want_r, cuda(IVF.group(idx0, nlist)[1]))        # the replay saw other inputs than the capture


# ---- 9. the fp16-operand library ---------------------------------------------------------------------------------------------------
def small_run():
    """grouping (paired) and searches at two widths, with and without statistics"""
    out = {}
    for C_, k, nprobe, norm in ((96, 8, 2, True), (1024, 3, 1, False)):
        ivf = make_ivf(C_, paired=(C_ == 96))
        ts = tstats(C_, 3)
        x = layout_queries(C_, 2, 35, layout(C_)[3])
        i, d, p = ivf.search_topk(x, k, *((ts["hr_mean"], ts["hr_std"]) if norm else (None, None)), nprobe=nprobe, probes=True)
        out.update({f"idx{C_}": i.cpu().numpy(), f"dist2{C_}": d.cpu().numpy(), f"probes{C_}": p.cpu().numpy(),
                    f"order{C_}": ivf.order.cpu().numpy(), f"offsets{C_}": ivf.offsets.cpu().numpy(),
                    f"keys{C_}": ivf.bank.rows("keys")[0].cpu().numpy(), f"norms{C_}": ivf.bank.rows("keys")[1].cpu().numpy()})
    return out


def test_fp16_library_gives_the_same_bits(tmp_path):
    """retrieval_ivf.hip uses fp16 MFMA and integer work in both builds: libjat_hip_fp16.so (a child process) computes what this
    process computes"""
    code = ("import sys, numpy as np\n"
            "sys.path.insert(0, 'tests')\n"
            "import jatsr_amd._lib as L\n"
            "from test_retrieval_ivf_gpu import small_run\n"
            "assert L.operand_dtype() == 'fp16'\n"
            "np.savez(sys.argv[1], **small_run())\n")
    env = dict(os.environ, JAT_OPERAND_DTYPE="fp16")
    env.pop("JAT_LIB_PATH", None)
    path = str(tmp_path / "fp16.npz")
    out = subprocess.run([sys.executable, "-c", code, path], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
    other, here = dict(np.load(path)), small_run()
    assert sorted(other) == sorted(here) and len(here) == 14
    for k, v in here.items():
        assert v.tobytes() == other[k].tobytes(), k


# ---- 10. end to end -----------------------------------------------------------------------------------------------------------------
def write_data_dir(root, Cc, lengths):
    os.makedirs(root / "train")
    for i, n in enumerate(lengths):
        jio.save_latent_file(root / "train" / f"f{i}.pt", hr_latent=torch.from_numpy(recipe.gaussian("ivf_dir_hr", (Cc, n), i)),
                             lr_latent=torch.from_numpy(recipe.gaussian("ivf_dir_lr", (Cc, n), i)))
    st = R.stats(Cc, 31)
    (root / "global_stats_separated.json").write_text(json.dumps({k: [float(v) for v in a] for k, a in st.items()}))


def micro_model():
    cfg = recipe.CONFIGS["micro"]
    m = jatsr_amd.JaT_AudioSR_V3(**cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in recipe.make_state_dict(cfg).items()}, strict=False)
    return m.cuda().eval()


def test_build_load_sample_and_infer(tmp_path):
    from jatsr_amd.infer import main as infer_main
    cfg = recipe.CONFIGS["micro"]
    Cc = cfg["input_channels"]
    lengths = [90, 50, 77]
    write_data_dir(tmp_path / "data", Cc, lengths)
    stats_path = tmp_path / "data" / "global_stats_separated.json"
    base = ["build", "--data-dir", str(tmp_path / "data")]
    RT.main(base + ["--out", str(tmp_path / "ivf.pt"), "--ivf", "--ivf-lists", "6", "--kmeans-iters", "4"])
    RT.main(base + ["--out", str(tmp_path / "ivf_km.pt"), "--ivf", "--clusters", "60", "--ivf-nprobe", "3", "--key", "lr"])
    for bad in (["--ivf", "--scales", "1,2"], ["--ivf-lists", "4"], ["--ivf-nprobe", "2"], ["--ivf", "--ivf-lists", "0"],
                ["--ivf", "--ivf-lists", "1000"]):
        with pytest.raises((SystemExit, ValueError)):
            RT.main(base + ["--out", str(tmp_path / "bad.pt")] + bad)
    assert not os.path.exists(tmp_path / "bad.pt")
    report = json.load(open(str(tmp_path / "ivf.pt") + ".ivf.json"))
    ivf = RT.load_bank(tmp_path / "ivf.pt")
    assert isinstance(ivf, IVFBank) and torch.load(tmp_path / "ivf.pt", weights_only=False)["format"] == 3
    assert len(ivf) == sum(lengths) == report["rows"] and ivf.nlist == report["lists"] <= 6 and ivf.nprobe == 1
    assert int(ivf.offsets[-1]) == len(ivf) and sorted(ivf.order.cpu().tolist()) == list(range(len(ivf)))
    km = RT.load_bank(tmp_path / "ivf_km.pt")
    assert isinstance(km, IVFBank) and km.key == "lr" and km.nprobe == 3 and len(km) <= 60
    assert os.path.exists(str(tmp_path / "ivf_km.pt") + ".kmeans.json")
    # a round trip keeps every part
    ivf.save(tmp_path / "again.pt")
    back = IVFBank.load(tmp_path / "again.pt")
    assert torch.equal(back.rows("keys")[0], ivf.rows("keys")[0]) and torch.equal(back.offsets, ivf.offsets)
    assert torch.equal(back.order, ivf.order) and torch.equal(back.centroids.rows("keys")[0], ivf.centroids.rows("keys")[0])
    # the sampler
    m = micro_model()
    total, chunk, ov = 70, 40, 8
    plan = jatsr_amd.chunk_plan(total, chunk, ov)
    st = jio.load_stats(stats_path, channels=Cc, device="cuda")
    lr = cuda(recipe.gaussian("rt_e2e_lr", (Cc, total), 1) * 1.3 + 0.2)
    noise = [cuda(recipe.gaussian("rt_e2e_noise", (1, Cc, e - s), i)) for i, (s, e) in enumerate(plan)]
    args = (m, lr, st["hr_mean"], st["hr_std"], st["lr_mean"], st["lr_std"])
    kw = dict(num_steps=3, cfg_scale=2.0, chunk_frames=chunk, overlap_frames=ov, noise=noise)
    plain = jatsr_amd.sample_long(*args, **kw)
    for k in (1, 4):
        got = jatsr_amd.sample_long(*args, bank=ivf, index_rate=0.4, index_k=k, **kw)
        assert torch.equal(bits(got), bits(ivf.retrieve(plain, 0.4, stats=st, k=k))) and not torch.equal(bits(got), bits(plain))
    # a format-1 file written from ivf.bank is a plain bank, and blends the same positions
    ivf.bank.save(tmp_path / "flat.pt")
    flat = RT.load_bank(tmp_path / "flat.pt")
    assert isinstance(flat, LatentBank) and not isinstance(flat, IVFBank)
    y, idx, dist2 = ivf.retrieve(plain, 0.4, stats=st, k=4, neighbours=True)
    assert torch.equal(bits(flat.blend_topk(plain, idx, dist2, 0.4, st["hr_mean"], st["hr_std"])), bits(y))
    y1, idx1, _ = ivf.retrieve(plain, 0.4, stats=st, neighbours=True)
    assert torch.equal(bits(flat.blend(plain, idx1, 0.4, st["hr_mean"], st["hr_std"])), bits(y1))
    # infer
    torch.save({"model_state_dict": {k: torch.from_numpy(v) for k, v in recipe.make_state_dict(cfg).items()},
                "config": dict(cfg)}, tmp_path / "last.pt")
    jio.save_latent_file(tmp_path / "clip.pt", hr_latent=torch.from_numpy(recipe.gaussian("rt_inf_hr", (Cc, 200), 1)),
                         lr_latent=torch.from_numpy(recipe.gaussian("rt_inf_lr", (Cc, 200), 2)))
    common = ["--checkpoint", str(tmp_path / "last.pt"), "--input-file", str(tmp_path / "clip.pt"), "--stats-file", str(stats_path),
              "--steps", "2", "--cfg-scale", "2.0", "--seed", "3", "--index-rate", "0.5"]
    infer_main(common + ["--index-bank", str(tmp_path / "ivf.pt"), "--index-nprobe", "2", "--output-dir", str(tmp_path / "o1")])
    f1 = torch.load(tmp_path / "o1" / "clip_generated_cfg2.0_idx.pt", weights_only=False)
    assert f1["metadata"]["index_nprobe"] == 2 and f1["metadata"]["index_lists"] == ivf.nlist and f1["metadata"]["bank_rows"] == len(ivf)
    assert torch.isfinite(f1["generated_latent"]).all()
    with pytest.raises(SystemExit, match="index-nprobe"):
        infer_main(common + ["--index-bank", str(tmp_path / "flat.pt"), "--index-nprobe", "2", "--output-dir", str(tmp_path / "o2")])


# ---- 11. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_in_python():
    ivf = make_ivf(96)
    x = layout_queries(96, 1, 5, layout(96)[3])
    for k in (0, 9):
        with pytest.raises(ValueError, match="index_k"):
            ivf.search_topk(x, k)
    for nprobe in (0, 9, 1.0):
        with pytest.raises(ValueError, match="nprobe"):
            ivf.search_topk(x, 1, nprobe=nprobe)
        with pytest.raises(ValueError, match="nprobe"):
            IVFBank(ivf.bank, ivf.centroids, ivf.offsets, ivf.order, nprobe)
    with pytest.raises(ValueError, match="expected a CUDA fp32"):
        ivf.search_topk(layout_queries(32, 1, 5, layout(32)[3]), 1)
    with pytest.raises(ValueError, match="channels"):
        IVFBank(ivf.bank, bank_of(layout(32)[3]), ivf.offsets, ivf.order)
    with pytest.raises(ValueError, match="offsets"):
        IVFBank(ivf.bank, ivf.centroids, ivf.offsets[:-1], ivf.order)
    rows, _, idx, centres = layout(96)
    bank = bank_of(rows)
    with pytest.raises(ValueError, match="idx"):
        RT.group_rows(bank, cuda(idx[:-1]), len(SIZES))
    with pytest.raises(ValueError, match="idx"):
        RT.group_rows(bank, cuda(idx.astype(np.int64)), len(SIZES))
    for nlist in (0, len(rows) + 1):
        with pytest.raises(ValueError, match="lists for a bank"):
            RT.group_rows(bank, cuda(idx), nlist)
    with pytest.raises(ValueError, match="channels"):
        IVFBank.from_centroids(bank, bank_of(layout(32)[3]))
    with pytest.raises(ValueError, match="clusters"):
        IVFBank.build(bank, nlist=0)
    with pytest.raises(ValueError, match="index_rate"):
        ivf.retrieve(x, 1.5)


def test_refusals_through_the_raw_abi():
    lib = L.lib()
    rows, values, idx, centres = layout(96)
    nlist, N = len(SIZES), len(rows)
    src, cent = bank_of(rows), bank_of(centres)
    didx = cuda(idx)
    offsets, order = torch.zeros(nlist + 1, dtype=torch.int32, device="cuda"), torch.zeros(N, dtype=torch.int32, device="cuda")
    n = C.c_size_t()
    assert lib.jat_bank_group_workspace_bytes(src._h, nlist, C.byref(n)) == 0 and n.value >= 4 * (N + nlist + 1)
    gwork = group_work(src, nlist)
    for bad in (0, N + 1):
        assert lib.jat_bank_group_workspace_bytes(src._h, bad, C.byref(n)) == INV
        assert raw_group(src, didx, bad, LatentBank(96, N), offsets, order, gwork) == INV
    assert lib.jat_bank_group_workspace_bytes(src._h, nlist, None) == INV
    assert lib.jat_bank_group_workspace_bytes(LatentBank(96, 4)._h, 1, C.byref(n)) == STATE
    assert raw_group(src, didx, nlist, LatentBank(96, N), offsets, order, gwork[:-1]) == INV          # a short workspace
    assert raw_group(src, didx, nlist, LatentBank(96, N), offsets, order, None) == INV
    assert raw_group(src, None, nlist, LatentBank(96, N), offsets, order, gwork) == INV
    assert raw_group(src, didx, nlist, LatentBank(96, N), None, order, gwork) == INV
    assert raw_group(src, didx, nlist, LatentBank(96, N - 1), offsets, order, gwork) == INV           # too small a destination
    assert raw_group(src, didx, nlist, LatentBank(64, N), offsets, order, gwork) == INV               # mixed channel counts
    assert raw_group(src, didx, nlist, LatentBank(96, N, key="lr"), offsets, order, gwork) == INV     # mixed pairedness
    assert raw_group(src, didx, nlist, src, offsets, order, gwork) == INV
    assert raw_group(LatentBank(96, N), didx, nlist, LatentBank(96, N), offsets, order, gwork) == STATE   # an empty source
    full = bank_of(rows[:5], capacity=N)
    assert raw_group(src, didx, nlist, full, offsets, order, gwork) == STATE and len(full) == 5       # a destination that is not empty
    assert b"must be empty" in lib.jat_last_error()
    # the search
    g, goff, gorder = RT.group_rows(src, didx, nlist)
    B, T = 1, 5
    x = layout_queries(96, B, T, centres)
    oi, od = torch.full((B, T, 8), 7, dtype=torch.int32, device="cuda"), torch.full((B, T, 8), 7.0, device="cuda")
    work = search_work(g, cent, B * T, 8, 8)

    def call(bank=g, cents=cent, off=goff, xx=x, k=8, nprobe=8, i=oi, w=work, mean=None, std=None):
        return raw_search(bank, cents, off, xx, mean, std, k, nprobe, i, od, None, w)
    assert call() == 0
    torch.cuda.synchronize()
    good = oi.clone()
    for k in (0, 9, -1):
        assert call(k=k) == INV and lib.jat_ivf_search_workspace_bytes(g._h, cent._h, 5, k, 1, C.byref(n)) == INV
    for nprobe in (0, 9, -1):
        assert call(nprobe=nprobe) == INV and lib.jat_ivf_search_workspace_bytes(g._h, cent._h, 5, 1, nprobe, C.byref(n)) == INV
    assert call(cents=bank_of(layout(32)[3])) == INV                                                   # mixed channel counts
    assert lib.jat_ivf_search_workspace_bytes(g._h, bank_of(layout(32)[3])._h, 5, 1, 1, C.byref(n)) == INV
    assert call(cents=g) == INV                                                                        # the same bank twice
    assert call(w=work[:-1]) == INV and call(w=None) == INV and call(off=None) == INV and call(i=None) == INV
    assert call(mean=x) == INV                                                                         # mean without std
    assert call(bank=LatentBank(96, 4)) == STATE and call(cents=LatentBank(96, 4)) == STATE            # an empty bank, no centroids
    assert lib.jat_ivf_search_workspace_bytes(g._h, cent._h, 0, 1, 1, C.byref(n)) == INV
    assert lib.jat_ivf_search_workspace_bytes(g._h, cent._h, 5, 1, 1, None) == INV
    torch.cuda.synchronize()
    assert torch.equal(oi, good)                                                                       # a refused call wrote nothing
    # N > 2^22: a real bank of 2^22 + 1 rows of 32 channels (268 MB of zeros)
    big = LatentBank(32, 2 ** 22 + 1)
    big.load_rows(torch.zeros(2 ** 22 + 1, 32, dtype=torch.float16, device="cuda"))
    bidx = torch.zeros(2 ** 22 + 1, dtype=torch.int32, device="cuda")
    assert lib.jat_bank_group_workspace_bytes(big._h, 1, C.byref(n)) == INV
    assert raw_group(big, bidx, 1, LatentBank(32, 2 ** 22 + 1), bidx, bidx, gwork) == INV
    assert b"2^22" in lib.jat_last_error()
    small = bank_of(layout(32)[3])
    x32 = layout_queries(32, 1, 5, layout(32)[3])
    assert raw_search(big, small, goff, x32, None, None, 1, 1, oi, od, None, work) == INV
    assert b"2^22" in lib.jat_last_error()
    with pytest.raises(ValueError, match="exceeds"):
        IVFBank.from_centroids(big, small)
