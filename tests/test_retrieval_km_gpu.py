"""k-means compaction of a retrieval bank on the GPU (jat_bank_assign, jat_bank_cluster_update, jat_bank_sum_dist2,
LatentBank.assign / cluster_update, retrieval.kmeans, build --clusters) against the numpy twin of tests/retrieval_km_ref.py.

The assignment is held against the fp64 brute force with the rule of the search tests: where the fp64 gap to the runner-up is
below tol = 4 max|d32 - d64| either index is allowed (tests/test_retrieval_km_cpu.py asserts that fewer than 1 % of the fixtures'
rows are such; the count is printed here) and dist2 stays within tol.  The update, the norms, the counts and the whole k-means run
on the planted mixture are compared bit for bit.  The three stream-taking entries also run on a delayed side stream
(tests/stream_check.py) and inside a captured graph."""
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

import retrieval_km_ref as KM  # noqa: E402
import retrieval_ref as R  # noqa: E402
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


def same_bits(t, a):
    got = t.detach().cpu().numpy()
    return got.shape == a.shape and got.dtype == a.dtype and got.tobytes() == np.ascontiguousarray(a).tobytes()


def bank_of(keys16, values16=None, capacity=None, stats=None):
    b = LatentBank(keys16.shape[1], capacity or keys16.shape[0], key="hr" if values16 is None else "lr")
    if stats is not None:
        b._set_stats(stats)
    b.load_rows(cuda(keys16), None if values16 is None else cuda(values16))
    return b


def norms_of(rows16):
    """the norms the existing bank_norms_kernel gives these fp16 rows"""
    return bank_of(rows16).rows("keys")[1].clone()


@functools.lru_cache(maxsize=None)
def assign_banks(name):
    pool, cent, ref = KM.assign_case(name)
    return bank_of(pool), bank_of(cent), ref


# ---- 1. the assignment against fp64 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(KM.ASSIGN_CASES))
def test_assignment_against_fp64(name):
    pool, cent, ref = assign_banks(name)
    idx, dist2 = cent.assign(pool)
    got, d2 = idx.cpu().numpy(), dist2.cpu().numpy().astype(np.float64)
    assert got.dtype == np.int32 and got.shape == (len(pool),) and got.min() >= 0 and got.max() < len(cent)
    off = got != ref["argmin"]
    print(f"{name}: {int(ref['loose'].sum())} of {len(got)} rows under the near-tie allowance, {int(off.sum())} differ from fp64")
    assert not (off & ~ref["loose"]).any()
    err = np.abs(d2 - np.maximum(ref["d64"][np.arange(len(got)), got], 0))
    print(f"{name}: worst dist2 error {err.max():.3g}, tol {ref['tol']:.3g}")
    assert (err <= ref["tol"]).all()


# ---- 2. ties and edges ----------------------------------------------------------------------------------------------------
def test_duplicated_centroids_give_the_lower_index():
    pool, cent, _ = KM.assign_case("wide")
    K = len(cent)
    double = np.concatenate([cent, cent, cent[:5]])                   # copies 128 + 2 and 2 (128 + 2) rows on: other tiles, waves
    idx, _ = bank_of(double).assign(bank_of(pool))
    one, _ = bank_of(cent).assign(bank_of(pool))
    assert int(idx.max()) < K and torch.equal(idx, one)
    same = np.repeat(cent[7:8], 300, 0)                               # 300 equal rows: every lane's candidate ties
    idx, dist2 = bank_of(same).assign(bank_of(pool))
    assert int(idx.max()) == 0 and same_bits(dist2, bank_of(cent[7:8]).assign(bank_of(pool))[1].cpu().numpy())


def test_one_centroid_and_one_row():
    pool, cent, ref = KM.assign_case("micro")
    idx, dist2 = bank_of(cent[:1]).assign(bank_of(pool))
    assert int(idx.abs().max()) == 0
    assert (np.abs(dist2.cpu().numpy() - np.maximum(ref["d64"][:, 0], 0)) <= ref["tol"]).all()
    idx, dist2 = bank_of(cent).assign(bank_of(pool), first=5, count=1)   # one row of the pool (K <= N holds for the pool)
    assert idx.tolist() == [int(ref["argmin"][5])] and abs(float(dist2) - ref["d64"][5].min()) <= ref["tol"]
    idx, dist2 = bank_of(pool[9:10]).assign(bank_of(pool[9:10]))      # N = K = 1, the row itself
    assert idx.tolist() == [0] and float(dist2) <= ref["tol"]


@pytest.mark.parametrize("name", ["micro", "wide"])
def test_windows_two_runs_and_changed(name):
    pool, cent, ref = assign_banks(name)
    N = len(pool)
    whole_i, whole_d = cent.assign(pool)
    again_i, again_d = cent.assign(pool)
    assert torch.equal(whole_i, again_i) and same_bits(again_d, whole_d.cpu().numpy())
    for first, count in ((0, 1), (1, 63), (37, 130), (N - 1, 1), (64, 64), (5, N - 5), (63, 66), (N - 70, 70)):
        idx, dist2 = cent.assign(pool, first=first, count=count)
        assert torch.equal(idx, whole_i[first:first + count]), (first, count)
        assert same_bits(dist2, whole_d[first:first + count].cpu().numpy()), (first, count)
    # changed: incremented by exactly the entries that differ from what the buffer held, from whatever it held
    held = whole_i.clone()
    wrong = torch.arange(N, device="cuda") % 7 == 3
    held[wrong] = (held[wrong] + 1) % len(cent) if len(cent) > 1 else -1
    held[0] = -1
    expect = int((held != whole_i).sum())
    changed = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    out, _ = cent.assign(pool, idx=held, changed=changed)
    assert out is held and torch.equal(held, whole_i) and int(changed) == 7 + expect and expect > 0
    cent.assign(pool, idx=held, changed=changed)
    assert int(changed) == 7 + expect                                 # nothing differs now
    first, count = 3, N - 10
    part = torch.full((count,), -1, dtype=torch.int32, device="cuda")
    changed.zero_()
    cent.assign(pool, first=first, count=count, idx=part, changed=changed)
    assert int(changed) == count and torch.equal(part, whole_i[first:first + count])


# ---- 3. agreement with the existing search --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(KM.ASSIGN_CASES))
def test_agreement_with_search(name):
    """the search takes the same rows as fp32 queries [1, C, N]: its lo plane is zero and its products are the assignment's, but
    it sums the query's norm itself in another order, so dist2 agrees within tol and idx wherever the fp64 margin exceeds tol"""
    pool_b, cent, ref = assign_banks(name)
    pool = KM.assign_case(name)[0]
    x = cuda(np.ascontiguousarray(pool.astype(np.float32).T)[None])
    s_idx, s_d = cent.search(x)
    a_idx, a_d = cent.assign(pool_b)
    decided = cuda(~ref["loose"])
    assert torch.equal(s_idx[0][decided], a_idx[decided])
    assert float((s_d[0] - a_d).abs().max()) <= 2 * ref["tol"]


# ---- 4. the update against the twin, bit for bit --------------------------------------------------------------------------
def run_update(keys, vals, cent, cvals, idx, check=True):
    pool, cb = bank_of(keys, vals), bank_of(cent, cvals)
    counts = cb.cluster_update(pool, cuda(idx), check=check)
    out = (cb.rows("keys")[0].clone(), cb.rows("values")[0].clone() if vals is not None else None, cb.rows("keys")[1].clone(), counts)
    return out, pool, cb


def check_update(keys, vals, cent, cvals, idx, check=True):
    (gk, gv, gn, gc), _, _ = run_update(keys, vals, cent, cvals, idx, check)
    wk, wc = KM.update(cent, keys, idx)
    assert same_bits(gc, wc) and same_bits(gk, wk)
    assert torch.equal(gn.view(torch.int32), norms_of(wk).view(torch.int32))
    if vals is not None:
        assert same_bits(gv, KM.update(cvals, vals, idx)[0])
    (k2, v2, n2, c2), _, _ = run_update(keys, vals, cent, cvals, idx, check)              # a second run: the scatter order may differ
    assert torch.equal(k2, gk) and torch.equal(n2.view(torch.int32), gn.view(torch.int32)) and torch.equal(c2, gc)
    return wk, wc


@pytest.mark.parametrize("paired", [False, True], ids=["keys", "paired"])
@pytest.mark.parametrize("C_", [32, 96, 1024])
def test_update_equals_the_twin(C_, paired):
    keys, vals, cent, cvals, idx = KM.update_case(C_, paired)
    wk, wc = check_update(keys, vals, cent, cvals, idx)
    assert wc[4] == 0 and wk[4].tobytes() == cent[4].tobytes()                          # the empty cluster kept its row
    # its norm too: the bits it had before
    (_, _, gn, _), _, _ = run_update(keys, vals, cent, cvals, idx)
    assert torch.equal(gn[4:5].view(torch.int32), norms_of(cent)[4:5].view(torch.int32))


def test_update_sum_beyond_2_53():
    """20 000 rows of 65504 and one of 2^-24 in one cluster: S > 2^53"""
    n = 20001
    keys = np.full((n, 32), 65504, np.float16)
    keys[:, 1] = -65504
    keys[-1] = np.float16(2.0 ** -24)
    keys[:, 2] = np.float16(-(2.0 ** -24))
    wk, wc = check_update(keys, None, np.ones((2, 32), np.float16), None, np.zeros(n, np.int32))
    assert wc.tolist() == [n, 0] and float(wk[0, 0]) == 65504.0 and float(wk[0, 2]) == -(2.0 ** -24)


def test_update_rounds_the_sum_to_nearest():
    """the case of tests/test_retrieval_km_cpu.py in which a truncated int64 -> double conversion gives 48000 and the defined one
    48032, in channel 0; the negated values in channel 1"""
    col = np.array([48000.0] * 11879 + [48032.0] * 20886 + [2.0 ** -24] * 3, np.float16)
    keys = np.zeros((len(col), 32), np.float16)
    keys[:, 0], keys[:, 1] = col, -col
    order = (np.arange(len(col)) * 7919) % len(col)                                     # the members in no particular order
    wk, _ = check_update(keys[order], None, np.zeros((1, 32), np.float16), None, np.zeros(len(col), np.int32))
    assert float(wk[0, 0]) == 48032.0 and float(wk[0, 1]) == -48032.0


def test_update_with_one_cluster_holding_most_of_the_pool():
    N, C_, K = 6000, 96, 5
    keys = (recipe.gaussian("km_big_keys", (N, C_), 0) * 4.0).astype(np.float16)
    idx = (np.arange(N) % 10 == 0) * (1 + np.arange(N) // 10 % 3)                       # 90 % in cluster 0, the rest in 1..3
    assert (idx == 0).sum() == 5400
    wk, wc = check_update(keys, None, keys[:K].copy(), None, idx.astype(np.int32))
    assert wc.tolist() == [5400, 200, 200, 200, 0]


def test_update_skips_indices_outside_the_clusters():
    keys, vals, cent, cvals, idx = KM.update_case(32, False)
    bad = idx.copy()
    bad[[10, 20, 30]] = [-1, 9, 2 ** 31 - 1]
    wk, wc = check_update(keys, None, cent, None, bad, check=False)
    assert wc.sum() == len(idx) - 3
    with pytest.raises(ValueError, match="outside"):
        bank_of(cent).cluster_update(bank_of(keys), cuda(bad))


# ---- 5. the inertia -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 1023, 1025, 70001])
def test_inertia(n):
    d = np.abs(recipe.gaussian("km_inertia", (n,), n)) * 3.0
    want = d.astype(np.float64).sum()
    got = RT.sum_dist2(cuda(d))
    assert got.dtype == torch.float64 and abs(float(got) - want) <= n * 2.0 ** -52 * want
    assert torch.equal(got.view(torch.int64), RT.sum_dist2(cuda(d)).view(torch.int64))


# ---- 6. the planted mixture -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("duplicates", [False, True], ids=["planted", "duplicated-seeds"])
def test_planted_mixture(duplicates):
    pool16, truth = KM.planted(duplicates)
    twin = KM.kmeans(pool16, KM.PLANTED["K"], iters=10)
    pool = bank_of(pool16, stats=tstats(96, 2))
    bank, report = RT.kmeans(pool, KM.PLANTED["K"], iters=10)
    assert same_bits(bank.rows("keys")[0], twin["keys"])                                 # the whole run, bit for bit
    assert torch.equal(bank.rows("keys")[1].view(torch.int32), norms_of(twin["keys"]).view(torch.int32))
    assert report["clusters"] == 24 and report["kept"] == len(twin["keep"]) == len(bank) == (23 if duplicates else 24)
    assert report["rows"] == 2000 and report["changed"] == twin["changed"] and report["iterations"] == len(twin["changed"])
    sizes = sorted(int(twin["counts"][i]) for i in twin["keep"])
    assert (report["size_min"], report["size_median"], report["size_max"]) == (sizes[0], sizes[len(sizes) // 2], sizes[-1])
    idx, _ = bank.assign(pool)
    planted = np.searchsorted(np.array(twin["keep"]), truth)                             # centroid order after the drop
    assert np.array_equal(idx.cpu().numpy(), planted)                                    # every row in its planted cluster
    assert bank.key == "hr" and RT.same_stats(bank.stats, pool.stats)
    # inertia: within the fp32 evaluation error of the twin's, and it never rises by more than the centroids' fp16 rounding
    # allows.  A centroid c' = c + e with |e_c| <= 2^-11 |c_c| around the exact mean c of n members costs n |e|^2 more than c
    # (the cross term vanishes at the mean): at most N C (2^-11 max|c|)^2 over the pool; each recorded value is a sum of N
    # distances evaluated within tol.
    N, C_ = 2000, 96
    for got, want, tol in zip(report["inertia"], twin["inertia"], twin["tol"]):
        assert abs(got - want) <= N * tol
    for t in range(1, len(report["inertia"])):
        bound = N * C_ * (2.0 ** -11 * twin["max_abs"][t]) ** 2 + N * (twin["tol"][t] + twin["tol"][t - 1])
        assert report["inertia"][t] <= report["inertia"][t - 1] + bound
    again, report2 = RT.kmeans(pool, KM.PLANTED["K"], iters=10)
    assert torch.equal(again.rows("keys")[0], bank.rows("keys")[0]) and report2 == report   # inertia included: reproducible


def test_kmeans_of_a_paired_pool_and_without_dropping():
    pool16, _ = KM.planted(True)
    vals16 = (recipe.gaussian("km_planted_vals", pool16.shape, 3)).astype(np.float16)
    twin = KM.kmeans(pool16, 24, iters=3, values16=vals16, drop_empty=False)
    bank, report = RT.kmeans(bank_of(pool16, vals16), 24, iters=3, drop_empty=False)
    assert len(bank) == 24 and report["kept"] == 24 and report["size_min"] == 0 and bank.key == "lr"
    assert same_bits(bank.rows("keys")[0], twin["keys"]) and same_bits(bank.rows("values")[0], twin["values"])


# ---- 7. still an ordinary bank --------------------------------------------------------------------------------------------
def test_a_clustered_bank_is_an_ordinary_bank(tmp_path):
    pool16, _ = KM.planted()
    ts = tstats(96, 2)
    twin = KM.kmeans(pool16, 24, iters=10)
    bank, _ = RT.kmeans(bank_of(pool16, stats=ts), 24)
    plain = bank_of(twin["keys"], stats=ts)
    x = cuda(recipe.gaussian("km_queries", (2, 96, 33), 0) * 2.0)
    for a, b in zip(bank.search(x, ts["hr_mean"], ts["hr_std"]), plain.search(x, ts["hr_mean"], ts["hr_std"])):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    for k in (1, 3):
        assert torch.equal(bank.retrieve(x, 0.4, stats=ts, k=k).view(torch.int32), plain.retrieve(x, 0.4, stats=ts, k=k).view(torch.int32))
    bank.save(tmp_path / "km.pt")
    back = RT.load_bank(tmp_path / "km.pt")
    assert isinstance(back, LatentBank) and torch.load(tmp_path / "km.pt", weights_only=False)["format"] == 1
    assert torch.equal(back.rows("keys")[0], bank.rows("keys")[0])
    ms = MultiScaleBank.__new__(MultiScaleBank)
    ms.scales, ms.weights = (1, 2), RT.check_scale_weights(None, 2)
    ms._adopt([bank, plain])
    ms.save(tmp_path / "km_ms.pt")
    back = RT.load_bank(tmp_path / "km_ms.pt")
    assert isinstance(back, MultiScaleBank) and torch.equal(back.banks[1].rows("keys")[0], bank.rows("keys")[0])
    assert torch.equal(back.retrieve(x, 0.4, stats=ts).view(torch.int32), ms.retrieve(x, 0.4, stats=ts).view(torch.int32))


def write_data_dir(root, Cc, lengths):
    os.makedirs(root / "train")
    for i, n in enumerate(lengths):
        jio.save_latent_file(root / "train" / f"f{i}.pt", hr_latent=torch.from_numpy(recipe.gaussian("km_dir_hr", (Cc, n), i)),
                             lr_latent=torch.from_numpy(recipe.gaussian("km_dir_lr", (Cc, n), i)))
    st = R.stats(Cc, 31)
    (root / "global_stats_separated.json").write_text(json.dumps({k: [float(v) for v in a] for k, a in st.items()}))
    return jio.load_stats(root / "global_stats_separated.json", channels=Cc)


def test_build_with_clusters_and_infer(tmp_path):
    from jatsr_amd.infer import main as infer_main
    cfg = recipe.CONFIGS["micro"]
    Cc, T = cfg["input_channels"], 200
    lengths = [90, 50, 77]
    stats = write_data_dir(tmp_path / "data", Cc, lengths)
    base = ["build", "--data-dir", str(tmp_path / "data")]
    RT.main(base + ["--out", str(tmp_path / "km.pt"), "--clusters", "12", "--kmeans-iters", "4"])
    RT.main(base + ["--out", str(tmp_path / "km100.pt"), "--clusters", "10", "--pool-frames", "100", "--key", "lr"])
    RT.main(base + ["--out", str(tmp_path / "km_ms.pt"), "--clusters", "9", "--scales", "1,2"])
    RT.main(base + ["--out", str(tmp_path / "plain.pt"), "--max-frames", "100"])
    report = json.load(open(str(tmp_path / "km.pt") + ".kmeans.json"))
    km = RT.load_bank(tmp_path / "km.pt")
    assert isinstance(km, LatentBank) and report["rows"] == sum(lengths) and report["clusters"] == 12
    assert len(km) == report["kept"] <= 12 and 1 <= report["iterations"] <= 4 and len(report["inertia"]) == report["iterations"]
    # the pool is every frame; the twin from the same rows
    rows = np.concatenate([R.pack_rows(recipe.gaussian("km_dir_hr", (Cc, n), i).astype(np.float16), stats["hr_mean"].numpy(),
                                       stats["hr_std"].numpy()) for i, n in enumerate(lengths)])
    twin = KM.kmeans(rows, 12, iters=4)
    if all(g > t for g, t in zip(twin["gap"], twin["tol"])):                             # no near tie met: the twin's rows
        assert same_bits(km.rows("keys")[0], twin["keys"])
    r100 = json.load(open(str(tmp_path / "km100.pt") + ".kmeans.json"))
    assert r100["rows"] == sum(c for _, _, c in RT.frame_plan(lengths, 100)) <= 100 and RT.load_bank(tmp_path / "km100.pt").key == "lr"
    ms = RT.load_bank(tmp_path / "km_ms.pt")
    rms = json.load(open(str(tmp_path / "km_ms.pt") + ".kmeans.json"))
    assert isinstance(ms, MultiScaleBank) and len(ms) == 9 and len(rms) == 2 and all(r["clusters"] == 9 for r in rms)
    assert not os.path.exists(str(tmp_path / "plain.pt") + ".kmeans.json") and len(RT.load_bank(tmp_path / "plain.pt")) <= 100
    for bad in (["--clusters", "0"], ["--pool-frames", "50"], ["--clusters", "5", "--kmeans-iters", "0"],
                ["--clusters", "1000"]):
        with pytest.raises((SystemExit, ValueError)):
            RT.main(base + ["--out", str(tmp_path / "bad.pt")] + bad)
    assert not os.path.exists(tmp_path / "bad.pt")
    torch.save({"model_state_dict": {k: torch.from_numpy(v) for k, v in recipe.make_state_dict(cfg).items()},
                "config": dict(cfg)}, tmp_path / "last.pt")
    jio.save_latent_file(tmp_path / "clip.pt", hr_latent=torch.from_numpy(recipe.gaussian("rt_inf_hr", (Cc, T), 1)),
                         lr_latent=torch.from_numpy(recipe.gaussian("rt_inf_lr", (Cc, T), 2)))
    common = ["--checkpoint", str(tmp_path / "last.pt"), "--input-file", str(tmp_path / "clip.pt"), "--stats-file",
              str(tmp_path / "data" / "global_stats_separated.json"), "--steps", "2", "--cfg-scale", "2.0", "--seed", "3",
              "--index-rate", "0.5"]
    infer_main(common + ["--index-bank", str(tmp_path / "km.pt"), "--output-dir", str(tmp_path / "o1")])
    infer_main(common + ["--index-bank", str(tmp_path / "km_ms.pt"), "--output-dir", str(tmp_path / "o2")])
    name = "clip_generated_cfg2.0_idx.pt"
    f1 = torch.load(tmp_path / "o1" / name, weights_only=False)
    f2 = torch.load(tmp_path / "o2" / name, weights_only=False)
    assert f1["metadata"]["bank_rows"] == len(km) and f2["metadata"]["index_scales"] == [1, 2]
    plain = torch.load(tmp_path / "o1" / "clip_generated_cfg2.0.pt", weights_only=False)["generated_latent"]
    assert not torch.equal(f1["generated_latent"], plain) and torch.isfinite(f1["generated_latent"]).all()


# ---- 8. streams and graphs ------------------------------------------------------------------------------------------------
def raw_assign(pool, cent, first, count, idx, dist2, changed, work):
    return L.lib().jat_bank_assign(pool._h, first, count, cent._h, L.ptr(idx), L.ptr(dist2), L.ptr(changed), L.ptr(work),
                                   256 if work is None else work.numel(), L.stream_ptr())


def raw_update(pool, idx, cent, counts, work):
    return L.lib().jat_bank_cluster_update(pool._h, L.ptr(idx), cent._h, L.ptr(counts), L.ptr(work), work.numel(), L.stream_ptr())


def update_work(pool, K):
    n = C.c_size_t()
    assert L.lib().jat_bank_cluster_update_workspace_bytes(pool._h, K, C.byref(n)) == 0
    return torch.empty(n.value, dtype=torch.uint8, device="cuda")


def stream_cases():
    Cc, N, K = 96, 333, 11

    def gen(shape, salt):
        return cuda(recipe.gaussian("km_stream", tuple(shape), salt).astype(np.float16))

    def fresh(live, outs):
        return LatentBank(Cc, N), LatentBank(Cc, K)                     # created before the delay starts; filled on the stream

    def banks(st, live):
        pool, cent = st
        pool.load_rows(live["pool"])
        cent.load_rows(live["cent"])
        return pool, cent

    def assign():
        def call(st, i, o):
            pool, cent = banks(st, i)
            assert raw_assign(pool, cent, 3, N - 5, o["idx"], o["dist2"], i["changed"], o["work"]) == 0
            return {"wrapper": cent.assign(pool)[0]}
        return Case({"pool": gen((N, Cc), 1), "cent": gen((K, Cc), 2), "changed": torch.full((1,), 5, dtype=torch.int32, device="cuda")},
                    call, outputs={"idx": torch.empty(N - 5, dtype=torch.int32, device="cuda"), "dist2": torch.empty(N - 5, device="cuda"),
                                   "work": torch.empty(256, dtype=torch.uint8, device="cuda")},
                    decoys={"changed": torch.full((1,), 1000, dtype=torch.int32, device="cuda")}, state=fresh)

    def update():
        idx = cuda((np.arange(N) * 7 % K).astype(np.int32))

        def call(st, i, o):
            pool, cent = banks(st, i)
            assert raw_update(pool, i["idx"], cent, o["counts"], update_work(pool, K)) == 0
            return {"rows": cent.rows("keys")[0].clone(), "norms": cent.rows("keys")[1].clone()}
        return Case({"pool": gen((N, Cc), 3), "cent": gen((K, Cc), 4), "idx": idx}, call,
                    outputs={"counts": torch.empty(K, dtype=torch.int32, device="cuda")},
                    decoys={"idx": cuda((np.arange(N) * 5 % K).astype(np.int32))}, state=fresh)

    def total():
        def call(st, i, o):
            assert L.lib().jat_bank_sum_dist2(L.ptr(i["d"]), i["d"].numel(), L.ptr(o["sum"]), L.stream_ptr()) == 0
            return {"wrapper": RT.sum_dist2(i["d"])}
        return Case({"d": cuda(np.abs(recipe.gaussian("km_stream_d", (5000,), 0)))}, call,
                    outputs={"sum": torch.empty(1, dtype=torch.float64, device="cuda")})

    return {"jat_bank_assign": assign, "jat_bank_cluster_update": update, "jat_bank_sum_dist2": total}


def test_every_stream_taking_entry_has_a_case():
    header = open(os.path.join(ROOT, "include", "jat_hip_km.h")).read()
    import re
    takes = set(re.findall(r"\bint (jat_[a-z0-9_]+)\([^;]*void\* stream\)", header))
    assert takes == set(stream_cases()) and len(takes) == 3


@pytest.mark.parametrize("name", ["jat_bank_assign", "jat_bank_cluster_update", "jat_bank_sum_dist2"])
def test_side_stream(name):
    check_case(stream_cases()[name](), name, synchronises=False)


def test_graph_capture():
    """one k-means iteration (assign, inertia, update) captured into a graph and replayed: no allocation, synchronisation or copy"""
    pool16, _ = KM.planted()
    K = 24
    pool = bank_of(pool16)
    seeds = pool16[KM.seed_positions(len(pool16), K)]
    cent = bank_of(seeds[::-1].copy())                                 # not the order the rows favour: the first pass moves every centroid
    N = len(pool)
    idx = torch.full((N,), -1, dtype=torch.int32, device="cuda")
    dist2, changed = torch.zeros(N, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    counts, total = torch.zeros(K, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.float64, device="cuda")
    awork, uwork = torch.empty(256, dtype=torch.uint8, device="cuda"), update_work(pool, K)

    def run():
        assert raw_assign(pool, cent, 0, N, idx, dist2, changed, awork) == 0
        assert L.lib().jat_bank_sum_dist2(L.ptr(dist2), N, L.ptr(total), L.stream_ptr()) == 0
        assert raw_update(pool, idx, cent, counts, uwork) == 0
    run()                                                              # the first iteration, eagerly
    torch.cuda.synchronize()
    first = cent.rows("keys")[0].clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    g.replay()                                                         # capturing ran nothing: this is the second iteration
    torch.cuda.synchronize()
    twin1, _ = KM.update(seeds[::-1], pool16, KM.assign_reference(pool16, seeds[::-1])["argmin"])
    ref2 = KM.assign_reference(pool16, twin1)
    twin2, counts2 = KM.update(twin1, pool16, ref2["argmin"])
    assert same_bits(first, twin1) and same_bits(cent.rows("keys")[0], twin2) and same_bits(counts, counts2)
    assert int(changed) == N + int((ref2["argmin"] != KM.assign_reference(pool16, seeds[::-1])["argmin"]).sum())
    assert abs(float(total) - np.maximum(ref2["d64"].min(1), 0).sum()) <= N * ref2["tol"]


# ---- 9. the fp16-operand library ------------------------------------------------------------------------------------------
def small_run():
    """assign, update (paired) and a whole k-means run at C = 96"""
    pool, cent, _ = KM.assign_case("slab")
    idx, dist2 = bank_of(cent).assign(bank_of(pool))
    keys, vals, c0, cv, uidx = KM.update_case(96, True)
    (uk, uv, un, uc), _, _ = run_update(keys, vals, c0, cv, uidx)
    bank, report = RT.kmeans(bank_of(KM.planted()[0]), 24)
    return {"idx": idx.cpu().numpy(), "dist2": dist2.cpu().numpy(), "uk": uk.cpu().numpy(), "uv": uv.cpu().numpy(),
            "un": un.cpu().numpy(), "uc": uc.cpu().numpy(), "km": bank.rows("keys")[0].cpu().numpy(),
            "inertia": np.array(report["inertia"])}


def test_fp16_library_gives_the_same_bits(tmp_path):
    """retrieval_km.hip uses fp16 MFMA and integer sums in both builds: libjat_hip_fp16.so (a child process) computes what this
    process computes"""
    code = ("import sys, numpy as np\n"
            "sys.path.insert(0, 'tests')\n"
            "import jatsr_amd._lib as L\n"
            "from test_retrieval_km_gpu import small_run\n"
            "assert L.operand_dtype() == 'fp16'\n"
            "np.savez(sys.argv[1], **small_run())\n")
    env = dict(os.environ, JAT_OPERAND_DTYPE="fp16")
    env.pop("JAT_LIB_PATH", None)
    path = str(tmp_path / "fp16.npz")
    out = subprocess.run([sys.executable, "-c", code, path], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
    other, here = dict(np.load(path)), small_run()
    assert sorted(other) == sorted(here) and len(here) == 8
    for k, v in here.items():
        assert v.tobytes() == other[k].tobytes(), k


# ---- 10. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_in_python():
    pool16, cent16, _ = KM.assign_case("micro")
    pool, cent = bank_of(pool16), bank_of(cent16)
    with pytest.raises(ValueError, match="paired"):
        bank_of(cent16, cent16).assign(pool)                                             # mixed pairedness
    with pytest.raises(ValueError, match="channels"):
        bank_of(np.zeros((3, 64), np.float16)).assign(pool)
    with pytest.raises(ValueError, match="centroids for a pool"):
        pool.assign(cent)                                                                # K = 300 > N = 7
    with pytest.raises(ValueError, match="same bank"):
        pool.assign(pool)
    for first, count in ((-1, 5), (0, 0), (0, 301), (300, 1), (299, 2)):
        with pytest.raises(ValueError):
            cent.assign(pool, first=first, count=count)
    with pytest.raises(ValueError, match="idx"):
        cent.assign(pool, idx=torch.zeros(299, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="idx"):
        cent.assign(pool, idx=torch.zeros(300, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="changed"):
        cent.assign(pool, changed=torch.zeros(2, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="idx"):
        cent.cluster_update(pool, torch.zeros(299, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="clusters for a pool"):
        RT.kmeans(pool, 301)
    for bad in (0, 2.0, True):
        with pytest.raises(ValueError, match="clusters"):
            RT.kmeans(pool, bad)
    with pytest.raises(ValueError, match="iters"):
        RT.kmeans(pool, 3, iters=0)
    with pytest.raises(ValueError, match="dist2"):
        RT.sum_dist2(torch.zeros(0, device="cuda"))


def test_refusals_through_the_raw_abi():
    lib = L.lib()
    pool16, cent16, _ = KM.assign_case("micro")
    pool, cent = bank_of(pool16), bank_of(cent16)
    N, K = len(pool), len(cent)
    idx = torch.full((N,), 3, dtype=torch.int32, device="cuda")
    dist2 = torch.full((N,), 7.0, device="cuda")
    counts = torch.full((K,), 5, dtype=torch.int32, device="cuda")
    work, uwork = torch.empty(256, dtype=torch.uint8, device="cuda"), update_work(pool, K)
    before = cent.rows("keys")[0].clone()
    n = C.c_size_t()
    assert lib.jat_bank_assign_workspace_bytes(pool._h, cent._h, N, C.byref(n)) == 0 and n.value == 256
    assert raw_assign(pool, cent, 0, N, idx, dist2, None, work[:255]) == INV                       # a short workspace
    assert raw_assign(pool, cent, 0, N, idx, dist2, None, None) == INV
    assert L.lib().jat_bank_assign(pool._h, 0, N, cent._h, None, L.ptr(dist2), None, L.ptr(work), 256, L.stream_ptr()) == INV
    for first, count in ((-1, 5), (0, 0), (0, N + 1), (N, 1), (N - 1, 2), (1, N)):
        assert raw_assign(pool, cent, first, count, idx, dist2, None, work) == INV, (first, count)
    assert raw_assign(cent, pool, 0, K, idx, dist2, None, work) == INV                             # K > N
    assert raw_assign(pool, pool, 0, N, idx, dist2, None, work) == INV
    paired, wide = bank_of(cent16, cent16), bank_of(np.zeros((3, 64), np.float16))
    assert raw_assign(pool, paired, 0, N, idx, dist2, None, work) == INV                           # mixed pairedness
    assert raw_assign(pool, wide, 0, N, idx, dist2, None, work) == INV                             # mixed channels
    assert raw_assign(pool, LatentBank(32, 4), 0, N, idx, dist2, None, work) == L.JAT_E_STATE      # no centroids yet
    assert lib.jat_bank_assign_workspace_bytes(pool._h, paired._h, N, C.byref(n)) == INV
    assert lib.jat_bank_assign_workspace_bytes(pool._h, cent._h, 0, C.byref(n)) == INV
    assert lib.jat_bank_assign_workspace_bytes(pool._h, cent._h, 2 ** 22 + 1, C.byref(n)) == INV
    assert lib.jat_bank_assign_workspace_bytes(pool._h, cent._h, N, None) == INV
    # the update
    assert lib.jat_bank_cluster_update_workspace_bytes(pool._h, K, C.byref(n)) == 0 and n.value == uwork.numel() >= 4 * (N + 2 * K)
    assert lib.jat_bank_cluster_update_workspace_bytes(pool._h, N + 1, C.byref(n)) == INV          # K > N
    assert lib.jat_bank_cluster_update_workspace_bytes(pool._h, 0, C.byref(n)) == INV
    assert lib.jat_bank_cluster_update_workspace_bytes(pool._h, K, None) == INV
    assert raw_update(pool, idx, cent, counts, uwork[:-1]) == INV                                  # a short workspace
    assert raw_update(pool, None, cent, counts, uwork) == INV
    assert raw_update(pool, idx, cent, None, uwork) == INV
    assert raw_update(pool, idx, paired, counts, uwork) == INV
    assert raw_update(pool, idx, wide, counts, uwork) == INV
    assert raw_update(cent, idx, pool, counts, uwork) == INV                                       # K > N
    assert raw_update(pool, idx, pool, counts, uwork) == INV
    # N > 2^22: a real pool of 2^22 + 1 rows of 32 channels (268 MB of zeros)
    big = LatentBank(32, 2 ** 22 + 1)
    big.load_rows(torch.zeros(2 ** 22 + 1, 32, dtype=torch.float16, device="cuda"))
    bidx = torch.zeros(4, dtype=torch.int32, device="cuda")
    assert raw_assign(big, cent, 0, 4, bidx, None, None, work) == INV and b"2^22" in lib.jat_last_error()
    assert lib.jat_bank_cluster_update_workspace_bytes(big._h, K, C.byref(n)) == INV
    assert raw_update(big, bidx, cent, counts, uwork) == INV
    del big
    d = L.lib().jat_bank_sum_dist2
    total = torch.full((1,), 9.0, dtype=torch.float64, device="cuda")
    assert d(None, 5, L.ptr(total), L.stream_ptr()) == INV and d(L.ptr(dist2), 0, L.ptr(total), L.stream_ptr()) == INV
    assert d(L.ptr(dist2), N, None, L.stream_ptr()) == INV and d(L.ptr(dist2), 2 ** 31, L.ptr(total), L.stream_ptr()) == INV
    torch.cuda.synchronize()                                                                       # nothing was launched
    assert (idx == 3).all() and (dist2 == 7.0).all() and (counts == 5).all() and float(total) == 9.0
    assert torch.equal(cent.rows("keys")[0], before)
    # a bad idx entry is checked on the device: skipped, never an address
    idx[5], idx[6] = -7, K
    assert raw_update(pool, idx, cent, counts, uwork) == 0
    assert int(counts.sum()) == N - 2 and int(counts[3]) == N - 2
