"""Host side of k-means compaction, no GPU: the five entry points are declared in include/jat_hip_km.h (and in no
other header), bound in `_lib.KM_SIGNATURES` and exported from both libraries; the twin of tests/retrieval_km_ref.py on examples
worked by hand, at the two roundings of the mean (a sum beyond 2^53, and one whose int64 -> double rounding decides the fp16
result), with an empty cluster; the seed positions; the command line; the file format; the refusals that come before any device
call; and the margins of the fixtures the GPU tests share: fewer than 1 % of the assignment fixtures' rows may fall under the
near-tie allowance, and no row of the planted mixtures may."""
import ctypes
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

import jatsr_amd
import retrieval_km_ref as KM
import retrieval_ref as R
from jatsr_amd import _lib
from jatsr_amd import retrieval as RT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jatsr-just-audio-transformer-super-solution_amd", "csrc")
SYMBOLS = ("jat_bank_assign_workspace_bytes", "jat_bank_assign", "jat_bank_cluster_update_workspace_bytes",
           "jat_bank_cluster_update", "jat_bank_sum_dist2")


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


# ---- symbols ------------------------------------------------------------------------------------------------------------
def test_symbols_declared_bound_and_exported(built):
    header = open(os.path.join(ROOT, "include", "jat_hip_km.h")).read()
    old = "".join(open(os.path.join(ROOT, "include", h)).read() for h in ("jat_hip.h", "jat_hip_ms.h", "jat_hip_harm.h"))
    assert '#include "jat_hip.h"' in header
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.KM_SIGNATURES and name not in _lib.SIGNATURES and name not in _lib.MS_SIGNATURES, name
        assert name not in old, name
        assert getattr(built, name).argtypes == _lib.KM_SIGNATURES[name][1]
    assert set(re.findall(r"\bint (jat_[a-z0-9_]+)\(", header)) == set(_lib.KM_SIGNATURES) == set(SYMBOLS)
    assert int(re.search(r"#define JAT_KM_MAX_POOL (\d+)", header).group(1)) == _lib.KM_MAX_POOL == 2 ** 22
    assert [len(_lib.KM_SIGNATURES[n][1]) for n in SYMBOLS] == [4, 10, 3, 7, 4]
    for so in ("libjat_hip.so", "libjat_hip_fp16.so"):
        nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(CSRC, so)], capture_output=True, text=True,
                            check=True).stdout
        exported = set(re.findall(r" T (jat_[a-z0-9_]+)", nm))
        assert set(SYMBOLS) <= exported, (so, set(SYMBOLS) - exported)
    assert "kmeans" in jatsr_amd.__all__
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "OBJS += retrieval_km.o jat_retrieval_km.o\n" in mk and "FP16OBJS += retrieval_km_fp16.o jat_retrieval_km_fp16.o\n" in mk
    assert mk.count("../../include/jat_hip_km.h") == 2               # the two %.cpp pattern rules
    assert mk.count("jat_retrieval_km_kernels.h") == 4                # every pattern rule


def test_argument_errors_need_no_gpu(built):
    INV = _lib.JAT_E_INVALID
    n = ctypes.c_size_t()
    assert built.jat_bank_assign_workspace_bytes(None, None, 10, ctypes.byref(n)) == INV
    assert b"null bank" in built.jat_last_error()
    assert built.jat_bank_assign(None, 0, 1, None, None, None, None, None, 0, None) == INV
    assert built.jat_bank_cluster_update_workspace_bytes(None, 3, ctypes.byref(n)) == INV
    assert built.jat_bank_cluster_update(None, None, None, None, None, 0, None) == INV
    assert built.jat_bank_sum_dist2(None, 5, None, None) == INV
    assert b"null buffer" in built.jat_last_error()


# ---- the twin on examples worked by hand -----------------------------------------------------------------------------------
def test_hand_example():
    # C = 2.  pool rows (1, 0), (3, 0), (0, 5), (0, 7), (10, 10); centroids (2, 0) and (0, 6)
    pool = np.array([[1, 0], [3, 0], [0, 5], [0, 7], [10, 10]], np.float16)
    cent = np.array([[2, 0], [0, 6]], np.float16)
    ref = KM.assign_reference(pool, cent)
    assert ref["d64"].tolist() == [[1, 37], [1, 45], [29, 1], [53, 1], [164, 116]]
    assert ref["argmin"].tolist() == [0, 0, 1, 1, 1] and ref["gap"].tolist() == [36, 44, 28, 52, 48] and not ref["loose"].any()
    idx = ref["argmin"]
    new, counts = KM.update(cent, pool, idx)
    assert counts.tolist() == [2, 3]
    assert new.tolist() == [[2.0, 0.0], [float(np.float16(10 / 3)), float(np.float16(22 / 3))]]
    # units: 1.0 is 2^24, the least subnormal is 1, the largest value is 2047 * 2^29, signs kept
    assert KM.units(np.array([1.0, 2.0 ** -24, 65504, -65504, -0.0, -2.0 ** -24], np.float16)).tolist() == \
        [2 ** 24, 1, 2047 * 2 ** 29, -2047 * 2 ** 29, 0, -1]
    # equal distances: the lower index
    tie = KM.assign_reference(np.array([[1, 1]], np.float16), np.array([[5, 5], [1, 3], [3, 1], [1, 3]], np.float16))
    assert tie["argmin"].tolist() == [1] and tie["gap"][0] == 0.0


def exact_mean_row(values):
    """the correctly rounded fp16 of the exact mean, by rational arithmetic: what ONE rounding would give"""
    s = sum(Fraction(float(v)) for v in values) / len(values)
    lo = np.float16(float(s))
    with np.errstate(over="ignore"):
        cands = {float(lo), float(np.nextafter(lo, np.float16(np.inf))), float(np.nextafter(lo, np.float16(-np.inf)))}
    return min(sorted(c for c in cands if np.isfinite(c)), key=lambda c: abs(Fraction(c) - s))


def test_sum_beyond_2_53():
    """20 000 rows of 65504 and one of 2^-24: S = 20000 * 2047 * 2^29 + 1 > 2^53 is exact as an integer and rounds as it enters
    fp64 (to the multiple of 4 below it, so here a truncating conversion gives the same: the next test separates them)"""
    vals = [65504.0] * 20000 + [2.0 ** -24]
    S = sum(int(v) for v in KM.units(np.array(vals, np.float16)))
    assert S == 20000 * 2047 * 2 ** 29 + 1 and S > 2 ** 53 and float(S) != S
    got = KM.mean_row([S], len(vals))
    assert float(got[0]) == exact_mean_row(vals) == 65504.0             # 65504 * 20000 / 20001 = 65500.7; the grid is 32 wide
    pool = np.zeros((len(vals), 32), np.float16)
    pool[:, 0] = vals
    new, counts = KM.update(np.ones((1, 32), np.float16), pool, np.zeros(len(vals), np.int64))
    assert counts.tolist() == [20001] and float(new[0, 0]) == 65504.0 and (new[0, 1:] == 0).all()


def test_the_rounding_of_the_sum_decides_the_fp16_result():
    """11 879 rows of 48000, 20 886 of 48032 and three of 2^-24: n = 2^15 and S = 2^15 (3001 * 2^28 + 2^15) + 3.  To nearest
    even S becomes A + 4 in fp64 (A = S - 3), the quotient lies above the fp32 tie 3001 * 2^28 + 2^15 and rounds up, and the fp16
    result is 48032, the correctly rounded mean.  Truncated, S becomes A, the quotient IS that tie, goes to the even 3001 * 2^28,
    which is the fp16 tie between 48000 and 48032 and goes to the even 48000."""
    vals = [48000.0] * 11879 + [48032.0] * 20886 + [2.0 ** -24] * 3
    n = len(vals)
    S = sum(int(v) for v in KM.units(np.array(vals, np.float16)))
    assert n == 2 ** 15 and S == 2 ** 15 * (3001 * 2 ** 28 + 2 ** 15) + 3 and 2 ** 54 < S < 2 ** 55
    assert float(S) == S + 1                                            # Python's int -> float rounds to nearest even
    assert float(KM.mean_row([S], n)[0]) == 48032.0 == exact_mean_row(vals)
    truncated = (np.float64(S - 3) / np.float64(n)).astype(np.float32) * np.float32(2.0 ** -24)
    assert float(truncated.astype(np.float16)) == 48000.0


def test_empty_cluster_and_bad_indices():
    keys, _, cent, _, idx = KM.update_case(32, False)
    new, counts = KM.update(cent, keys, idx)
    assert counts[4] == 0 and new[4].tobytes() == cent[4].tobytes() and counts.sum() == len(idx) and (counts[[0, 1, 2, 3, 5]] > 0).all()
    assert all(new[i].tobytes() != cent[i].tobytes() for i in range(9) if i != 4)
    bad = idx.copy()
    bad[[10, 20]] = [-1, 9]
    new2, counts2 = KM.update(cent, keys, bad)
    assert counts2.sum() == len(idx) - 2                                # outside [0, K): the row joins no cluster
    # -0 members: the sum is the integer 0 and the mean is +0
    z = KM.update(np.ones((1, 32), np.float16), np.full((4, 32), -0.0, np.float16), np.zeros(4, np.int64))[0]
    assert z.tobytes() == np.zeros((1, 32), np.float16).tobytes()


def test_seed_positions_are_distinct():
    for N, K in ((1, 1), (7, 7), (10, 3), (2000, 24), (2 ** 22, 10000), (4200, 4100), (5, 4)):
        s = RT.seed_positions(N, K)
        assert s == KM.seed_positions(N, K) and len(set(s)) == K and s[0] == 0 and s[-1] < N and s == sorted(s)


# ---- fixtures of the GPU tests --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(KM.ASSIGN_CASES))
def test_fewer_than_one_percent_of_the_fixture_rows_are_near_ties(name):
    pool, cent, ref = KM.assign_case(name)
    loose = int(ref["loose"].sum())
    print(f"{name}: {loose} of {len(pool)} rows have an fp64 margin below tol = {ref['tol']:.3g}; fp32 brute force differs in "
          f"{ref['mismatch32']}")
    assert loose < 0.01 * len(pool)
    assert (ref["argmin"][[i * len(pool) // 3 for i in range(min(3, len(cent)))]] == np.arange(min(3, len(cent)))).all()


@pytest.mark.parametrize("duplicates", [False, True], ids=["planted", "duplicated-seeds"])
def test_planted_mixture_meets_its_margin(duplicates):
    """in every iteration of the twin's run the least fp64 gap to a runner-up that is another row exceeds the tolerance, so an
    assignment within the tolerance is the twin's; every row ends in its planted cluster"""
    pool, truth = KM.planted(duplicates)
    run = KM.kmeans(pool, KM.PLANTED["K"], iters=10)
    print(f"iterations {len(run['changed'])}, changed {run['changed']}, least gap {min(run['gap']):.3g}, tol {max(run['tol']):.3g}")
    assert all(g > 100 * t for g, t in zip(run["gap"], run["tol"]))
    assert np.array_equal(run["idx"], truth) and run["changed"][-1] == 0 and len(run["changed"]) <= 4
    assert run["keep"] == ([0] + list(range(2, 24)) if duplicates else list(range(24)))
    if duplicates:
        assert run["counts"][1] == 0 and run["keys"][0].tobytes() == pool[0].tobytes()


def test_sklearn_agrees_where_it_is_installed():
    """a cross-check only: Lloyd from the same seeds reaches the planted partition"""
    cluster = pytest.importorskip("sklearn.cluster")
    pool, truth = KM.planted()
    seeds = pool[KM.seed_positions(len(pool), 24)].astype(np.float64)
    km = cluster.KMeans(n_clusters=24, init=seeds, n_init=1, algorithm="lloyd").fit(pool.astype(np.float64))
    assert np.array_equal(km.labels_, truth)


# ---- command line and file format -----------------------------------------------------------------------------------------
def test_parser():
    p = RT.build_parser()
    a = p.parse_args(["build", "--data-dir", "d", "--out", "o.pt"])
    assert a.clusters is None and a.pool_frames is None and a.kmeans_iters == 10 and a.max_frames == 100_000
    a = p.parse_args(["build", "--data-dir", "d", "--out", "o.pt", "--clusters", "10000", "--pool-frames", "500000",
                      "--kmeans-iters", "4", "--scales", "1,2"])
    assert (a.clusters, a.pool_frames, a.kmeans_iters, a.scales) == (10000, 500000, 4, (1, 2))
    with pytest.raises(SystemExit):
        p.parse_args(["build", "--data-dir", "d", "--out", "o.pt", "--clusters", "many"])
    for bad in (0, -3, True, 2.5, "7", None):
        with pytest.raises(ValueError, match="clusters"):
            RT.check_clusters(bad)
    assert RT.check_clusters(7) == 7
    assert RT.check_pool_frames(None) == 2 ** 22 and RT.check_pool_frames(5) == 5
    for bad in (0, 2 ** 22 + 1, True, "5"):
        with pytest.raises(ValueError, match="pool_frames"):
            RT.check_pool_frames(bad)


def test_centroid_rows_round_trip_through_the_bank_file(tmp_path):
    """a centroid bank is an ordinary bank: the twin's rows go through pack_state / torch.save / unpack_state unchanged"""
    pool, _ = KM.planted()
    run = KM.kmeans(pool, 24, iters=3)
    st = {k: torch.from_numpy(v) for k, v in R.stats(96, 1).items()}
    for key, values in (("hr", None), ("lr", torch.from_numpy(run["keys"][::-1].copy()))):
        d = RT.pack_state(torch.from_numpy(run["keys"]), values, key, st)
        torch.save(d, tmp_path / "km.pt")
        keys, vals, k, channels, stats = RT.unpack_state(torch.load(tmp_path / "km.pt", weights_only=False))
        assert d["format"] == 1 and (k, channels) == (key, 96) and keys.numpy().tobytes() == run["keys"].tobytes()
        assert (vals is None) == (values is None) and RT.same_stats(stats, st)
    ms = RT.pack_ms_state((1, 2), RT.check_scale_weights(None, 2), [d, d])
    assert ms["format"] == 2 and len(RT.unpack_ms_state(ms)[2]) == 2
