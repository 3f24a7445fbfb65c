"""Host side of top-k latent retrieval, no GPU: the fp64 reference of tests/retrieval_topk_ref.py against RVC's
formula and against the k = 1 reference, the preconditions of the GPU gates of tests/test_retrieval_topk_gpu.py from fp64
alone, the argument checks that come before any device call, and the new symbols in the header, the ctypes table and both
libraries."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import jatsr_amd
import retrieval_ref as R
import retrieval_topk_ref as K
from jatsr_amd import _lib, infer
from jatsr_amd import retrieval as RT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jatsr-just-audio-transformer-super-solution_amd", "csrc")
SYMBOLS = ("jat_bank_topk_workspace_bytes", "jat_bank_search_topk", "jat_bank_blend_topk")


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


# ---- the reference ------------------------------------------------------------------------------------------------------
def test_weights_are_rvc_weights_above_the_floor():
    rng = np.random.RandomState(3)
    for k in (1, 2, 5, 8):
        d = np.sort(rng.uniform(1e-3, 2e3, size=(200, k)).astype(np.float32), axis=1)
        idx = np.arange(k, dtype=np.int32)[None].repeat(200, 0)
        w, want = K.weights(idx, d), K.rvc_weights(d)
        assert np.abs(w.sum(1) - 1).max() <= 1e-12 and w[:, 0].max() == w.max()
        assert (np.abs(w - want) <= 1e-12 * want).all()
    # below the floor a distance counts as the floor; an unused place carries no weight; nothing overflows
    w = K.weights(np.array([0, 1, 2, -1]), np.array([0.0, 1e-9, 1e-6, np.inf], np.float32))
    assert np.allclose(w, [1 / 3, 1 / 3, 1 / 3, 0], rtol=1e-12) and w[3] == 0
    w = K.weights(np.array([4, 5, 6]), np.array([1e30, 1e30, 2e30], np.float32))
    assert np.allclose(w, np.array([1, 1, 0.25]) / 2.25, rtol=1e-6)
    assert (K.weights(np.array([-1, -1]), np.array([np.inf, np.inf], np.float32)) == 0).all()


def test_topk_order_and_short_banks():
    d = np.array([[3.0, 1.0, 1.0, -0.5, 7.0]])
    idx, dist2 = K.topk(d, 3)
    assert idx.tolist() == [[3, 1, 2]] and dist2.tolist() == [[0.0, 1.0, 1.0]]          # ties: the lower index; max(d, 0)
    idx, dist2 = K.topk(d[:, :2], 4)
    assert idx.tolist() == [[1, 0, -1, -1]] and dist2.tolist() == [[1.0, 3.0, np.inf, np.inf]]
    s, ok = K.decided(np.array([[0.0, 1.0, 1.05, 3.0, 9.0]]), 3, 0.1)
    assert ok.tolist() == [[True, False, False]] and s.shape == (1, 4)
    s, ok = K.decided(np.array([[0.0, 1.0, 2.0, 2.05]]), 3, 0.1)                        # rank 2 against rank 3, outside the list
    assert ok.tolist() == [[True, True, False]]


def test_blend_reference_at_k1_is_the_blend_reference():
    C_, N, B, T = 32, 23, 2, 7
    rows = jatsr_amd.recipe.gaussian("rtk_cpu_rows", (N, C_), 0).astype(np.float16)
    st = R.stats(C_, 2)
    x = jatsr_amd.recipe.gaussian("rtk_cpu_x", (B, C_, T), 1)
    idx = (np.arange(B * T).reshape(B, T) * 5 % N).astype(np.int32)
    d = np.abs(jatsr_amd.recipe.gaussian("rtk_cpu_d", (B, T, 1), 2)).astype(np.float32)
    for mean, std in ((None, None), (st["hr_mean"], st["hr_std"])):
        want, _ = R.blend(x, rows, idx, 0.4, mean, std)
        got, bound, w = K.blend_topk(x, rows, idx[..., None], d, 0.4, mean, std)
        assert (w == 1).all() and np.array_equal(got, want) and (bound > 0).all()


# ---- preconditions of the GPU gates -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(R.SEARCH_CASES))
def test_undecided_ranks_are_rare_and_fp32_decides_the_rest(case):
    x, keys, ref, idx64, s, ok = K.topk_case(case)
    n = ok.size
    print(f"{case}: tol {ref['tol']:.3e}, undecided ranks at k = 8: {int((~ok).sum())} of {n}")
    assert n == idx64.size and (idx64 >= 0).all()
    assert (~ok).sum() <= 0.01 * n
    d32 = R.dist(R.queries(x), keys, np.float32)
    for k in (4, 8):
        i32, _ = K.topk(d32, k)
        i64, _ = K.topk(ref["d64"], k)
        _, okk = K.decided(ref["d64"], k, ref["tol"])
        wrong = (i32 != i64) & okk
        print(f"{case} k = {k}: decided ranks the fp32 replica orders differently: {int(wrong.sum())}")
        assert not wrong.any()


# ---- argument checks ----------------------------------------------------------------------------------------------------
def test_index_k_parsing():
    a = infer.build_parser().parse_args([])
    assert a.index_k == 1
    for k in range(1, 9):
        assert infer.build_parser().parse_args(["--index-bank", "b.pt", "--index-k", str(k)]).index_k == k
    for bad in ("0", "9", "-1", "2.5", "eight", ""):
        with pytest.raises(SystemExit):
            infer.build_parser().parse_args(["--index-bank", "b.pt", "--index-k", bad])


@pytest.mark.parametrize("k", [0, 9, -3, 2.5, None, True, "4", float("nan")])
def test_index_k_is_validated_before_anything_runs(k):
    with pytest.raises(ValueError, match="index_k"):
        jatsr_amd.sample_long(None, None, None, None, None, None, bank=object(), index_rate=0.4, index_k=k)
    with pytest.raises(ValueError, match="index_k"):
        RT.check_index_k(k)


def test_index_k_and_floor_values():
    assert [RT.check_index_k(k) for k in (1, 2, 8)] == [1, 2, 8] and _lib.BANK_MAX_K == 8 == K.MAX_K
    assert RT.check_dist2_floor(1e-6) == float(np.float32(1e-6))
    for bad in (0.0, -1e-6, float("nan"), float("inf"), 1e-60):                # 1e-60 is 0 in fp32
        with pytest.raises(ValueError, match="dist2_floor"):
            RT.check_dist2_floor(bad)


def test_symbols_declared_bound_and_exported(built):
    header = open(os.path.join(ROOT, "include", "jat_hip.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.SIGNATURES, name
    assert int(re.search(r"#define JAT_BANK_MAX_K (\d+)", header).group(1)) == _lib.BANK_MAX_K
    for so in ("libjat_hip.so", "libjat_hip_fp16.so"):
        nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(CSRC, so)], capture_output=True, text=True,
                            check=True).stdout
        exported = set(re.findall(r" T (jat_[a-z0-9_]+)", nm))
        assert set(SYMBOLS) <= exported, (so, set(SYMBOLS) - exported)
    assert len(_lib.SIGNATURES["jat_bank_search_topk"][1]) == 12 and len(_lib.SIGNATURES["jat_bank_blend_topk"][1]) == 13


def test_argument_errors_need_no_gpu(built):
    """what jat_retrieval.cpp refuses ahead of any device call"""
    n = ctypes.c_size_t()
    INV = _lib.JAT_E_INVALID
    assert built.jat_bank_topk_workspace_bytes(None, 8, 4, ctypes.byref(n)) == INV
    assert built.jat_bank_search_topk(None, None, None, None, 1, 1, 4, None, None, None, 0, None) == INV
    assert b"null bank" in built.jat_last_error()
    assert built.jat_bank_blend_topk(None, None, None, None, 4, None, None, 0.5, 1e-6, None, 1, 1, None) == INV
    assert b"null bank" in built.jat_last_error()
