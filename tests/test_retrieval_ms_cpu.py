"""Host side of multi-scale latent retrieval, no GPU: the three entry points are declared in include/jat_hip_ms.h (and
nowhere in include/jat_hip.h), bound in `_lib.MS_SIGNATURES` and exported from both libraries; the scale and weight checks; the
format-2 bank dictionary; the twin of tests/retrieval_ms_ref.py against torch's interpolation; the roadmap's rate; the argument
checks that come before any device call; and the margin condition of the end-to-end GPU test's planted fixture."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import jatsr_amd
import retrieval_ms_ref as M
import retrieval_ref as R
from jatsr_amd import _lib, infer
from jatsr_amd import retrieval as RT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jatsr-just-audio-transformer-super-solution_amd", "csrc")
SYMBOLS = ("jat_bank_add_pooled", "jat_bank_pool_frames", "jat_bank_mix_scales")


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


# ---- symbols ------------------------------------------------------------------------------------------------------------
def test_symbols_declared_bound_and_exported(built):
    header = open(os.path.join(ROOT, "include", "jat_hip_ms.h")).read()
    old = open(os.path.join(ROOT, "include", "jat_hip.h")).read()
    assert '#include "jat_hip.h"' in header
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.MS_SIGNATURES and name not in _lib.SIGNATURES, name
        assert name not in old, name
        assert getattr(built, name).argtypes == _lib.MS_SIGNATURES[name][1]
    assert set(re.findall(r"\bint (jat_[a-z0-9_]+)\(", header)) == set(_lib.MS_SIGNATURES)
    assert int(re.search(r"#define JAT_BANK_MAX_SCALES (\d+)", header).group(1)) == _lib.BANK_MAX_SCALES == 4
    assert [len(_lib.MS_SIGNATURES[n][1]) for n in SYMBOLS] == [14, 10, 11]
    for so in ("libjat_hip.so", "libjat_hip_fp16.so"):
        nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(CSRC, so)], capture_output=True, text=True,
                            check=True).stdout
        exported = set(re.findall(r" T (jat_[a-z0-9_]+)", nm))
        assert set(SYMBOLS) <= exported, (so, set(SYMBOLS) - exported)
    for name in ("MultiScaleBank", "load_bank"):
        assert name in jatsr_amd.__all__
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "OBJS += retrieval_ms.o\n" in mk and "FP16OBJS += retrieval_ms_fp16.o\n" in mk
    assert mk.count("../../include/jat_hip_ms.h") == 2              # the two %.cpp pattern rules


# ---- host checks --------------------------------------------------------------------------------------------------------
def test_check_scales():
    for good in ((1,), (1, 2, 4), (2, 8), (1, 2, 4, 8), [4], "1,2,4", "8", " 2, 4 "):
        got = RT.check_scales(good)
        assert isinstance(got, tuple) and all(isinstance(v, int) for v in got)
    assert RT.check_scales("1,2,4") == (1, 2, 4) == RT.check_scales([1, 2, 4]) and RT.scales_arg("2,8") == (2, 8)
    for bad in ((), (3,), (1, 1), (2, 1), (4, 2, 1), (1, 2, 3), (0,), (16,), (1, 2, 4, 8, 8), (-2,), (2.0,), (True,), "1,,2", "",
                "1;2", "a", None, 4, (1, 2, 4, 8, 16)):
        with pytest.raises(ValueError, match="scales"):
            RT.check_scales(bad)
    import argparse
    for bad in ("3", "2,1", "1,2,4,8,8", "x"):
        with pytest.raises(argparse.ArgumentTypeError):
            RT.scales_arg(bad)


def test_check_scale_weights():
    assert RT.check_scale_weights(None, 1) == (1.0,) and RT.check_scale_weights([7.5], 1) == (1.0,)
    third = float(np.float32(1.0 / 3.0))
    assert RT.check_scale_weights(None, 3) == (third,) * 3
    got = RT.check_scale_weights([2, 1, 1], 3)
    assert got == (0.5, 0.25, 0.25) == RT.check_scale_weights("2,1,1", 3)
    for w, n in (([1, 2, 3, 4], 4), ([0.1, 1e3], 2), ([1e-30, 1e-30, 1e-30], 3)):
        got = RT.check_scale_weights(w, n)
        assert np.array_equal(np.array(got, np.float32), M.scale_weights(w, n)) and abs(sum(got) - 1) < 1e-6
        assert all(v == float(np.float32(v)) for v in got)
    for w, n in (([1, 1], 3), ([1, 1, 1], 2), ([1, 0], 2), ([1, -1], 2), ([1, float("nan")], 2), ([1, float("inf")], 2),
                 ("1,x", 2), ([], 1), ([1e-60, 1.0], 2)):
        with pytest.raises(ValueError, match="weights"):
            RT.check_scale_weights(w, n)
    assert RT.scale_weights_arg("2,1,1") == [2.0, 1.0, 1.0]
    import argparse
    for bad in ("0,1", "a", "1,-1", ""):
        with pytest.raises(argparse.ArgumentTypeError):
            RT.scale_weights_arg(bad)


def test_parsers():
    a = infer.build_parser().parse_args([])
    assert a.index_scale_weights is None
    a = infer.build_parser().parse_args(["--index-bank", "b.pt", "--index-scale-weights", "2,1,1"])
    assert a.index_scale_weights == [2.0, 1.0, 1.0]
    with pytest.raises(SystemExit):
        infer.build_parser().parse_args(["--index-bank", "b.pt", "--index-scale-weights", "1,0"])
    b = RT.build_parser().parse_args(["build", "--data-dir", "d", "--out", "o.pt"])
    assert b.scales is None and b.scale_weights is None                       # without --scales: the file as it always was
    b = RT.build_parser().parse_args(["build", "--data-dir", "d", "--out", "o.pt", "--scales", "1,2,4", "--scale-weights", "1,1,2"])
    assert b.scales == (1, 2, 4) and b.scale_weights == [1.0, 1.0, 2.0]
    for bad in ("1,3", "2,1", "1,2,4,8,8"):
        with pytest.raises(SystemExit):
            RT.build_parser().parse_args(["build", "--data-dir", "d", "--out", "o.pt", "--scales", bad])


def test_roadmap_rate():
    """(x + r sum_s up_s) / (1 + n r) is (1 - R) x + R mean_s up_s at R = n r / (1 + n r), in fp64"""
    rng = np.random.RandomState(5)
    for n in (1, 2, 3, 4):
        for r in (0.0, 0.1, 0.4, 1.0, 2.5):
            x, ups = rng.randn(50), rng.randn(n, 50)
            road = (x + r * ups.sum(0)) / (1 + n * r)
            rate = RT.MultiScaleBank.roadmap_rate(r, n)
            assert 0.0 <= rate < 1.0 and rate == n * r / (1 + n * r)
            ours = (1 - rate) * x + rate * ups.mean(0)
            assert np.abs(ours - road).max() <= 1e-14


# ---- the file format ----------------------------------------------------------------------------------------------------
def one_state(n=6, C_=32, key="hr", salt=0):
    g = torch.Generator().manual_seed(salt)
    keys = torch.randn(n, C_, generator=g).half()
    values = torch.randn(n, C_, generator=g).half() if key == "lr" else None
    return RT.pack_state(keys, values, key, R.stats(C_, 4))


@pytest.mark.parametrize("key", ["hr", "lr"])
def test_format_2_round_trip(tmp_path, key):
    banks = [one_state(key=key, salt=i) for i in range(3)]
    w = RT.check_scale_weights([3, 2, 1], 3)
    d = RT.pack_ms_state((1, 2, 4), w, banks)
    assert d["format"] == 2 == RT.FORMAT_MS and RT.FORMAT == 1 and d["scales"] == [1, 2, 4] and d["weights"] == list(w)
    assert all(b["format"] == 1 for b in d["banks"])
    torch.save(d, tmp_path / "ms.pt")
    scales, weights, got = RT.unpack_ms_state(torch.load(tmp_path / "ms.pt", weights_only=False))
    assert scales == (1, 2, 4) and weights == w                                # not normalised a second time
    for a, b in zip(got, banks):
        assert torch.equal(a["keys"], b["keys"]) and a["key"] == key and RT.same_stats(a["stats"], b["stats"])
        assert (a["values"] is None) == (key == "hr") and (key == "hr" or torch.equal(a["values"], b["values"]))
    # equal weights survive as well (three fp32 thirds sum to 1 + 2^-24 or so)
    third = RT.check_scale_weights(None, 3)
    assert RT.unpack_ms_state(RT.pack_ms_state((2, 4, 8), third, banks))[1] == third


def test_format_2_is_refused_where_format_1_is_expected_and_the_reverse(tmp_path):
    banks = [one_state(salt=i) for i in range(2)]
    d = RT.pack_ms_state((1, 4), RT.check_scale_weights(None, 2), banks)
    with pytest.raises(ValueError, match="load_bank"):
        RT.unpack_state(d)
    with pytest.raises(ValueError, match="load_bank"):
        RT.LatentBank.from_state(d)                                            # refused before any device call
    torch.save(d, tmp_path / "ms.pt")
    with pytest.raises(ValueError, match="load_bank"):
        RT.LatentBank.load(tmp_path / "ms.pt")
    with pytest.raises(ValueError, match="format 2"):
        RT.unpack_ms_state(banks[0])
    with pytest.raises(ValueError, match="format 2"):
        RT.MultiScaleBank.from_state(banks[0])
    # malformed format-2 dictionaries
    with pytest.raises(ValueError):
        RT.pack_ms_state((1, 2, 4), RT.check_scale_weights(None, 3), banks)    # three scales, two banks
    with pytest.raises(ValueError, match="weights"):
        RT.pack_ms_state((1, 4), (0.5, 0.25), banks)
    with pytest.raises(ValueError, match="scales"):
        RT.pack_ms_state((4, 1), RT.check_scale_weights(None, 2), banks)
    with pytest.raises(ValueError, match="share"):
        RT.pack_ms_state((1, 4), RT.check_scale_weights(None, 2), [banks[0], one_state(n=7)])
    with pytest.raises(ValueError, match="share"):
        RT.pack_ms_state((1, 4), RT.check_scale_weights(None, 2), [banks[0], one_state(key="lr")])
    with pytest.raises(KeyError):
        RT.unpack_ms_state({"format": 2, "scales": [1, 4], "banks": banks})


# ---- the twin -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [2, 4, 8])
def test_twin_interpolation_is_torchs(s):
    """F.interpolate(mode="linear", align_corners=False) at scale factor s, T a multiple of s.  torch clamps the source
    position at 0 where the twin clamps the two taps: the same value in exact arithmetic, so fp64 agrees to a rounding and
    fp32 to two (the twin rounds (1 - w) v + w v at the edges, torch returns v)."""
    rng = np.random.RandomState(s)
    for Ts in (1, 2, 5, 16):
        v = rng.randn(2, 3, Ts)
        T = Ts * s
        want = torch.nn.functional.interpolate(torch.from_numpy(v), scale_factor=s, mode="linear", align_corners=False).numpy()
        got = M.interp(v.astype(np.float32), s, T, np.float64)
        v32 = v.astype(np.float32).astype(np.float64)
        want32 = torch.nn.functional.interpolate(torch.from_numpy(v32), scale_factor=s, mode="linear", align_corners=False).numpy()
        assert got.shape == want.shape == (2, 3, T)
        assert np.abs(got - want32).max() <= 2.0 ** -52 * np.abs(v32).max()
        got32 = M.interp(v.astype(np.float32), s, T, np.float32)
        assert got32.dtype == np.float32 and np.abs(got32 - want32).max() <= 2 * 2.0 ** -24 * np.abs(v32).max()
    ja, jb, w = M.taps(33, 4)                                                  # T = 33: 9 pooled frames, the last of one frame
    assert ja[:3].tolist() == [0, 0, 0] and jb[:3].tolist() == [0, 0, 1] and w[:4].tolist() == [0.625, 0.875, 0.125, 0.375]
    assert (ja[-1], jb[-1], w[-1]) == (7, 8, 0.625) and jb.max() == 8       # t = 32: p = 7.625, into the one-frame window
    assert (M.taps(1, 8)[0] == 0).all() and (M.taps(3, 4)[1] == 0).all()       # T < s: one pooled frame


def test_twin_pooling_and_mix_basics():
    rng = np.random.RandomState(1)
    x = rng.randn(2, 4, 11).astype(np.float32)
    st = R.stats(4, 2)
    assert np.array_equal(M.pool_queries(x, 1), x)                              # s = 1: the frames themselves
    q = R.normalise(x, st["hr_mean"], st["hr_std"])
    p4 = M.pool_queries(x, 4, st["hr_mean"], st["hr_std"])
    assert p4.shape == (2, 4, 3) and p4.dtype == np.float32
    assert np.array_equal(p4[..., 0], (((q[..., 0] + q[..., 1]) + q[..., 2]) + q[..., 3]) / np.float32(4))
    assert np.array_equal(p4[..., 2], ((q[..., 8] + q[..., 9]) + q[..., 10]) / np.float32(3))      # the cut window: / 3
    p64 = M.pool_queries(x, 4, st["hr_mean"], st["hr_std"], np.float64)
    assert np.abs(p4 - p64).max() < 1e-5
    # window 1 of the pooled pack is the pack
    src = (rng.randn(4, 37) * 3).astype(np.float16)
    assert np.array_equal(M.pool_rows(src, st["hr_mean"], st["hr_std"], 2, 5, 7, 1), R.pack_rows(src, st["hr_mean"], st["hr_std"], 2, 5, 7))
    # the mix: rate 0 is x, a single scale 1 of weight 1 is the blend's last line, the bound holds between the two precisions
    tracks = [rng.randn(2, 4, M.pooled_length(11, s)).astype(np.float32) for s in (1, 2, 4, 8)]
    a = M.scale_weights([1, 2, 3, 4], 4)
    assert np.array_equal(M.mix(x, (1, 2, 4, 8), tracks, a, 0.0), x)
    y1 = M.mix(x, (1,), tracks[:1], M.scale_weights(None, 1), 0.4)
    r = np.float32(0.4)
    assert np.array_equal(y1, M.fma32(np.full_like(x, np.float32(1) - r), x, r * tracks[0]))
    # fma32 is one rounding: against exact rational arithmetic, also where the sum cancels and on rounding ties
    from fractions import Fraction
    fa = np.concatenate([rng.randn(200), [1.0, 1.0 + 2.0 ** -23, 3.0]]).astype(np.float32)
    fb = np.concatenate([rng.randn(200), [1.0 + 2.0 ** -23, 1.0 - 2.0 ** -24, 2.0 ** -25]]).astype(np.float32)
    fc = np.concatenate([-(fa[:200] * fb[:200]).astype(np.float32) * (rng.rand(200) < 0.5), [2.0 ** -48, -1.0, 1.0]]).astype(np.float32)
    for ai, bi, ci, got in zip(fa, fb, fc, M.fma32(fa, fb, fc)):
        exact = Fraction(float(ai)) * Fraction(float(bi)) + Fraction(float(ci))
        lo, hi = np.nextafter(got, np.float32(-np.inf)), np.nextafter(got, np.float32(np.inf))
        err = abs(Fraction(float(got)) - exact)
        assert err <= abs(Fraction(float(lo)) - exact) and err <= abs(Fraction(float(hi)) - exact)
        if err == abs(Fraction(float(lo)) - exact) or err == abs(Fraction(float(hi)) - exact):     # a tie goes to the even one
            assert (np.float32(got).view(np.int32) & 1) == 0
    y32, y64 = M.mix(x, (1, 2, 4, 8), tracks, a, 0.4), M.mix(x, (1, 2, 4, 8), tracks, a, 0.4, np.float64)
    assert (np.abs(y32 - y64) <= M.mix_bound(x, (1, 2, 4, 8), tracks, a, 0.4)).all()
    assert np.array_equal(M.scale_weights(None, 1), [1.0])


# ---- the planted fixture of the end-to-end GPU test ---------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(M.E2E_QUERIES))
def test_planted_fixture_meets_its_margin(name):
    """No query may be excused: for EVERY pooled query at every scale the fp64 nearest row is the planted one and the second
    nearest is at least 1.0 further in squared distance, while the error of an fp32 evaluation of the same distances (tol, the
    gate of tests/test_gpu_retrieval.py) is below 1e-2.  So the nearest index is decided for every query, at k = 1 and as the
    first column at k = 4.  The ranks 2 to 4 of a k = 4 list have no planted margin: there the GPU test applies the rule of
    tests/test_retrieval_topk_gpu.py (a rank whose fp64 gaps to both neighbouring ranks exceed tol must be fp64's), and this
    test shows from fp64 alone that the rule leaves at most 1 % of those ranks undecided."""
    import retrieval_topk_ref as K
    fx = M.e2e_fixture()
    x, truth = M.e2e_queries(name)
    assert all(r.shape == (300, M.E2E_C) and r.dtype == np.float16 for r in fx["rows"].values())
    for s, ref in M.e2e_brute_force(name).items():
        d, order = ref["sorted"], ref["order"]
        assert order.shape == (x.shape[0] * M.pooled_length(x.shape[2], s), 300)
        margin = d[:, 1] - d[:, 0]
        _, ok = K.decided(ref["d64"], 4, ref["tol"])
        print(f"{name} scale {s}: {order.shape[0]} queries, nearest d2 <= {d[:, 0].max():.3f}, least margin to the second "
              f"{margin.min():.3f}, tol {ref['tol']:.2e}, undecided ranks at k = 4: {int((~ok).sum())} of {ok.size}")
        assert np.array_equal(order[:, 0], truth[s].reshape(-1))
        assert (margin >= 1.0).all() and ref["tol"] < 1e-2
        assert ok[:, 0].all() and (~ok).sum() <= 0.01 * ok.size
        assert d[:, 0].max() < 1.0                                              # the noise: 96 x 0.05^2 / s and the fp16 rounding


# ---- argument checks ahead of any device call ---------------------------------------------------------------------------
def test_argument_errors_need_no_gpu(built):
    INV = _lib.JAT_E_INVALID
    assert built.jat_bank_add_pooled(None, None, None, 0, 10, 0, 1, 1, 2, None, None, None, None, None) == INV
    assert b"null bank" in built.jat_last_error()
    two, one = (ctypes.c_int32 * 1)(2), (ctypes.c_int32 * 1)(1)
    ptrs = (ctypes.c_void_p * 1)(4096)
    w = (ctypes.c_float * 1)(1.0)
    X = ctypes.c_void_p(1 << 20)
    assert built.jat_bank_pool_frames(None, None, None, 1, 32, 8, 1, two, ptrs, None) == INV              # null x
    assert built.jat_bank_pool_frames(X, None, None, 1, 48, 8, 1, two, ptrs, None) == INV                 # channels
    assert b"channels" in built.jat_last_error()
    assert built.jat_bank_pool_frames(X, None, None, 1, 32, 0, 1, two, ptrs, None) == INV                 # T = 0
    assert built.jat_bank_pool_frames(X, None, None, 1, 32, 8, 1, one, ptrs, None) == INV                 # scale 1
    assert built.jat_bank_pool_frames(X, None, None, 1, 32, 8, 0, two, ptrs, None) == INV                 # n = 0
    assert built.jat_bank_pool_frames(X, X, None, 1, 32, 8, 1, two, ptrs, None) == INV                    # mean without std
    assert built.jat_bank_mix_scales(None, 1, one, ptrs, w, 0.5, X, 1, 32, 8, None) == INV
    assert built.jat_bank_mix_scales(X, 1, one, ptrs, w, 1.5, ctypes.c_void_p(1 << 22), 1, 32, 8, None) == INV
    assert b"index rate" in built.jat_last_error()
    assert built.jat_bank_mix_scales(X, 1, (ctypes.c_int32 * 1)(3), ptrs, w, 0.5, ctypes.c_void_p(1 << 22), 1, 32, 8, None) == INV
    assert b"scale 3" in built.jat_last_error()
    assert built.jat_bank_mix_scales(X, 1, one, (ctypes.c_void_p * 1)(1 << 22), w, 0.5, ctypes.c_void_p(1 << 22), 1, 32, 8, None) == INV
    assert b"overlaps y" in built.jat_last_error()
    with pytest.raises(ValueError, match="scales"):
        RT.MultiScaleBank(32, 10, scales=(1, 3))                                # refused before the GPU is asked for
    with pytest.raises(ValueError, match="weights"):
        RT.MultiScaleBank(32, 10, scales=(1, 2), weights=[1.0])
