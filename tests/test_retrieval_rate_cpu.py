"""Host side of the voicing-aware index rates, no GPU: the three entry points are declared in include/jat_hip_rate.h
(and in no other header), bound in `_lib.RATE_SIGNATURES` and exported from both libraries; the numpy twins of
tests/retrieval_rate_ref.py on tracks worked by hand; the exact ratio boundary; the difference-form smoothing; the command line
and its refusals; the refusals of the C ABI that come before any launch; and the tone / noise / glide fixture in fp64, whose
inner frames the GPU test classes again."""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import pitch_ref as P
import retrieval_rate_ref as RR
from jatsr_amd import _lib
from jatsr_amd import retrieval as RT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jatsr-just-audio-transformer-super-solution_amd", "csrc")
SYMBOLS = ("jat_f0_classes", "jat_rate_track", "jat_rate_mix")
F32 = np.float32


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


# ---- symbols ------------------------------------------------------------------------------------------------------------
def test_symbols_declared_bound_and_exported(built):
    header = open(os.path.join(ROOT, "include", "jat_hip_rate.h")).read()
    old = "".join(open(os.path.join(ROOT, "include", h)).read()
                  for h in ("jat_hip.h", "jat_hip_ms.h", "jat_hip_harm.h", "jat_hip_km.h", "jat_hip_ivf.h"))
    assert '#include "jat_hip.h"' in header
    others = (_lib.SIGNATURES, _lib.MS_SIGNATURES, _lib.HARM_SIGNATURES, _lib.KM_SIGNATURES, _lib.IVF_SIGNATURES)
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.RATE_SIGNATURES and not any(name in t for t in others), name
        assert name not in old, name
        assert getattr(built, name).argtypes == _lib.RATE_SIGNATURES[name][1]
    assert set(re.findall(r"\bint (jat_[a-z0-9_]+)\(", header)) == set(_lib.RATE_SIGNATURES) == set(SYMBOLS)
    assert int(re.search(r"#define JAT_RATE_MAX_HALF_WINDOW (\d+)", header).group(1)) == _lib.RATE_MAX_HALF_WINDOW == \
        RR.MAX_HALF_WINDOW == 32
    assert int(re.search(r"#define JAT_RATE_MAX_SMOOTH (\d+)", header).group(1)) == _lib.RATE_MAX_SMOOTH == RR.MAX_SMOOTH == 16
    assert [len(_lib.RATE_SIGNATURES[n][1]) for n in SYMBOLS] == [11, 8, 8]
    for so in ("libjat_hip.so", "libjat_hip_fp16.so"):
        nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(CSRC, so)], capture_output=True, text=True,
                            check=True).stdout
        exported = set(re.findall(r" T (jat_[a-z0-9_]+)", nm))
        assert set(SYMBOLS) <= exported, (so, set(SYMBOLS) - exported)
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "OBJS += retrieval_rate.o jat_retrieval_rate.o\n" in mk
    assert "FP16OBJS += retrieval_rate_fp16.o jat_retrieval_rate_fp16.o\n" in mk
    assert mk.count("../../include/jat_hip_rate.h") == 2              # the two %.cpp pattern rules
    assert mk.count("jat_retrieval_rate_kernels.h") == 4              # every pattern rule
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "_lib.RATE_SIGNATURES" in entry                            # build() checks the new symbols


def test_existing_kernel_sources_are_not_restated():
    """the per-frame rate is one new kernel behind the existing blends, not a copy of them"""
    src = open(os.path.join(CSRC, "retrieval_rate.hip")).read()
    assert "mfma" not in src and "atomic" not in src.lower().replace("no atomics", "")
    assert "#pragma clang fp contract(off)" in src


def test_abi_refusals_need_no_gpu(built):
    """every refusal comes before the launch, so the pointers are never read: small host integers stand in for buffers"""
    INV = _lib.JAT_E_INVALID
    p = ctypes.c_void_p(4096)
    rates = (ctypes.c_float * 3)(0.1, 0.2, 0.3)
    ok = dict(f0=p, voiced=p, B=1, F=8, W=4, ratio=1.03, m=7, cls=p)

    def classes(**kw):
        a = dict(ok, **kw)
        return built.jat_f0_classes(a["f0"], a["voiced"], a["B"], a["F"], a["W"], a["ratio"], a["m"], a["cls"], None, None, None)
    for bad in (dict(f0=None), dict(voiced=None), dict(cls=None), dict(B=0), dict(B=65536), dict(F=0), dict(W=-1), dict(W=33),
                dict(m=0), dict(m=10), dict(W=0, m=2), dict(ratio=1.0), dict(ratio=0.5), dict(ratio=float("inf")),
                dict(ratio=float("nan"))):
        assert classes(**bad) == INV, bad
        assert b"jat_f0_classes" in built.jat_last_error()

    def track(cls=p, B=1, F=8, T=8, table=rates, S=2, r=p):
        return built.jat_rate_track(cls, B, F, T, table, S, r, None)
    for bad in (dict(cls=None), dict(table=None), dict(r=None), dict(B=0), dict(F=0), dict(T=0), dict(S=-1), dict(S=17),
                dict(table=(ctypes.c_float * 3)(0.1, 1.5, 0.3)), dict(table=(ctypes.c_float * 3)(-0.1, 0.5, 0.3)),
                dict(table=(ctypes.c_float * 3)(0.1, 0.5, float("nan"))), dict(table=(ctypes.c_float * 3)(float("inf"), 0.5, 0.3))):
        assert track(**bad) == INV, bad
        assert b"jat_rate_track" in built.jat_last_error()

    def mix(x=p, v=ctypes.c_void_p(1 << 20), rates=ctypes.c_void_p(1 << 21), y=ctypes.c_void_p(1 << 22), B=1, C=4, T=8):
        return built.jat_rate_mix(x, v, rates, y, B, C, T, None)
    for bad in (dict(x=None), dict(v=None), dict(rates=None), dict(y=None), dict(B=0), dict(C=0), dict(T=0),
                dict(y=ctypes.c_void_p(4096 + 16)), dict(y=ctypes.c_void_p((1 << 20) + 4)), dict(y=ctypes.c_void_p((1 << 21) + 4))):
        assert mix(**bad) == INV, bad
        assert b"jat_rate_mix" in built.jat_last_error()


# ---- the twins on tracks worked by hand ----------------------------------------------------------------------------------------
def test_classes_by_hand():
    # ratio = 2^(50/1200) = 1.0293: 100 ~ 101 ~ 102; 200 ~ 205 (205.86), 205 ~ 210 (211.01), 200 !~ 210
    f0 = np.array([[100, 101, 102, 0, 200, 205, 210, np.nan]], F32)
    cls, count, summary = RR.f0_classes(f0, np.ones((1, 8), np.uint8), W=1, min_count=3)
    assert count.tolist() == [[2, 3, 2, 0, 2, 3, 2, 0]]                  # a flag on f0 = 0 or NaN is not live
    assert cls.tolist() == [[1, 2, 1, 0, 1, 2, 1, 0]] and summary.tolist() == [[6, 2]]
    cls, count, _ = RR.f0_classes(f0, np.ones((1, 8), np.uint8), W=2, min_count=3)
    assert count.tolist() == [[3, 3, 3, 0, 2, 3, 2, 0]]                  # 200 and 210 are 84 cents apart
    assert cls.tolist() == [[2, 2, 2, 0, 1, 2, 1, 0]]
    # a frame without its flag, +inf, a negative value: none is live, none is counted by a neighbour
    f0 = np.array([[100, 100, np.inf, 100, -100, 100]], F32)
    cls, count, summary = RR.f0_classes(f0, np.array([[1, 0, 1, 1, 1, 1]]), W=1, min_count=1)
    assert count.tolist() == [[1, 0, 0, 1, 0, 1]] and cls.tolist() == [[2, 0, 0, 2, 0, 2]] and summary.tolist() == [[3, 3]]
    # W = 0: every live frame counts itself
    cls, count, _ = RR.f0_classes(f0, np.ones((1, 6)), W=0, min_count=1)
    assert count.tolist() == [[1, 1, 0, 1, 0, 1]] and cls.tolist() == [[2, 2, 0, 2, 0, 2]]
    assert RR.default_min_count(4) == RT.default_min_count(4) == 7 and RT.default_min_count(0) == 1
    assert [RT.default_min_count(w) <= 2 * w + 1 for w in range(33)] == [True] * 33


def test_the_ratio_boundary_counts_as_agreeing():
    ratio = RR.cents_ratio(50.0)
    assert float(ratio) == RT.cents_ratio(50.0) == 1.0293022394180298
    edge = F32(F32(100) * ratio)                                          # exactly f0[t] * ratio
    _, count, _ = RR.f0_classes(np.array([[100, edge]], F32), np.ones((1, 2)), W=1, ratio=ratio, min_count=2)
    assert count.tolist() == [[2, 2]]
    above = np.nextafter(edge, F32(np.inf))
    _, count, _ = RR.f0_classes(np.array([[100, above]], F32), np.ones((1, 2)), W=1, ratio=ratio, min_count=2)
    assert count.tolist() == [[1, 1]]
    # a product that rounds to +inf: every finite f0 lies below it, the other direction decides
    big = F32(3.3e38)
    _, count, _ = RR.f0_classes(np.array([[big, big, 100]], F32), np.ones((1, 3)), W=2, ratio=ratio, min_count=2)
    assert count.tolist() == [[2, 2, 1]]


def test_rate_track_by_hand():
    cls = np.array([[0, 0, 2, 2, 2, 1]], np.uint8)
    # c = 0 0 1 1 1 .5 | 0 0: the two frames behind the pitch track are unvoiced
    assert RR.rate_track(cls, 8, [0, 0.5, 1], 0).tolist() == [[0, 0, 1, 1, 1, 0.5, 0, 0]]
    got = RR.rate_track(cls, 8, [0, 0.5, 1], 1)
    want = [0.0, 0.3333333432674408, 0.6666666269302368, 1.0, 0.8333333134651184, 0.5, 0.1666666716337204, 0.0]
    assert got.tolist() == [want]
    assert RR.rate_track(cls, 3, [0.25, 0.5, 1], 0).tolist() == [[0.25, 0.25, 1]]           # T < F
    assert RR.rate_track(np.array([[7, 1, 200]], np.uint8), 3, [0.25, 0.5, 1], 0).tolist() == [[1, 0.5, 1]]   # above 2: 2
    assert RR.rate_table(0.4, 0.33, 0.7).tolist() == [F32(0.4 * 0.33), F32(0.4 * 0.7), F32(0.4)]
    assert RT.rate_table(0.4, 0.33, 0.7) == tuple(float(v) for v in RR.rate_table(0.4, 0.33, 0.7))
    assert RT.rate_table(0.4) == (float(F32(0.4)),) * 3                   # protect = unstable = 1: one rate


def test_difference_form_smoothing():
    rng = np.random.default_rng(5)
    for table in ([0.13, 0.29, 0.41], [F32(0.4 * 0.33), F32(0.4 * 0.7), F32(0.4)], [0, 1, 1], [1 / 3, 1 / 3, 1 / 3]):
        table = np.asarray(table, F32)
        for S in (0, 2, 16):
            cls = np.repeat(rng.integers(0, 3, size=(2, 6)), 40, axis=1).astype(np.uint8)      # stretches of 40 frames
            T = cls.shape[1] + 25
            r = RR.rate_track(cls, T, table, S)
            c = np.concatenate([table[cls], np.full((2, 25), table[0], F32)], axis=1)
            assert ((r >= 0) & (r <= 1)).all()
            for b in range(2):
                change = np.flatnonzero(c[b, 1:] != c[b, :-1])                                  # a change between t and t + 1
                t = np.arange(T)
                far = np.ones(T, bool) if len(change) == 0 else \
                    (np.abs(t[:, None] - change[None, :] - 0.5).min(axis=1) > S)
                assert far.sum() > 0 and (r[b, far].view(np.uint32) == c[b, far].view(np.uint32)).all(), (table, S)
            if S == 0:
                assert (r.view(np.uint32) == c.view(np.uint32)).all()
    # a constant class row: one value, whatever the window
    third = np.asarray([1 / 3] * 3, F32)
    r = RR.rate_track(np.full((1, 50), 1, np.uint8), 50, third, 16)
    assert (r == third[0]).all()


# ---- the command line ------------------------------------------------------------------------------------------------------------
def test_parser_flags():
    from jatsr_amd.infer import build_parser, rate_flags
    p = build_parser()
    a = p.parse_args([])
    assert a.index_protect is None and a.index_unstable is None and a.index_smooth is None and a.index_f0_method is None
    assert not rate_flags(a)
    from jatsr_amd import pitch
    methods = next(act for act in p._actions if act.dest == "index_f0_method").choices
    assert len(methods) == 2 and methods[0] == "yin" and all(callable(getattr(pitch, m)) for m in methods)   # both trackers
    a = p.parse_args(["--index-protect", "0.33", "--index-unstable", "0.7", "--index-smooth", "3", "--index-f0-method", methods[1]])
    assert (a.index_protect, a.index_unstable, a.index_smooth, a.index_f0_method) == (0.33, 0.7, 3, methods[1]) and rate_flags(a)
    for flag in ("--index-protect", "--index-unstable", "--index-smooth"):
        assert rate_flags(p.parse_args([flag, "1"]))                      # any of the three makes the rate a track
    for bad in (["--index-protect", "1.5"], ["--index-protect", "-0.1"], ["--index-protect", "nan"], ["--index-unstable", "2"],
                ["--index-unstable", "x"], ["--index-smooth", "17"], ["--index-smooth", "-1"], ["--index-smooth", "1.5"],
                ["--index-f0-method", "crepe"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    text = p.format_help()
    assert "plain factor" in text and "0.33" in text                     # ours is not RVC's slider


def test_infer_refuses_before_any_device_work(tmp_path):
    from jatsr_amd.infer import build_parser, run
    p = build_parser()
    with pytest.raises(SystemExit, match="need --index-bank"):
        run(p.parse_args(["--index-protect", "0.5"]))
    with pytest.raises(SystemExit, match="need --index-bank"):
        run(p.parse_args(["--index-f0-method", "yin"]))
    with pytest.raises(SystemExit, match="--index-f0-method needs"):
        run(p.parse_args(["--index-bank", "b.pt", "--index-f0-method", "yin"]))
    with pytest.raises(SystemExit, match="pitch of the LR audio"):
        run(p.parse_args(["--index-bank", "b.pt", "--index-smooth", "2"]))


def test_python_checks_need_no_gpu():
    for bad in (-1, 33, 4.0, True, None):
        with pytest.raises(ValueError, match="half_window"):
            RT.check_half_window(bad)
    for bad in (-1, 17, 2.0, True):
        with pytest.raises(ValueError, match="smooth"):
            RT.check_smooth(bad)
    for bad in (-0.1, 1.1, float("nan")):
        with pytest.raises(ValueError, match="protect"):
            RT.rate_table(0.4, protect=bad)
        with pytest.raises(ValueError, match="unstable"):
            RT.rate_table(0.4, unstable=bad)
        with pytest.raises(ValueError, match="index_rate"):
            RT.rate_table(bad)
    for bad in (0.0, -50.0, 1e-6, 1e9, float("nan")):
        with pytest.raises(ValueError, match="cents"):
            RT.cents_ratio(bad)
    # a track on the wrong device, of the wrong dtype, shape or range (CPU tensors: nothing is launched)
    dev = torch.device("cpu")
    good = torch.full((2, 5), 0.5)
    assert RT.check_rates(good, 2, 5, dev).shape == (2, 5) and RT.check_rates(good[0], 1, 5, dev).shape == (1, 5)
    for bad, what in ((good.double(), "dtype"), (good[:, :4], "shape"), (good[0], "shape"), (good + 0.6, "outside"),
                      (good - 0.6, "outside"), (good * float("nan"), "outside"), ([0.5] * 5, "expected a tensor")):
        with pytest.raises(ValueError, match=what):
            RT.check_rates(bad, 2, 5, dev)
    with pytest.raises(ValueError, match="expected cuda"):
        RT.check_rates(good, 2, 5, "cuda:0")
    assert RT.is_rate_track(good) and not RT.is_rate_track(0.4) and not RT.is_rate_track(torch.tensor(0.4))
    from jatsr_amd.sampler import sample_long
    lr = torch.zeros(4, 10)
    with pytest.raises(ValueError, match="needs a bank"):
        sample_long(None, lr, None, None, None, None, index_rates=torch.zeros(10))
    with pytest.raises(ValueError, match="10 frames"):
        sample_long(None, lr, None, None, None, None, bank=types.SimpleNamespace(), index_rates=torch.zeros(9))


# ---- the fixture in fp64 -----------------------------------------------------------------------------------------------------------
def test_fixture_in_fp64():
    """0.4 s each of a 220 Hz tone, white noise and a glide 200 -> 400 Hz: the frames at least W + 2 = 6 frames inside a segment
    are stable, not live and unstable.  The frames nearer a boundary (or an end of the file) are left out: 36 of 104, 34.6 %."""
    x = RR.fixture_signal()
    y = P.yin(x, sr=RR.SR, hop_length=RR.HOP, dtype=np.float64)
    f0, voiced = y["f0"].astype(F32)[None], y["voiced"][None]
    F = RR.fixture_frames()
    assert f0.shape == (1, F) and F == 104
    seg = RR.fixture_inner()
    left_out = int((seg < 0).sum())
    print(f"fixture: {left_out} of {F} frames left out ({left_out / F:.3f}); inner frames per segment "
          f"{[int((seg == s).sum()) for s in range(3)]}")
    assert left_out == 36 and all((seg == s).sum() >= 20 for s in range(3))
    W = RR.FIXTURE_W
    want = np.array(RR.FIXTURE_CLASSES)[seg[seg >= 0]]
    counts = {}
    for cents in (40.0, 50.0, 60.0):                                      # no inner frame hangs on the limit
        cls, count, summary = RR.f0_classes(f0, voiced, W=W, ratio=RR.cents_ratio(cents))
        assert (cls[0, seg >= 0] == want).all(), cents
        counts[cents] = count[0]
    c = counts[50.0]
    assert (c[seg == 0] == 2 * W + 1).all() and (c[seg == 1] == 0).all()
    assert (counts[40.0][seg == 2] == 3).all() and (counts[60.0][seg == 2] == 3).all()       # far from min_count = 7
    tone = f0[0, seg == 0]
    assert np.abs(P.cents(tone, 220.0)).max() < 1.0
    glide = f0[0, seg == 2].astype(np.float64)
    step = 1200.0 * np.log2(glide[1:] / glide[:-1])
    assert (np.abs(step - 1200.0 * RR.HOP / RR.SEG) < 3.0).all()          # 34.8 cents a frame: 15 inside, 20 outside the limit
