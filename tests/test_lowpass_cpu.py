"""The host side of the IIR low-pass families (jatsr_amd/lowpass.py) and the numpy twins of tests/lowpass_ref.py,
without a GPU: the designs against scipy's, the fp64 twin against scipy's sosfilt / sosfiltfilt, the blocked fp32 twin against
the sequential ones, the per-recording draw, and every refusal of the module and of the prepare / infer command lines."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lowpass_ref as R  # noqa: E402
from jatsr_amd import lowpass as LP  # noqa: E402
from jatsr_amd._lib import JatError  # noqa: E402

SR = 48000
CUTOFFS = (SR / 48.0, 2500.0, 8000.0, 16000.0, 0.49 * SR)
# |H| (512 frequencies, wherever |H| > 1e-8) and zi of design_sos against scipy, relative: fp64 round-off of the design.  The
# largest figures measured over DESIGN_CASES were 2.25e-12 (|H|; the worst points lie deep in the stop band, where the sections'
# numerators nearly cancel) and 7.4e-15 (zi against sosfilt_zi of the same sections); the gates are twice those
H_TOL, ZI_TOL = 4.5e-12, 1.5e-14
DESIGN_CASES = [(kind, order, cut, rp) for kind in LP.KINDS for order in range(1, 11) for cut in CUTOFFS
                for rp in ((1.0,) if kind == "butter" else (0.1, 1.0, 3.0))]


def scipy_sos(ss, kind, order, cut, rp):
    return ss.butter(order, cut, fs=SR, output="sos") if kind == "butter" else ss.cheby1(order, rp, cut, fs=SR, output="sos")


def test_design_matches_scipy():
    ss = pytest.importorskip("scipy.signal")
    worst_h = worst_zi = 0.0
    for kind, order, cut, rp in DESIGN_CASES:
        sos, ref = LP.design_sos(kind, order, cut, SR, rp), scipy_sos(ss, kind, order, cut, rp)
        assert sos.shape == ref.shape == (math.ceil(order / 2), 6) and sos.dtype == np.float64
        _, h = ss.sosfreqz(sos, 512)
        _, g = ss.sosfreqz(ref, 512)
        keep = np.abs(g) > 1e-8
        worst_h = max(worst_h, float(np.max(np.abs(np.abs(h[keep]) - np.abs(g[keep])) / np.abs(g[keep]))))
        zi, want = LP.sos_zi(sos), ss.sosfilt_zi(sos)
        worst_zi = max(worst_zi, float(np.abs(zi - want).max() / np.abs(want).max()))
        # the step steady state does not depend on how the sections pair up: the last section's state against scipy's own design
        assert abs(LP.dc_gain(sos) - LP.dc_gain(ref)) <= 1e-12 * abs(LP.dc_gain(ref))
    print(f"design against scipy: |H| {worst_h:.2e} (gate {H_TOL:.1e}), zi {worst_zi:.2e} (gate {ZI_TOL:.1e})")
    assert worst_h <= H_TOL and worst_zi <= ZI_TOL


def test_design_layout_and_gain():
    for kind, order, cut, rp in DESIGN_CASES:
        sos = LP.design_sos(kind, order, cut, SR, rp)
        assert (sos[:, 3] == 1.0).all()
        first = [k for k in range(len(sos)) if sos[k, 2] == 0.0 and sos[k, 5] == 0.0]
        assert len(first) == order % 2                                   # one first-order section for an odd order
        radius = [math.sqrt(s[5]) if s[5] else abs(s[4]) for s in sos]
        assert radius == sorted(radius) and radius[-1] < 1.0             # the pair nearest the unit circle comes last
        dc = LP.dc_gain(sos)
        want = 1.0 if kind == "butter" or order % 2 else 10.0 ** (-rp / 20.0)   # Chebyshev: passband maximum 1
        assert abs(dc - want) < 1e-9
        w = np.exp(-1j * np.pi * np.linspace(0, 1, 2049))
        H = np.prod([(s[0] + s[1] * w + s[2] * w * w) / (1 + s[4] * w + s[5] * w * w) for s in sos], axis=0)
        assert np.abs(H).max() <= 1.0 + 1e-9
        p5 = LP.pad_sos(sos)
        assert p5.shape == (5, 6) and LP.own_sections(p5) == len(sos) and (p5[len(sos):] == [1, 0, 0, 1, 0, 0]).all()
        assert LP.padlen(p5) == 3 * (2 * len(sos) + 1 - order % 2)
    assert LP.padlen(LP.pad_sos(LP.design_sos("butter", 10, 1000.0, SR))) == 33
    assert LP.padlen(LP.pad_sos(np.zeros((0, 6)))) == 3


def test_transition_matrix_is_the_zero_input_recurrence():
    rows = R.Rows(R.filter_list())
    for r in range(rows.K):
        A = LP.transition_matrix(rows.sos[r])
        s0 = np.random.default_rng(r).standard_normal(R.STATE)
        s0[2 * rows.nsec[r]:] = 0.0
        one = R.Rows([rows.sos[r][:rows.nsec[r]]])
        s = [s0[c:c + 1].copy() for c in range(R.STATE)]
        R._step(R._split(one.coef(np.float64), one.nsec), s, np.zeros(1))
        assert np.allclose(A @ s0, np.concatenate(s), rtol=0, atol=1e-15 * np.abs(s0).max())
        P = LP.transition_powers(rows.sos[r])
        assert P.shape == (9, 10, 10)
        assert np.allclose(P[0], np.linalg.matrix_power(A, 32), rtol=1e-9, atol=1e-300)
        assert np.allclose(P[8], np.linalg.matrix_power(P[0], 256), rtol=1e-6, atol=1e-300)


# ---- the twins ------------------------------------------------------------------------------------------------------------------------
N_TWIN = 6000


@pytest.fixture(scope="module")
def twins():
    filters = R.filter_list()
    rows = R.Rows(filters)
    x = np.stack([R.noise(N_TWIN, i) for i in range(rows.K)])
    out = {"filters": filters, "rows": rows, "x": x}
    for name, fn in (("filt", R.sosfilt), ("filtfilt", R.sosfiltfilt)):
        out[name] = {"f64": fn(x, rows, use_scipy=False), "f32": fn(x, rows, np.float32), "blocked": fn(x, rows, np.float32, blocked=True)}
    return out


def test_fp64_twin_is_scipy(twins):
    ss = pytest.importorskip("scipy.signal")
    eps32, eps64 = 2.0 ** -24, 2.0 ** -53
    for r, name in enumerate(R.FILTERS):
        x64 = twins["x"][r].astype(np.float64)
        assert np.array_equal(twins["filt"]["f64"][r], ss.sosfilt(twins["filters"][r], x64)), name    # the same loop: error 0
        # sosfiltfilt: fp64 round-off only.  The recurrence amplifies a rounding by the same factor in either precision, and the
        # sequential fp32 twin shows that factor (its error over eps32); twice that many eps64 is the gate
        gate = max(2.0 * R.rel_max(twins["filtfilt"]["f32"][r], twins["filtfilt"]["f64"][r]) / eps32 * eps64, 4 * eps64)
        got = R.rel_max(twins["filtfilt"]["f64"][r], ss.sosfiltfilt(twins["filters"][r], x64))
        print(f"{name}: fp64 twin against scipy.sosfiltfilt {got:.2e} (gate {gate:.2e})")
        assert got <= gate, name


def test_blocked_twin_against_the_sequential_twins(twins):
    """the measurement behind the GPU gate: per filter, rel-L2 of both fp32 twins against fp64 on 6000 white-noise samples.
    Blocking must not cost accuracy: within a block the arithmetic is the sequential one's and the carried states are rounded
    once per scan step, so the blocked error stays within 4 times the sequential one (plus one fp32 rounding of the output)."""
    for which in ("filt", "filtfilt"):
        for r, name in enumerate(R.FILTERS):
            seq = R.rel_l2(twins[which]["f32"][r], twins[which]["f64"][r])
            blk = R.rel_l2(twins[which]["blocked"][r], twins[which]["f64"][r])
            print(f"{which:8s} {name:16s} sequential fp32 {seq:.2e}  blocked fp32 {blk:.2e}")
            assert blk <= 4.0 * seq + 2.0 ** -24, (which, name)
            assert seq < 3e-4                                             # the cutoff floor of design_sos keeps fp32 usable


def test_blocked_twin_carries_across_blocks_and_tiles():
    """unit impulses on both sides of a lane-block boundary and of a tile boundary, and a step: the blocked twin against the
    sequential fp32 twin, whose only difference is the rounding of the carried states"""
    rows = R.Rows(R.filter_list())
    n = R.TILE + 700
    x = np.zeros((rows.K, n), np.float32)
    x[0, R.LANE_BLOCK - 1] = x[1, R.LANE_BLOCK] = x[2, R.TILE - 1] = x[3, R.TILE] = 1.0
    x[4] = 1.0
    seq, blk, ref = (R.sosfilt(x, rows, np.float32), R.sosfilt(x, rows, np.float32, blocked=True), R.sosfilt(x, rows))
    for r in range(rows.K):
        gate = 2.0 * max(R.rel_max(seq[r], ref[r]), 2.0 ** -24)
        assert R.rel_max(blk[r], ref[r]) <= 2.0 * gate, r
        at = int(np.argmax(x[r] != 0))
        assert (blk[r][:at] == 0).all() and blk[r][at] != 0               # nothing in front of the impulse, something on it
    assert abs(blk[4][-1] - 1.0) < 1e-5                                   # the step settles to the DC gain


def test_identity_cascade_returns_the_input():
    rows = R.Rows([np.zeros((0, 6))])
    x = R.noise(R.TILE + 5)[None].copy()
    x[0, 3] = -0.0
    for fn in (R.sosfilt, R.sosfiltfilt):
        assert fn(x, rows, np.float32, blocked=True).tobytes() == x.tobytes()
    assert rows.padlen[0] == 3 and (rows.zi == 0).all()


# ---- the draw and the refusals ------------------------------------------------------------------------------------------------------------
def test_random_filter_is_a_function_of_seed_and_name():
    a = LP.random_filter(7, "song_001")
    np.random.seed(3)
    import random
    random.seed(9)
    assert LP.random_filter(7, "song_001") == a
    assert a["kind"] in LP.KINDS and 2 <= a["order"] <= 10 and 2000.0 <= a["cutoff_hz"] <= 12000.0 and a["ripple_db"] == 1.0
    names = [f"song_{i:03d}" for i in range(400)]
    draws = [LP.random_filter(7, n, ("sinc", "butter", "cheby1"), (1000.0, 16000.0), (3, 6)) for n in names]
    assert draws != [LP.random_filter(8, n, ("sinc", "butter", "cheby1"), (1000.0, 16000.0), (3, 6)) for n in names]
    kinds = [d["kind"] for d in draws]
    assert all(kinds.count(k) > 90 for k in ("sinc", "butter", "cheby1"))
    iir = [d for d in draws if d["kind"] != "sinc"]
    assert {d["order"] for d in iir} == {3, 4, 5, 6} and all(1000.0 <= d["cutoff_hz"] <= 16000.0 for d in iir)
    logs = np.log([d["cutoff_hz"] for d in iir])                         # log-uniform: the median sits at the geometric mean
    assert abs(np.median(logs) - 0.5 * (math.log(1000.0) + math.log(16000.0))) < 0.25
    assert all(set(d) == {"kind"} for d in draws if d["kind"] == "sinc")
    one = LP.random_filter(1, "x", ("cheby1",), (4000.0, 4000.0), (8, 8), 0.5)
    assert one == {"kind": "cheby1", "order": 8, "cutoff_hz": 4000.0, "ripple_db": 0.5}


def test_design_refusals_name_the_limit():
    for kw, what in ((dict(order=0), "1..10"), (dict(order=11), "1..10"), (dict(order=2.5), "1..10"),
                     (dict(cutoff_hz=999.0), "sr / 48"), (dict(cutoff_hz=0.491 * SR), "0.49 sr"), (dict(cutoff_hz=float("nan")), "sr / 48"),
                     (dict(kind="cheby1", ripple_db=0.0), r"\(0, 3\]"), (dict(kind="cheby1", ripple_db=3.01), r"\(0, 3\]"),
                     (dict(kind="ellip"), "kind")):
        args = dict(dict(kind="butter", order=4, cutoff_hz=4000.0, sr=SR), **kw)
        with pytest.raises(JatError, match=what):
            LP.design_sos(**args)
    for kw in (dict(kinds=("bessel",)), dict(kinds=()), dict(order=(0, 4)), dict(order=(4, 11)), dict(order=(6, 4)),
               dict(cutoff_hz=(0.0, 100.0)), dict(cutoff_hz=(5000.0, 4000.0))):
        with pytest.raises(JatError):
            LP.random_filter(1, "x", **kw)
    with pytest.raises(JatError, match="S <= 5"):
        LP.pad_sos(np.zeros((6, 6)))
    with pytest.raises(JatError, match="a0 = 1"):
        LP.pad_sos(np.array([[1.0, 0, 0, 2.0, 0, 0]]))


PREPARE = ["--source-dir", "a", "--output-dir", "b", "--dac-weights", "c"]


def test_prepare_flags():
    from jatsr_amd import prepare
    parse = lambda extra: prepare.lr_filter_plan(prepare.build_parser().parse_args(PREPARE + extra))   # noqa: E731
    assert parse([]) is None and parse(["--lr-filter", "sinc"]) is None
    plan = parse(["--lr-filter", "mix", "--lr-cutoff-hz", "2000,8000", "--lr-order", "4,6", "--lr-seed", "5", "--lr-ripple-db", "0.5"])
    assert plan == {"seed": 5, "kinds": ("sinc", "butter", "cheby1"), "cutoff_hz": (2000.0, 8000.0), "order": (4, 6), "ripple_db": 0.5}
    assert parse(["--lr-filter", "butter"])["kinds"] == ("butter",) and parse(["--lr-filter", "cheby1"])["seed"] == 42
    assert parse(["--lr-filter", "cheby1", "--lr-cutoff-hz", "4000"])["cutoff_hz"] == (4000.0, 4000.0)
    for bad in (["--lr-cutoff-hz", "2000,8000"], ["--lr-order", "4,6"], ["--lr-ripple-db", "1"], ["--lr-seed", "1"],
                ["--lr-filter", "sinc", "--lr-order", "4"], ["--lr-filter", "butter", "--lr-ripple-db", "1"],
                ["--lr-filter", "cheby1", "--lr-order", "4,12"], ["--lr-filter", "mix", "--lr-cutoff-hz", "500,8000"],
                ["--lr-filter", "mix", "--lr-cutoff-hz", "8000,2000"], ["--lr-filter", "mix", "--lr-cutoff-hz", "a,b"],
                ["--lr-filter", "cheby1", "--lr-ripple-db", "4"]):
        with pytest.raises(SystemExit):
            parse(bad)
    with pytest.raises(SystemExit):
        prepare.build_parser().parse_args(PREPARE + ["--lr-filter", "ellip"])


def test_infer_flags():
    from jatsr_amd import infer
    parse = lambda extra: infer.lr_filter_of(infer.build_parser().parse_args(extra))   # noqa: E731
    assert parse([]) is None and parse(["--input-audio", "a.wav", "--simulate-lr"]) is None
    got = parse(["--input-audio", "a.wav", "--simulate-lr", "--lr-filter", "butter", "--lr-cutoff-hz", "6000", "--lr-order", "8"])
    assert got == {"kind": "butter", "order": 8, "cutoff_hz": 6000.0, "ripple_db": 1.0}
    got = parse(["--simulate-lr", "--lr-filter", "cheby1", "--lr-cutoff-hz", "4000", "--lr-ripple-db", "0.5"])
    assert got == {"kind": "cheby1", "order": 8, "cutoff_hz": 4000.0, "ripple_db": 0.5}
    for bad in (["--lr-cutoff-hz", "6000"], ["--lr-order", "4"], ["--lr-ripple-db", "1"],
                ["--lr-filter", "butter", "--lr-cutoff-hz", "6000"],                         # without --simulate-lr
                ["--simulate-lr", "--lr-filter", "butter"],                                  # without a cutoff
                ["--simulate-lr", "--lr-filter", "butter", "--lr-cutoff-hz", "6000", "--lr-ripple-db", "1"],
                ["--simulate-lr", "--lr-filter", "butter", "--lr-cutoff-hz", "600"],
                ["--simulate-lr", "--lr-filter", "butter", "--lr-cutoff-hz", "6000", "--lr-order", "11"]):
        with pytest.raises(SystemExit):
            parse(bad)
    with pytest.raises(SystemExit):
        infer.build_parser().parse_args(["--lr-filter", "sinc"])


def test_header_and_bindings_agree():
    import re

    from jatsr_amd import _lib as L
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "jat_hip_iir.h")).read()
    declared = set(re.findall(r"^(?:int|void) (jat_[a-z0-9_]+)\(", header, re.M))
    assert declared == set(L.IIR_SIGNATURES) and len(declared) == 7
    assert int(re.search(r"#define JAT_IIR_SECTIONS (\d+)", header).group(1)) == LP.SECTIONS
    assert int(re.search(r"#define JAT_IIR_POWERS (\d+)", header).group(1)) == LP.POWERS
