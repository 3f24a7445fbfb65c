"""The pYIN statement (tests/pyin_ref.py) and the host side of the library (csrc/jat_pyin.cpp), without a GPU: the fp32
statement decodes what the fp64 one does on every signal the GPU tests use (the condition under which their 1 % cap hides
nothing), the host tables agree with the fp64 formulas, every refusal of the host functions, the exported symbols, and the
property the tracker is there for: on the octave signal plain YIN drops to half the period and pYIN does not."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pitch_ref as P  # noqa: E402
import pyin_ref as Y  # noqa: E402
import jatsr_amd._lib as L  # noqa: E402
import jatsr_amd.pitch as pitch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(P.CASES) + ["octave"]


@pytest.fixture(scope="module")
def built_lib():
    if not os.path.exists(L.LIB_PATH):
        sys.path.insert(0, ROOT)
        import __graft_entry__ as g
        g.build()
    return L.lib()


@pytest.mark.parametrize("name", NAMES)
def test_fp32_statement_decodes_as_the_fp64_statement(name):
    x, r64, r32 = Y.case(name)
    T = Y.case_tables(name)
    for b, (a, s) in enumerate(zip(r64, r32)):
        frames = a["state"].shape[0]
        raw = int((a["state"] != s["state"]).sum())
        print(f"{name}[{b}]: {frames} frames, {int(a['voiced'].sum())} voiced, (voiced, bin) differs on {Y.same_track(a, s)}, "
              f"raw state on {raw}; n_bins {T['n_bins']}, H {T['H']}, at most {int((a['bin'] >= 0).sum(axis=1).max())} troughs")
        assert frames == 1 + x.shape[1] // T["hop_length"]
        assert Y.same_track(a, s) == 0
        assert (np.abs(a["voiced_prob"] - s["voiced_prob"]) <= 1e-4).all()


def test_case_shapes_reach_the_sizes_the_issue_names():
    shapes = {n: (Y.case_tables(n)["n_bins"], Y.case_tables(n)["H"]) for n in NAMES}
    assert shapes["defaults"] == (519, 50) and shapes["short"][0] == 665 and shapes["sr16k"][1] == 70
    assert shapes["frame4096"] == (639, 90) and shapes["octave"] == (519, 50)
    assert int((Y.case("frame4096")[1][0]["bin"] >= 0).sum(axis=1).max()) == 535
    x, r64, _ = Y.case("defaults")
    T = Y.case_tables("defaults")
    collisions = 0
    for f in range(r64[0]["bin"].shape[0]):
        b = r64[0]["bin"][f]
        b = b[b >= 0]
        collisions += len(b) - len(np.unique(b))
    print("collisions on defaults[0]:", collisions)
    assert collisions > 100                                             # the largest-lag-wins rule is exercised


def test_octave_property_of_the_fp64_statement():
    x, r64, _ = Y.case("octave")
    inner = slice(3, -3)
    y = P.yin(x[0])
    off_yin = np.abs(P.cents(y["f0"], 220.0))[inner]
    a = r64[0]
    off = np.abs(P.cents(np.where(a["voiced"], a["f0"], 1.0), 220.0))[inner]
    print(f"{off_yin.shape[0]} inner frames: yin > 600 cents on {int((off_yin > 600).sum())}; pyin voiced on "
          f"{int(a['voiced'][inner].sum())}, worst {off.max():.4f} cents")
    assert off_yin.shape[0] == 38 and (off_yin > 600).sum() >= 3
    # half a bin is 5 cents; 220 Hz lies at bin position 256.5004 above 50 Hz, so either neighbouring bin centre is 5.00
    # cents from it to the precision the figure is stated in
    assert a["voiced"][inner].all() and (off <= 600).all() and (off < 5.05).all()
    assert set(np.unique(a["track_bin"][inner])) <= {256, 257}


def _beta(a, b, n):
    out = np.zeros(n, np.float64)
    rc = L.lib().jat_pyin_beta_probs(a, b, n, C.c_void_p(out.ctypes.data))
    return rc, out


def test_beta_probs_against_the_fp64_formulas(built_lib):
    for a, b, n in ((2.0, 18.0, 100), (2.0, 18.0, 1), (1.0, 1.0, 7), (2.5, 7.25, 50), (0.5, 0.5, 64), (9.0, 2.0, 256)):
        rc, got = _beta(a, b, n)
        want = Y.beta_probs(a, b, n)
        print(f"Beta({a}, {b}), {n}: max |diff| {np.abs(got - want).max():.2e}, sum - 1 = {got.sum() - 1:.2e}")
        assert rc == 0 and np.abs(got - want).max() <= 1e-13 and abs(got.sum() - 1.0) <= 1e-14 and (got >= 0).all()
        try:
            from scipy import stats
        except ImportError:
            continue
        assert np.abs(got - np.diff(stats.beta.cdf(np.arange(n + 1) / n, a, b))).max() <= 1e-13
    for bad in ((0.0, 1.0, 10), (-1.0, 1.0, 10), (1.0, float("nan"), 10), (float("inf"), 1.0, 10), (2.0, 18.0, 0), (2.0, 18.0, 65537)):
        assert _beta(*bad)[0] == L.JAT_E_INVALID and L.lib().jat_last_error(), bad
    assert L.lib().jat_pyin_beta_probs(2.0, 18.0, 10, None) == L.JAT_E_INVALID


@pytest.mark.parametrize("name", ["defaults", "short", "sr16k", "frame4096"])
def test_tables_against_the_fp64_formulas(built_lib, name):
    T = Y.case_tables(name)
    h = pitch.pyin_handle(**Y.params(name))
    t = h.tables()
    assert (h.n_bins, h.H, h.min_period, h.max_period) == (T["n_bins"], T["H"], T["lo"], T["hi"])
    assert np.abs(t["beta"] - T["beta"]).max() <= 1e-13 and abs(t["beta"].sum() - 1) <= 1e-14
    u = 2.0 ** -24
    for k in ("logw", "logZ"):
        assert t[k].dtype == np.float32 and (np.abs(t[k] - T[k]) <= u * np.abs(T[k]) + 1e-12).all(), k   # fp64, rounded once
    assert (np.abs(t["freqs"].astype(np.float64) / T["freqs"] - 1) <= 2 * u).all()
    assert t["lk"] == np.float32(T["lk"]) and t["ls"] == np.float32(T["ls"]) and t["logpi"] == np.float32(T["logpi"])
    assert t["logw"][T["H"]] == 0 and len(t["logw"]) == 2 * T["H"] + 1
    try:
        from scipy import stats
    except ImportError:
        return
    lam, n = 2.0, 7
    pmf = stats.boltzmann.pmf(np.arange(n), lam, n)
    assert np.abs(T["A"][:n] * T["invD"][n] - pmf).max() <= 1e-15 and abs(pmf.sum() - 1) <= 1e-12


def test_refusals_of_the_host_functions(built_lib):
    base = dict(fmin=50.0, fmax=1000.0, sr=44100, frame_length=2048, hop_length=512, n_thresholds=100, beta_a=2.0, beta_b=18.0,
                boltzmann_parameter=2.0, resolution=0.1, max_transition_rate=35.92, switch_prob=0.01, no_trough_prob=0.01)

    def create(**over):
        v = dict(base, **over)
        h = C.c_void_p()
        rc = L.lib().jat_pyin_create(C.byref(L.JatPyinParams(*[v[n] for n, _ in L.JatPyinParams._fields_])), C.byref(h))
        return rc, h

    rc, h = create()
    assert rc == 0 and h
    nan, inf = float("nan"), float("inf")
    bad = [dict(frame_length=2047), dict(frame_length=14), dict(frame_length=8194), dict(hop_length=0), dict(hop_length=-3),
           dict(fmin=0.0), dict(fmin=nan), dict(fmax=50.0), dict(fmax=22050.0), dict(sr=0), dict(fmin=20000.0, fmax=22000.0),
           dict(n_thresholds=0), dict(n_thresholds=-1), dict(n_thresholds=257), dict(beta_a=0.0), dict(beta_a=-2.0), dict(beta_b=nan),
           dict(beta_b=inf), dict(boltzmann_parameter=0.0), dict(boltzmann_parameter=nan), dict(boltzmann_parameter=-1.0),
           dict(max_transition_rate=nan), dict(max_transition_rate=-1.0), dict(max_transition_rate=inf),
           dict(switch_prob=0.0), dict(switch_prob=1.0), dict(switch_prob=nan), dict(switch_prob=-0.1),
           dict(no_trough_prob=0.0), dict(no_trough_prob=1.0), dict(no_trough_prob=nan), dict(no_trough_prob=1.5),
           dict(resolution=0.0), dict(resolution=1.5), dict(resolution=nan), dict(resolution=-0.1),
           dict(resolution=0.05),                       # 1038 bins: beyond the 1024 the kernels take
           dict(resolution=1e-9),
           dict(max_transition_rate=100.0),             # H = 140: beyond 128
           dict(hop_length=4096)]                       # H = 400
    for over in bad:
        rc2, h2 = create(**over)
        assert rc2 == L.JAT_E_INVALID and not h2 and L.lib().jat_last_error(), over
    assert L.lib().jat_pyin_create(None, C.byref(C.c_void_p())) == L.JAT_E_INVALID
    assert create(n_thresholds=256)[0] == 0 and create(n_thresholds=1)[0] == 0 and create(resolution=1.0)[0] == 0
    sz = C.c_size_t(7)
    ok = L.lib().jat_pyin_workspace_bytes(h, 2, 44100, C.byref(sz))
    assert ok == 0 and sz.value > 2 * 87 * (883 * 4 + 520 * 4 + 2 * 519 * 2)
    for B, n in ((0, 100), (-1, 100), (65536, 100), (1, 0), (1, -5), (1, 2 ** 40)):
        sz = C.c_size_t(7)
        assert L.lib().jat_pyin_workspace_bytes(h, B, n, C.byref(sz)) == L.JAT_E_INVALID and sz.value == 7, (B, n)
    assert L.lib().jat_pyin_workspace_bytes(None, 1, 100, C.byref(sz)) == L.JAT_E_INVALID
    assert L.lib().jat_pyin_workspace_bytes(h, 1, 100, None) == L.JAT_E_INVALID
    assert L.lib().jat_pyin_shape(None, None, None, None, None) == L.JAT_E_INVALID
    assert L.lib().jat_pyin_tables(None, None, None, None, None, None) == L.JAT_E_INVALID
    assert L.lib().jat_pyin_track(None, None, 1, 100, None, None, None, None, None, None, None, None, None, None, 0, None) == L.JAT_E_INVALID
    assert L.lib().jat_pyin_track(h, None, 1, 100, None, None, None, None, None, None, None, None, None, None, 0, None) == L.JAT_E_INVALID
    assert L.lib().jat_pyin_profile(h, None) == L.JAT_E_INVALID
    us = (C.c_float * 4)()
    assert L.lib().jat_pyin_profile(h, us) == L.JAT_E_STATE
    L.lib().jat_pyin_destroy(h)
    L.lib().jat_pyin_destroy(None)
    # the Python layer
    with pytest.raises(ValueError, match="n_thresholds"):
        pitch.pyin_handle(n_thresholds=300)
    with pytest.raises(ValueError, match="integer"):
        pitch.pyin_handle(n_thresholds=10.5)
    assert pitch.pyin_handle() is pitch.pyin_handle(beta_parameters=(2, 18))


def test_symbols_declared_bound_and_exported_from_both_libraries(built_lib):
    names = ["jat_pyin_beta_probs", "jat_pyin_create", "jat_pyin_destroy", "jat_pyin_shape", "jat_pyin_tables",
             "jat_pyin_workspace_bytes", "jat_pyin_track", "jat_pyin_decode", "jat_pyin_set_profile", "jat_pyin_profile"]
    header = open(os.path.join(ROOT, "include", "jat_hip.h")).read()
    declared = set(re.findall(r"\b(jat_[a-z0-9_]+)\s*\(", header))
    csrc = os.path.dirname(L.LIB_PATH)
    for lib in ("libjat_hip.so", "libjat_hip_fp16.so"):
        nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(csrc, lib)], capture_output=True, text=True, check=True).stdout
        exported = set(re.findall(r" T (jat_[a-z0-9_]+)", nm))
        for n in names:
            assert n in declared and n in L.SIGNATURES and n in exported, (lib, n)
    assert sorted(n for n in L.SIGNATURES if n.startswith("jat_pyin")) == sorted(names)


def test_no_existing_test_calls_the_new_symbols():
    # test_gpu_streams.py came later and runs every stream-taking entry of the header on a side stream, these two included
    mine = {"test_pyin_cpu.py", "test_pyin_gpu.py", "pyin_ref.py", "test_gpu_streams.py"}
    for name in sorted(os.listdir(os.path.join(ROOT, "tests"))):
        if name.endswith(".py") and name not in mine:
            assert "pyin" not in open(os.path.join(ROOT, "tests", name)).read(), name
