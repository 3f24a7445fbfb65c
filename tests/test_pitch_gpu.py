"""The pitch tracker on the GPU (csrc/pitch.hip, jatsr_amd.pitch) against its fp64 statement (tests/pitch_ref.py).

YIN ends in discrete decisions (the first trough under a threshold, an arg-min, a voiced flag), so the continuous and the
discrete stage are gated apart:
  d        |d_gpu - d_64| <= (W + 2) 2^-24 d_64 element-wise: a sum of W non-negative terms, each with three roundings, in
           any order
  cmndf    relative error <= (2 (W + 2) + max_period + 4) 2^-24: the numerator, the running sum of up to max_period such
           terms, the mean and the divide
  discrete the reference's `select` run on the GPU's OWN cmndf (comparisons of fp32 values are exact in fp64) must give the
           GPU's index and voiced flag on every frame, and aperiodicity must be that cmndf entry bit for bit: no tolerance
  fp64     against the fp64 statement end to end, index / voiced may differ on at most 1 % of a case's frames (the CPU test
           shows the fp32 statement differing on none), and on frames whose index matches
           |cents(f0_gpu, f0_64)| <= max(4 x the numpy fp32 statement's maximum on the same input, 0.01 cent)
Every test prints its figures before it asserts.  Measured on MI355X: see DESIGN.md section 20.

The file is named test_pitch_gpu.py, not test_gpu_pitch.py, because tests/fp16_matrix.py needs a row for every
tests/test_gpu_*.py; it carries its own run on the fp16-operand library instead (test_fp16_library_gives_the_same_bits)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pitch_ref as P  # noqa: E402
import jatsr_amd._lib as L  # noqa: E402
import jatsr_amd.io as jio  # noqa: E402
import jatsr_amd.pitch as pitch  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
NAMES = sorted(P.CASES)
_gpu = {}


def cuda(a):
    return torch.from_numpy(np.array(a)).cuda()            # a copy: the shared cases are read-only


def params(name):
    sr, fl, hop, fmin, fmax, n, seeds, thr = P.CASES[name]
    return dict(sr=sr, fmin=fmin, fmax=fmax, frame_length=fl, hop_length=hop, trough_threshold=thr)


def gpu(name):
    """the GPU's outputs for a case, as numpy [B, ...]; computed once"""
    if name not in _gpu:
        x, _, _ = P.case(name)
        r = pitch.yin_full(cuda(x), want=("index", "d", "cmndf"), **params(name))
        _gpu[name] = {k: v.cpu().numpy() for k, v in r.items()}
    return _gpu[name]


@pytest.mark.parametrize("name", NAMES)
def test_d_and_cmndf_within_the_derived_bounds(name):
    sr, fl, hop, fmin, fmax, n, seeds, thr = P.CASES[name]
    W, (lo, hi) = fl // 2, P.periods(sr, fmin, fmax, fl)
    _, r64, r32 = P.case(name)
    g = gpu(name)
    assert g["d"].shape == (len(seeds), 1 + n // hop, hi + 1) and g["d"].dtype == np.float32
    for b, (a, s) in enumerate(zip(r64, r32)):
        d, c = g["d"][b].astype(np.float64), g["cmndf"][b].astype(np.float64)
        assert (d[:, 0] == 0).all() and (c[:, 0] == 1).all()
        err_d = np.abs(d - a["d"])
        err_c = np.abs(c - a["cmndf"])
        rel_d = float((err_d / np.maximum(a["d"], 1e-300)).max())
        rel_c = float((err_c / np.maximum(a["cmndf"], 1e-300)).max())
        y32_d = float((np.abs(s["d"] - a["d"]) / np.maximum(a["d"], 1e-300)).max())
        y32_c = float((np.abs(s["cmndf"] - a["cmndf"]) / np.maximum(a["cmndf"], 1e-300)).max())
        print(f"{name}[{b}]: d rel {rel_d:.2e} (gate {(W + 2) * U:.2e}, numpy fp32 {y32_d:.2e}); cmndf rel {rel_c:.2e} "
              f"(gate {(2 * (W + 2) + hi + 4) * U:.2e}, numpy fp32 {y32_c:.2e})")
        assert (err_d <= (W + 2) * U * a["d"]).all()
        assert (err_c <= (2 * (W + 2) + hi + 4) * U * a["cmndf"]).all()


@pytest.mark.parametrize("name", NAMES)
def test_discrete_stage_is_exact_on_the_gpus_own_cmndf(name):
    sr, fl, hop, fmin, fmax, n, seeds, thr = P.CASES[name]
    lo, hi = P.periods(sr, fmin, fmax, fl)
    g = gpu(name)
    for b in range(len(seeds)):
        c = g["cmndf"][b]
        k, voiced = P.select(c.astype(np.float64), lo, hi, float(np.float32(thr)))
        print(f"{name}[{b}]: {c.shape[0]} frames, {int(voiced.sum())} voiced, index differs on {int((g['index'][b] != k).sum())}, "
              f"voiced differs on {int((g['voiced'][b].astype(bool) != voiced).sum())}")
        assert g["index"][b].dtype == np.int32 and np.array_equal(g["index"][b], k)
        assert g["voiced"][b].dtype == np.uint8 and np.array_equal(g["voiced"][b], voiced.astype(np.uint8))
        f0, ap = P.finish(c, k, sr, lo, hi)                            # the fp32 statement of the interpolation on the same values
        assert g["aperiodicity"][b].tobytes() == ap.astype(np.float32).tobytes()
        rel = float(np.abs(g["f0"][b].astype(np.float64) / f0.astype(np.float64) - 1).max())
        print(f"{name}[{b}]: f0 vs the fp32 interpolation of the same cmndf: rel {rel:.2e}")
        assert rel <= 1e-6                                             # two divides and an add: a few fp32 ulp


@pytest.mark.parametrize("name", NAMES)
def test_end_to_end_against_the_fp64_statement(name):
    sr, fl, hop, fmin, fmax, n, seeds, thr = P.CASES[name]
    _, r64, r32 = P.case(name)
    g = gpu(name)
    for b, (a, s) in enumerate(zip(r64, r32)):
        frames = a["index"].shape[0]
        differ = int(((g["index"][b] != a["index"]) | (g["voiced"][b].astype(bool) != a["voiced"])).sum())
        same, same32 = g["index"][b] == a["index"], s["index"] == a["index"]
        worst = float(np.abs(P.cents(g["f0"][b][same], a["f0"][same])).max())
        yard = float(np.abs(P.cents(s["f0"][same32], a["f0"][same32])).max())
        print(f"{name}[{b}]: {differ} of {frames} frames decide differently (cap {0.01 * frames:.2f}); f0 {worst:.2e} cents "
              f"(numpy fp32 {yard:.2e}, gate {max(4 * yard, 0.01):.2e})")
        assert differ <= 0.01 * frames
        assert worst <= max(4 * yard, 0.01)
        assert np.isfinite(g["f0"][b]).all() and (g["f0"][b] > 0).all()


def _raw_yin(x, par, B, n, frames, lags, guard=96):
    """jat_yin straight through the ABI into buffers with guard bands on both sides -> (rc, payloads, guards_intact)"""
    spec = {"f0": (torch.float32, B * frames), "aperiodicity": (torch.float32, B * frames), "voiced": (torch.uint8, B * frames),
            "index": (torch.int32, B * frames), "d": (torch.float32, B * frames * lags), "cmndf": (torch.float32, B * frames * lags)}
    bufs = {}
    for k, (dt, m) in spec.items():
        t = torch.empty(m + 2 * guard, dtype=dt, device="cuda")
        t.fill_(77)
        bufs[k] = t
    ptr = {k: C.c_void_p(t.data_ptr() + guard * t.element_size()) for k, t in bufs.items()}
    rc = L.lib().jat_yin(C.byref(par), L.ptr(x), B, n, ptr["f0"], ptr["aperiodicity"], ptr["voiced"], ptr["index"], ptr["d"],
                         ptr["cmndf"], L.stream_ptr())
    torch.cuda.synchronize()
    intact = all(bool((t[:guard] == 77).all()) and bool((t[-guard:] == 77).all()) for t in bufs.values())
    return rc, {k: t[guard:-guard].cpu().numpy() for k, t in bufs.items()}, intact


def test_determinism_batch_independence_and_guard_bands():
    name = "defaults"
    sr, fl, hop, fmin, fmax, n, seeds, thr = P.CASES[name]
    x = cuda(P.case(name)[0])
    g = gpu(name)
    again = pitch.yin_full(x, want=("index", "d", "cmndf"), **params(name))
    for k, v in again.items():
        assert v.cpu().numpy().tobytes() == g[k].tobytes(), k               # run to run
    alone = pitch.yin_full(x[1].clone(), want=("index", "d", "cmndf"), **params(name))
    for k, v in alone.items():
        assert v.cpu().numpy().tobytes() == g[k][1].tobytes(), k            # a row alone and inside a batch
    f0, voiced, ap = pitch.yin(x, **params(name))
    assert voiced.dtype == torch.bool and f0.shape == voiced.shape == ap.shape == (3, 1 + n // hop)
    assert f0.cpu().numpy().tobytes() == g["f0"].tobytes() and np.array_equal(voiced.cpu().numpy(), g["voiced"].astype(bool))
    # a row that ends at the end of an allocation: samples past L are never read, and nothing is written past an output
    lo, hi = P.periods(sr, fmin, fmax, fl)
    par = L.JatYinParams(fmin, fmax, sr, fl, hop, thr)
    rc, out, intact = _raw_yin(x, par, 3, n, 1 + n // hop, hi + 1)
    assert rc == 0 and intact
    for k, v in out.items():
        assert v.tobytes() == g[k].tobytes(), k
    short = "short"
    sr, fl, hop, fmin, fmax, n, seeds, thr = P.CASES[short]
    lo, hi = P.periods(sr, fmin, fmax, fl)
    rc, out, intact = _raw_yin(cuda(P.case(short)[0]), L.JatYinParams(fmin, fmax, sr, fl, hop, thr), 1, n, 1 + n // hop, hi + 1)
    assert rc == 0 and intact and out["d"].tobytes() == gpu(short)["d"].tobytes()
    # the nullable outputs left out: the other three are unchanged
    plain = pitch.yin_full(x, **params(name))
    assert sorted(plain) == ["aperiodicity", "f0", "voiced"] and plain["f0"].cpu().numpy().tobytes() == g["f0"].tobytes()
    # zeros are unvoiced, and an odd W (frame_length 18) takes the loop's remainder path
    z = pitch.yin_full(torch.zeros(5000, device="cuda"), want=("index", "cmndf"))
    assert not z["voiced"].any() and (z["index"] == 0).all() and (z["cmndf"][:, 1:] == 0).all()
    xs = P.mix(8000, 300, 3, 18)
    r = pitch.yin_full(cuda(xs), 8000, 900.0, 3900.0, 18, 5, 0.2, want=("index", "d", "cmndf"))
    a = P.yin(xs, 8000, 900.0, 3900.0, 18, 5, 0.2)
    d = r["d"].cpu().numpy().astype(np.float64)
    assert P.periods(8000, 900.0, 3900.0, 18) == (2, 8) and d.shape == (61, 9)
    assert (np.abs(d - a["d"]) <= (9 + 2) * U * a["d"]).all()
    k, v = P.select(r["cmndf"].cpu().numpy().astype(np.float64), 2, 8, float(np.float32(0.2)))
    assert np.array_equal(r["index"].cpu().numpy(), k) and np.array_equal(r["voiced"].cpu().numpy().astype(bool), v)


def _compare_case(fa, va, fb, vb, gross=50.0):
    got = pitch._counts(cuda(fa), cuda(va), cuda(fb), cuda(vb), gross).cpu().numpy()
    B = fa.shape[0]
    want = np.stack([P.compare_counts(fa[b], va[b], fb[b], vb[b], gross) for b in range(B)])
    print("f0_compare got", got.tolist(), "want", want.tolist())
    assert got.shape == (B, 6) and np.array_equal(got[:, :4], want[:, :4])
    assert (np.abs(got[:, 4:] - want[:, 4:]) <= 1e-6 * np.abs(want[:, 4:])).all()
    return got


def test_f0_compare_counts_and_sums():
    rng = np.random.default_rng(7)
    B, frames = 3, 1001
    fb = (100.0 * 2.0 ** rng.uniform(0, 3, (B, frames))).astype(np.float32)
    fa = (fb * 2.0 ** (rng.normal(0, 30.0, (B, frames)) / 1200.0)).astype(np.float32)
    fa[:, ::17] *= 2.0                                                       # octave errors
    va, vb = (rng.uniform(size=(B, frames)) < 0.7).astype(np.uint8), (rng.uniform(size=(B, frames)) < 0.6).astype(np.uint8)
    got = _compare_case(fa, va, fb, vb)
    assert (got[:, 3] > 0).all() and (got[:, 3] < got[:, 1]).all()
    _compare_case(fa, va, fb, vb, gross=5.0)
    none = _compare_case(fa, va, fb, np.zeros_like(vb))                      # no voiced frame in the reference
    assert (none[:, [0, 1, 3, 4, 5]] == 0).all() and np.array_equal(none[:, 2], va.sum(axis=1))
    gross = _compare_case(fb * np.float32(1.5), vb, fb, vb)                  # every both-voiced frame is gross
    assert np.array_equal(gross[:, 3], gross[:, 1]) and (gross[:, 5] == 0).all() and (gross[:, 4] > 0).all()
    same = _compare_case(fb, vb, fb, vb)                                     # identical tracks
    assert (same[:, 2:] == 0).all() and np.array_equal(same[:, 0], same[:, 1])
    # the public function: one row, bool flags, a dict of Python numbers; and a batch gives lists
    one = pitch.compare_f0(cuda(fa[0]), cuda(va[0]).bool(), cuda(fb[0]), cuda(vb[0]).bool())
    assert one == pitch.report_from_counts(got[0], frames) and isinstance(one["n_gross"], int)
    many = pitch.compare_f0(cuda(fa), cuda(va), cuda(fb), cuda(vb))
    assert many["mean_abs_cents"][0] == one["mean_abs_cents"] and len(many["n_frames"]) == B
    out = torch.zeros(1, 6, dtype=torch.float64, device="cuda")
    for bad in ((0, 10, 50.0), (65536, 10, 50.0), (1, 0, 50.0), (1, 10, -1.0), (1, 10, float("nan")), (1, 10, float("inf"))):
        rc = L.lib().jat_f0_compare(L.ptr(out), L.ptr(out), L.ptr(out), L.ptr(out), bad[0], bad[1], bad[2], L.ptr(out), L.stream_ptr())
        assert rc == L.JAT_E_INVALID and L.lib().jat_last_error(), bad
    assert L.lib().jat_f0_compare(None, L.ptr(out), L.ptr(out), L.ptr(out), 1, 6, 50.0, L.ptr(out), L.stream_ptr()) == L.JAT_E_INVALID


def test_refusals_through_the_abi():
    """every refusal of jat_yin: JAT_E_INVALID with a message, never a fault, and nothing is written"""
    x = torch.zeros(2, 4096, device="cuda")
    base = dict(fmin=50.0, fmax=1000.0, sr=44100, frame_length=2048, hop_length=512, trough_threshold=0.1)

    def call(B=1, n=4096, **over):
        v = dict(base, **over)
        par = L.JatYinParams(v["fmin"], v["fmax"], v["sr"], v["frame_length"], v["hop_length"], v["trough_threshold"])
        f0 = torch.full((2, 16), 5.0, device="cuda")
        ap, vo = torch.full((2, 16), 5.0, device="cuda"), torch.full((2, 16), 5, dtype=torch.uint8, device="cuda")
        rc = L.lib().jat_yin(C.byref(par), L.ptr(x), B, n, L.ptr(f0), L.ptr(ap), L.ptr(vo), None, None, None, L.stream_ptr())
        torch.cuda.synchronize()
        return rc, bool((f0 == 5).all() and (ap == 5).all() and (vo == 5).all())

    assert call()[0] == 0
    bad = [dict(frame_length=2047), dict(frame_length=14), dict(frame_length=8194), dict(frame_length=0), dict(hop_length=0),
           dict(hop_length=-3), dict(fmin=0.0), dict(fmin=-5.0), dict(fmax=50.0), dict(fmax=40.0), dict(fmax=22050.0),
           dict(fmax=30000.0), dict(sr=0), dict(fmin=20000.0, fmax=22000.0), dict(frame_length=16), dict(n=0), dict(n=-4),
           dict(B=0), dict(B=-1), dict(B=65536), dict(hop_length=1, n=2 ** 31), dict(hop_length=1, n=2 ** 22),
           dict(trough_threshold=float("nan")), dict(trough_threshold=float("inf")), dict(fmin=float("nan"))]
    for over in bad:
        kw = {k: over[k] for k in ("B", "n") if k in over}
        rc, untouched = call(**kw, **{k: v for k, v in over.items() if k not in ("B", "n")})
        assert rc == L.JAT_E_INVALID and untouched and L.lib().jat_last_error(), over
    par = L.JatYinParams(50.0, 1000.0, 44100, 2048, 512, 0.1)
    f0 = torch.zeros(2, 16, device="cuda")
    assert L.lib().jat_yin(None, L.ptr(x), 1, 4096, L.ptr(f0), L.ptr(f0), L.ptr(f0), None, None, None, L.stream_ptr()) == L.JAT_E_INVALID
    assert L.lib().jat_yin(C.byref(par), None, 1, 4096, L.ptr(f0), L.ptr(f0), L.ptr(f0), None, None, None, L.stream_ptr()) == L.JAT_E_INVALID
    assert L.lib().jat_yin(C.byref(par), L.ptr(x), 1, 4096, None, L.ptr(f0), L.ptr(f0), None, None, None, L.stream_ptr()) == L.JAT_E_INVALID
    # the Python layer turns them into ValueError
    with pytest.raises(ValueError, match="frame_length"):
        pitch.yin(x, frame_length=2047)
    with pytest.raises(ValueError, match="hop_length"):
        pitch.yin(x, hop_length=0)
    with pytest.raises(ValueError, match="threshold"):
        pitch.yin(x, trough_threshold=float("nan"))
    with pytest.raises(L.JatError, match="float32"):
        pitch.yin(x.double())


def test_fp16_library_gives_the_same_bits(tmp_path):
    code = ("import sys, numpy as np, torch\n"
            "sys.path.insert(0, 'tests')\n"
            "import jatsr_amd._lib as L\n"
            "import jatsr_amd.pitch as pitch\n"
            "import pitch_ref as P\n"
            "assert L.operand_dtype() == sys.argv[2]\n"
            "x = torch.from_numpy(np.stack([P.mix(16000, 16000 + 5, s, 1024) for s in (0, 1)])).cuda()\n"
            "r = pitch.yin_full(x, 16000, 40.0, 800.0, 1024, 256, 0.1, want=('index', 'd', 'cmndf'))\n"
            "r['counts'] = pitch._counts(r['f0'][:1], r['voiced'][:1], r['f0'][1:], r['voiced'][1:], 50.0)\n"
            "np.savez(sys.argv[1], **{k: v.cpu().numpy() for k, v in r.items()})\n")
    got = {}
    for dtype in ("bf16", "fp16"):
        env = dict(os.environ, JAT_OPERAND_DTYPE=dtype)
        env.pop("JAT_LIB_PATH", None)
        path = str(tmp_path / f"{dtype}.npz")
        out = subprocess.run([sys.executable, "-c", code, path, dtype], cwd=ROOT, env=env, capture_output=True, text=True,
                             timeout=600)
        assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
        got[dtype] = dict(np.load(path))
    assert sorted(got["bf16"]) == sorted(got["fp16"]) and len(got["bf16"]) == 7
    for k, v in got["bf16"].items():
        assert v.tobytes() == got["fp16"][k].tobytes(), k
    x = np.stack([P.mix(16000, 16000 + 5, s, 1024) for s in (0, 1)])
    ref = P.yin(x[0], 16000, 40.0, 800.0, 1024, 256, 0.1)
    assert (np.abs(got["fp16"]["d"][0] - ref["d"]) <= (512 + 2) * U * ref["d"]).all()


def test_f0_metrics_and_the_command_line(tmp_path):
    sr, n = 44100, 44100
    gt = P.mix(sr, n, 0)
    pred = (gt + 0.02 * np.random.default_rng(3).standard_normal(n)).astype(np.float32)
    low = P.mix(sr, n - 300, 1)
    rep = pitch.f0_metrics(cuda(pred), cuda(gt), cuda(low))
    assert sorted(rep) == ["generated", "lr_input"]
    tp, tg = (pitch.yin(cuda(v[:n])) for v in (pred, gt))
    assert rep["generated"] == pitch.compare_f0(tp[0], tp[1], tg[0], tg[1])
    tl, tg2 = (pitch.yin(cuda(v[:n - 300])) for v in (low, gt))
    assert rep["lr_input"] == pitch.compare_f0(tl[0], tl[1], tg2[0], tg2[1])
    assert rep["generated"]["n_frames"] == 1 + n // 512 and rep["lr_input"]["n_frames"] == 1 + (n - 300) // 512
    assert 0 < rep["generated"]["n_ref_voiced"] < rep["generated"]["n_frames"]
    assert rep["generated"]["raw_pitch_accuracy"] > 0.9 and rep["generated"]["mean_abs_cents"] < 20
    same = pitch.f0_metrics(cuda(gt), cuda(gt))["generated"]
    assert same["raw_pitch_accuracy"] == 1.0 and same["voicing_error_rate"] == 0.0 and same["mean_abs_cents"] == 0.0
    batch = pitch.f0_metrics(cuda(np.stack([pred, gt])), cuda(np.stack([gt, gt])))["generated"]
    assert batch["n_gross"] == [rep["generated"]["n_gross"], 0] and batch["mean_abs_cents"][0] == rep["generated"]["mean_abs_cents"]
    for name, v in (("pred", pred), ("gt", gt), ("low", low)):
        jio.write_wav_float32(tmp_path / f"{name}.wav", v, sr)
    out = pitch.main(["--pred", str(tmp_path / "pred.wav"), "--gt", str(tmp_path / "gt.wav"), "--lr", str(tmp_path / "low.wav"),
                      "--json", str(tmp_path / "rep.json"), "--track", str(tmp_path / "track.npy")])
    assert out == rep and json.loads((tmp_path / "rep.json").read_text()) == rep
    track = np.load(tmp_path / "track.npy")
    assert track.shape == (6, 1 + (n - 300) // 512) and track.dtype == np.float32
    assert np.array_equal(track[2], tg[0].cpu().numpy()[:track.shape[1]]) and set(np.unique(track[1])) <= {0.0, 1.0}


def test_infer_f0_metrics_flag(tmp_path):
    """the synthetic codec and checkpoint of tests/test_gpu_metrics.py: the flag adds the "f0" entry and changes nothing else"""
    from test_gpu_metrics import _infer_setup
    from jatsr_amd.infer import main as infer_main
    base = _infer_setup(tmp_path)
    infer_main(base + ["--output-dir", str(tmp_path / "m"), "--metrics"])
    infer_main(base + ["--output-dir", str(tmp_path / "mf"), "--metrics", "--f0-metrics"])
    infer_main(base + ["--output-dir", str(tmp_path / "f"), "--f0-metrics"])
    wavs = ["song_generated.wav", "song_hr_gt.wav", "song_lr_input.wav"]
    for d in ("m", "mf", "f"):
        assert sorted(os.listdir(tmp_path / d)) == sorted(wavs + ["song_generated.pt", "song_metrics.json"])
        for name in wavs:
            assert (tmp_path / d / name).read_bytes() == (tmp_path / "m" / name).read_bytes(), (d, name)
    plain, both, only = (json.loads((tmp_path / d / "song_metrics.json").read_text()) for d in ("m", "mf", "f"))
    assert "f0" not in plain and set(both) == set(plain) | {"f0"} and all(both[k] == plain[k] for k in plain)
    assert json.dumps({k: both[k] for k in plain}, indent=2) == (tmp_path / "m" / "song_metrics.json").read_text()
    assert list(only) == ["f0"] and only["f0"] == both["f0"]
    from jatsr_amd import metrics
    gen, hr, lr = (metrics.load_audio(tmp_path / "mf" / name)[0] for name in wavs)
    assert both["f0"] == pitch.f0_metrics(gen, hr, lr) and sorted(both["f0"]) == ["generated", "lr_input"]
    assert set(both["f0"]["generated"]) == set(pitch.RATE_KEYS) | set(pitch.COUNT_KEYS)
    assert both["f0"]["generated"]["n_frames"] == 1 + hr.shape[0] // 512


def test_prepare_f0_flag(tmp_path):
    """the WAVs and the synthetic codec of tests/test_gpu_prepare.py: --f0 adds hr_f0 / hr_voiced with the latent's frame
    count and changes nothing else; the readers ignore the new keys"""
    import jatsr_amd.recipe as recipe
    from test_gpu_prepare import _write_wavs
    from jatsr_amd.data import LatentStore
    from jatsr_amd.dac import load_dac_codec
    from jatsr_amd.prepare import hr_pitch_track, main as prepare_main
    full = {"decoder." + k: torch.from_numpy(v) for k, v in recipe.make_dac_state_dict().items()}
    full.update({k: torch.from_numpy(v) for k, v in recipe.make_dac_encoder_state_dict().items()})
    torch.save(full, tmp_path / "dac.pt")
    _write_wavs(tmp_path / "wav")
    argv = ["--source-dir", str(tmp_path / "wav"), "--dac-weights", str(tmp_path / "dac.pt"), "--val-fraction", "0.0", "--seed", "1"]
    prepare_main(argv + ["--output-dir", str(tmp_path / "plain")])
    prepare_main(argv + ["--output-dir", str(tmp_path / "f0"), "--f0"])
    codec = load_dac_codec(str(tmp_path / "dac.pt"))
    for stem in ("a", "b"):
        a = torch.load(tmp_path / "plain" / "train" / f"{stem}.pt", weights_only=False)
        b = torch.load(tmp_path / "f0" / "train" / f"{stem}.pt", weights_only=False)
        assert sorted(a) == ["hr_latent", "lr_latent", "metadata"] and sorted(b) == sorted(list(a) + ["hr_f0", "hr_voiced"])
        assert all(torch.equal(a[k], b[k]) for k in ("hr_latent", "lr_latent")) and a["metadata"] == b["metadata"]
        T = a["hr_latent"].shape[1]
        assert b["hr_f0"].shape == (T,) and b["hr_f0"].dtype == torch.float32 and not b["hr_f0"].is_cuda
        assert b["hr_voiced"].shape == (T,) and b["hr_voiced"].dtype == torch.uint8 and int(b["hr_voiced"].max()) <= 1
        x, sr = jio.read_wav(tmp_path / "wav" / f"{stem}.wav")
        f0, voiced = hr_pitch_track(torch.from_numpy(x).cuda(), sr, codec, T)
        assert torch.equal(f0.cpu(), b["hr_f0"]) and torch.equal(voiced.cpu(), b["hr_voiced"])
        f0_long, voiced_long = hr_pitch_track(torch.from_numpy(x).cuda(), sr, codec, T + 40)     # frames the track does not reach
        assert torch.equal(f0_long[:T], f0) and (f0_long[-30:] == 0).all() and (voiced_long[-30:] == 0).all()
        hr, lr = jio.load_latent_file(tmp_path / "f0" / "train" / f"{stem}.pt")
        assert torch.equal(hr, a["hr_latent"].float()) and torch.equal(lr, a["lr_latent"].float())
    for name in ("running_stats.pt", "global_stats_separated.json"):
        if name.endswith(".json"):
            assert (tmp_path / "plain" / name).read_bytes() == (tmp_path / "f0" / name).read_bytes()
    store = LatentStore(tmp_path / "f0", "train", frames=8)
    assert len(store) == 2 and store.lengths == LatentStore(tmp_path / "plain", "train", frames=8).lengths
