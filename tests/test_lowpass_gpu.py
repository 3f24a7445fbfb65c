"""The IIR low-pass cascades on the GPU (jat_iir_sosfilt / jat_iir_sosfiltfilt, jatsr_amd.lowpass, prepare_audio(lr_filter=),
infer --lr-filter) against the numpy twins of tests/lowpass_ref.py: within the accuracy gate of the fp64 twin, and bit for bit
equal to the blocked fp32 twin, whose rounding points are the kernel's."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lowpass_ref as R  # noqa: E402
import jatsr_amd  # noqa: E402,F401
import jatsr_amd.io as jio  # noqa: E402
import jatsr_amd.recipe as recipe  # noqa: E402
from jatsr_amd import _lib as L  # noqa: E402
from jatsr_amd import lowpass as LP  # noqa: E402
from stream_check import Case, check_case  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV, STATE_E = L.JAT_E_INVALID, L.JAT_E_STATE
F32 = np.float32
SENTINEL = 0x5A
NAMES = list(R.FILTERS)
ENTRIES = ("sosfilt", "sosfiltfilt")


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(t, a):
    got = t.detach().cpu().numpy()
    return got.shape == a.shape and got.dtype == a.dtype and got.tobytes() == np.ascontiguousarray(a).tobytes()


def sentinel(shape, dtype=torch.float32):
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(torch.uint8).fill_(SENTINEL)
    return t


def untouched(t):
    return bool((t.view(torch.uint8) == SENTINEL).all())


_banks = {}


def bank(which):
    """a single filter by index, "all" (the five filters of lowpass_ref.FILTERS) or "identity" """
    if which not in _banks:
        filters = R.filter_list()
        _banks[which] = LP.LowpassBank(filters if which == "all" else [np.zeros((0, 6))] if which == "identity" else [filters[which]])
    return _banks[which]


def run(entry, x, which, rows=None, out=None):
    return getattr(LP, entry)(x, bank(which), rows, out)


def cases_of(f):
    """{n: ([input names], x fp32 [inputs, n])} of filter f, from the shared references"""
    by_n = {}
    for (g, n, name), ref in R.references().items():
        if g == f:
            by_n.setdefault(n, []).append((name, ref["x"]))
    return {n: ([a for a, _ in v], np.stack([b for _, b in v])) for n, v in sorted(by_n.items())}


def test_geometry_and_padlen():
    lb, tile = C.c_int32(), C.c_int32()
    assert L.lib().jat_iir_geometry(C.byref(lb), C.byref(tile)) == 0 and L.lib().jat_iir_geometry(None, None) == 0
    assert (lb.value, tile.value) == (R.LANE_BLOCK, R.TILE) and tile.value % lb.value == 0
    table = R.Rows(R.filter_list())
    assert [bank(f).padlen for f in range(5)] == table.padlen.tolist() == [33, 33, 24, 9, 6]
    assert bank("all").padlen == 33 and bank("identity").padlen == 3


# ---- accuracy and the twin's bits -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", range(5), ids=NAMES)
def test_accuracy_against_the_fp64_twin(f):
    """white noise (both ways round), a unit step and unit impulses beside the lane-block and tile boundaries, at every length
    of lowpass_ref.lengths.  Gate per case: twice the larger error of the two fp32 twins against fp64 on that input, in rel-L2
    and in max-abs over the output's peak.  The kernel runs without contraction, so it also equals the blocked twin bit for bit."""
    refs = R.references()
    worst = {e: [0.0, 0.0, 0.0, 0.0] for e in ENTRIES}
    for n, (names, x) in cases_of(f).items():
        for entry in ENTRIES:
            if refs[(f, n, names[0])][entry] is None:
                assert n <= bank(f).padlen
                continue
            y = run(entry, cuda(x), f).cpu().numpy()
            for i, name in enumerate(names):
                ref = refs[(f, n, name)][entry]
                for j, metric in enumerate((R.rel_l2, R.rel_max)):
                    got, gate = metric(y[i], ref["f64"]), R.gate(ref, metric)
                    assert got <= gate, (NAMES[f], entry, n, name, metric.__name__, got, gate)
                    if name == "noise" and n == R.LONGEST:
                        worst[entry][2 * j:2 * j + 2] = [got, gate]
                assert y[i].tobytes() == ref["blocked"].tobytes(), (NAMES[f], entry, n, name)
    for entry in ENTRIES:
        w = worst[entry]
        print(f"{NAMES[f]:16s} {entry:12s} noise, n = {R.LONGEST}: rel-L2 {w[0]:.2e} (gate {w[1]:.2e}), max-abs / peak {w[2]:.2e} "
              f"(gate {w[3]:.2e})")


def test_identity_cascade_returns_the_input():
    for n in R.lengths(3):
        x = R.noise(n, 9)
        x[n // 2] = -0.0
        for entry in ENTRIES:
            assert same_bits(run(entry, cuda(x), "identity"), x), (entry, n)


# ---- identical bits ---------------------------------------------------------------------------------------------------------------------
BATCH = (0, 3, 1)          # Butterworth 10, Butterworth 2 beside it, Chebyshev 10
BATCH_B = (2, 4, 3)        # Chebyshev 7, Butterworth 1, Butterworth 2


@pytest.mark.parametrize("rows", [BATCH, BATCH_B], ids=["b10_b2_c10", "c7_b1_b2"])
def test_a_row_alone_in_a_batch_again_and_in_place(rows):
    """B = 3 with a different filter on every row against B = 1 of each row (one bank of all five filters, and the row's own
    bank), a second run, and y = x"""
    for n in R.lengths(33):
        x = np.stack([R.noise(n, 20 + r) for r in rows])
        dx = cuda(x)
        for entry in ENTRIES:
            if entry == "sosfiltfilt" and n <= 33:
                with pytest.raises(ValueError, match="padlen"):
                    run(entry, dx, "all", rows)
                continue
            y = run(entry, dx, "all", rows)
            assert same_bits(dx, x)
            assert torch.equal(run(entry, dx, "all", rows), y), (entry, n)                      # again
            for i, f in enumerate(rows):
                assert torch.equal(run(entry, dx[i:i + 1], "all", [f]), y[i:i + 1]), (entry, n, f)   # alone, the same table
                assert torch.equal(run(entry, dx[i], f), y[i]), (entry, n, f)                          # alone, its own table
            z = dx.clone()
            assert run(entry, z, "all", rows, out=z) is z and torch.equal(z, y), (entry, n)     # in place


def small_run():
    """both entries once on a batch of different filters across a tile boundary"""
    n = R.TILE + 1
    x = cuda(np.stack([R.noise(n, 20 + r) for r in BATCH]))
    return {entry: run(entry, x, "all", BATCH).cpu().numpy() for entry in ENTRIES}


def test_fp16_library_gives_the_same_bits(tmp_path):
    """iir.hip is fp32 in both builds: libjat_hip_fp16.so (a child process) computes what this process computes"""
    code = ("import sys, numpy as np\n"
            "sys.path.insert(0, 'tests')\n"
            "import jatsr_amd._lib as L\n"
            "from test_lowpass_gpu import small_run\n"
            "assert L.operand_dtype() == 'fp16'\n"
            "np.savez(sys.argv[1], **small_run())\n")
    env = dict(os.environ, JAT_OPERAND_DTYPE="fp16")
    env.pop("JAT_LIB_PATH", None)
    path = str(tmp_path / "fp16.npz")
    out = subprocess.run([sys.executable, "-c", code, path], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
    other, here = dict(np.load(path)), small_run()
    assert sorted(other) == sorted(here) == sorted(ENTRIES)
    for k, v in here.items():
        assert v.tobytes() == other[k].tobytes(), k


# ---- values -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", range(5), ids=NAMES)
def test_values(f):
    refs, n = R.references(), R.LONGEST
    sos = R.filter_list()[f]
    # a step settles to the design's DC gain (the Chebyshev 10 at sr / 48 rings longest: e^-35 after 12 000 samples)
    step = run("sosfilt", cuda(np.ones(n, F32)), f).cpu().numpy()
    assert abs(step[-1] - LP.dc_gain(sos)) <= R.gate(refs[(f, n, "step")]["sosfilt"], R.rel_max) * np.abs(step).max() + 2.0 ** -23
    # the zero-phase filter commutes with time reversal: the reversed input gives the reversed output.  scipy's sosfiltfilt is
    # forward-then-backward, its mirror image backward-then-forward: the two agree once the edge transients have died, so the
    # rows are compared farther than one tile (e^-24 for the Chebyshev 10 at sr / 48, the longest memory here) from both ends
    rev = run("sosfiltfilt", cuda(refs[(f, n, "reversed")]["x"]), f).cpu().numpy()
    want = refs[(f, n, "noise")]["sosfiltfilt"]["f64"][::-1]
    inner = slice(R.TILE, n - R.TILE)
    ref = {k: v[inner] for k, v in refs[(f, n, "reversed")]["sosfiltfilt"].items()}
    for metric in (R.rel_l2, R.rel_max):
        assert metric(rev[inner], want[inner]) <= R.gate(ref, metric), metric.__name__
    # its impulse response is symmetric about the impulse, which sits 8192 samples from the nearer end
    ref = refs[(f, n, f"impulse@{R.TILE}")]["sosfiltfilt"]
    h = run("sosfiltfilt", cuda(refs[(f, n, f"impulse@{R.TILE}")]["x"]), f).cpu().numpy()
    left, right = h[:R.TILE + 1][::-1], h[R.TILE:2 * R.TILE + 1]
    assert np.abs(left - right).max() <= R.gate(ref, R.rel_max) * np.abs(ref["f64"]).max()
    assert np.abs(ref["f64"][:64]).max() <= 1e-6 * np.abs(ref["f64"]).max()   # decayed below fp32's resolution before either end


# ---- streams ------------------------------------------------------------------------------------------------------------------------------
def raw(entry, handle, idx, x, y, B, n, work, nbytes=None):
    fn = getattr(L.lib(), "jat_iir_" + entry)
    return fn(handle, L.ptr(idx), L.ptr(x), L.ptr(y), B, n, L.ptr(work), work.numel() if nbytes is None and work is not None else nbytes or 0,
              L.stream_ptr())


def stream_cases():
    n = R.TILE + 1
    x = np.stack([R.noise(n, 20 + r) for r in BATCH])
    idx = torch.tensor(BATCH, dtype=torch.int32, device="cuda")
    work = torch.empty(LP.workspace_bytes(3, n), dtype=torch.uint8, device="cuda")

    def case(entry):
        def call(st, i, o):
            assert raw(entry, bank("all").ptr, i["rows"], i["x"], o["y"], 3, n, work) == 0
            return {"w_y": getattr(LP, entry)(i["x"], bank("all"), BATCH)}
        return Case({"x": cuda(x), "rows": idx}, call, outputs={"y": torch.empty(3, n, device="cuda")},
                    decoys={"rows": torch.tensor(BATCH_B, dtype=torch.int32, device="cuda")})
    return {"jat_iir_sosfilt": lambda: case("sosfilt"), "jat_iir_sosfiltfilt": lambda: case("sosfiltfilt")}


def test_every_stream_taking_entry_has_a_case():
    header = open(os.path.join(ROOT, "include", "jat_hip_iir.h")).read()
    takes = set(re.findall(r"\bint (jat_[a-z0-9_]+)\([^;]*void\* stream\)", header))
    assert takes == set(stream_cases()) and len(takes) == 2


@pytest.mark.parametrize("name", ["jat_iir_sosfilt", "jat_iir_sosfiltfilt"])
def test_side_stream(name):
    check_case(stream_cases()[name](), name, synchronises=False)


def test_graph_capture():
    """both entries captured into one graph and replayed after the input and the row filters changed: no allocation,
    synchronisation or copy in the filtering calls"""
    n = R.TILE + 1
    xa, xb = (np.stack([R.noise(n, s + r) for r in range(3)]) for s in (30, 40))
    x, idx = cuda(xa), torch.tensor(BATCH, dtype=torch.int32, device="cuda")
    y1, y2 = torch.zeros(3, n, device="cuda"), torch.zeros(3, n, device="cuda")
    work = torch.empty(LP.workspace_bytes(3, n), dtype=torch.uint8, device="cuda")
    h = bank("all").ptr

    def go():
        assert raw("sosfilt", h, idx, x, y1, 3, n, work) == 0
        assert raw("sosfiltfilt", h, idx, x, y2, 3, n, work) == 0
    go()                                                                  # eagerly once: what the first launch of a kernel sets up
    torch.cuda.synchronize()
    first = y2.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        go()
    x.copy_(cuda(xb))
    idx.copy_(torch.tensor(BATCH_B, dtype=torch.int32, device="cuda"))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y1, LP.sosfilt(cuda(xb), bank("all"), BATCH_B)) and torch.equal(y2, LP.sosfiltfilt(cuda(xb), bank("all"), BATCH_B))
    assert not torch.equal(y2, first)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_through_the_raw_abi_write_nothing():
    n = 100
    x, idx = cuda(np.stack([R.noise(n, r) for r in range(3)])), torch.tensor(BATCH, dtype=torch.int32, device="cuda")
    y = sentinel((3, n))
    nbytes = LP.workspace_bytes(3, n)
    work = sentinel((nbytes,), torch.uint8)
    h = bank("all").ptr
    ok = dict(handle=h, idx=idx, x=x, y=y, B=3, n=n, work=work, nbytes=nbytes)
    for entry in ENTRIES:
        assert raw(entry, **dict(ok, work=work, nbytes=nbytes - 1)) == STATE_E, entry
        for bad in (dict(handle=None), dict(idx=None), dict(x=None), dict(y=None), dict(work=None), dict(B=0), dict(B=-1), dict(B=65536),
                    dict(n=0), dict(n=-5), dict(n=(1 << 30) + 1)):
            assert raw(entry, **dict(ok, **bad)) == INV, (entry, bad)
    for short in (33, 10, 1):                                             # n <= padlen, as scipy refuses it
        assert raw("sosfiltfilt", **dict(ok, n=short)) == INV
    assert raw("sosfiltfilt", bank(3).ptr, idx, x, y, 3, 9, work, nbytes) == INV    # Butterworth 2: padlen 9
    torch.cuda.synchronize()
    assert untouched(y) and untouched(work)
    assert raw("sosfiltfilt", bank(3).ptr, torch.zeros(3, dtype=torch.int32, device="cuda"), x, y, 3, 10, work, nbytes) == 0   # padlen + 1 is taken
    size = C.c_size_t(7)
    for B, m in ((0, 10), (65536, 10), (1, 0), (1, (1 << 30) + 1)):
        assert L.lib().jat_iir_workspace_bytes(B, m, C.byref(size)) == INV and size.value == 7
    assert L.lib().jat_iir_workspace_bytes(1, 10, None) == INV
    # create: what a table must not hold
    sos, zi, pw = (np.ascontiguousarray(a, np.float64) for a in (bank("all").sos, bank("all").zi, bank("all").powers))
    dbl = C.POINTER(C.c_double)
    out = C.c_void_p()

    def create(s=sos, z=zi, p=pw, Rn=5, o=C.byref(out)):
        return L.lib().jat_iir_create(*(None if a is None else a.ctypes.data_as(dbl) for a in (s, z, p)), Rn, L.stream_ptr(), o)
    bad_a0, bad_nan, bad_gap = sos.copy(), sos.copy(), sos.copy()
    bad_a0[1, 0, 3] = 2.0
    bad_nan[2, 1, 4] = np.nan
    bad_gap[3, 0] = [1, 0, 0, 1, 0, 0]                                    # Butterworth 2 is one section: an identity in front of nothing is fine
    bad_gap[0, 0] = [1, 0, 0, 1, 0, 0]                                    # an identity in front of four sections is not
    for kw in (dict(s=None), dict(z=None), dict(p=None), dict(Rn=0), dict(Rn=4097), dict(o=None), dict(s=bad_a0), dict(s=bad_nan),
               dict(s=bad_gap), dict(z=zi * np.inf), dict(p=pw * np.nan)):
        assert create(**kw) == INV and not out.value, list(kw)


def test_refusals_in_python():
    x = cuda(np.stack([R.noise(100, r) for r in range(3)]))
    for rows, what in (([0, 1, 5], "outside 0..4"), ([0, -1, 2], "outside 0..4"), ([0, 1], "3 rows"), (None, "needs `rows`")):
        for entry in ENTRIES:                                             # the device cannot refuse an index: the host does
            with pytest.raises(ValueError, match=what):
                run(entry, x, "all", rows)
    with pytest.raises(ValueError, match="padlen"):
        LP.sosfiltfilt(x[:, :33], bank(0))
    with pytest.raises(L.JatError, match="CUDA"):
        LP.sosfilt(x.cpu(), bank(0))
    with pytest.raises(L.JatError, match="float32"):
        LP.sosfilt(x.double(), bank(0))
    with pytest.raises(ValueError, match="out must be"):
        LP.sosfilt(x, bank(0), out=torch.empty(3, 99, device="cuda"))
    with pytest.raises(L.JatError, match="S <= 5"):
        LP.LowpassBank([np.tile([1.0, 0, 0, 1, 0, 0], (6, 1))])
    with pytest.raises(L.JatError, match="cutoff"):
        LP.simulate_lr_filtered(x, 48000, {"kind": "butter", "order": 4, "cutoff_hz": 10.0})
    y = LP.sosfiltfilt(x.view(3, 1, 100), LP.design_sos("butter", 4, 6000.0, 48000))       # an sos in place of a bank, leading axes kept
    assert y.shape == (3, 1, 100) and torch.equal(y.view(3, 100), LP.simulate_lr_filtered(x, 48000, {"kind": "butter", "order": 4,
                                                                                                    "cutoff_hz": 6000.0}))


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dac_file(tmp_path_factory):
    full = {"decoder." + k: torch.from_numpy(v) for k, v in recipe.make_dac_state_dict().items()}
    full.update({k: torch.from_numpy(v) for k, v in recipe.make_dac_encoder_state_dict().items()})
    path = tmp_path_factory.mktemp("dac") / "dac.pt"
    torch.save(full, path)
    return str(path)


CHEBY = {"kind": "cheby1", "order": 8, "cutoff_hz": 4000.0, "ripple_db": 1.0}


def test_prepare_audio_with_a_filter(dac_file):
    import jatsr_amd.dac as D
    from jatsr_amd.prepare import HIGH_SR, chunk_bounds, prepare_audio, to_codec_rate
    codec = D.load_dac_codec(dac_file)
    sr = 22050
    x = recipe.make_dac_audio(1, int(9.3 * sr), 41, sample_rate=sr)[0, 0]
    plain = prepare_audio(x, sr, codec)
    assert "lr_filter" not in plain
    never = prepare_audio(x, sr, codec, lr_filter=None)
    assert all(torch.equal(plain[k], never[k]) for k in ("hr_latent", "lr_latent", "sum", "sq_sum")) and "lr_filter" not in never
    res = prepare_audio(x, sr, codec, lr_filter=dict(CHEBY))
    assert res["lr_filter"] == CHEBY
    assert torch.equal(res["hr_latent"], plain["hr_latent"]) and not torch.equal(res["lr_latent"], plain["lr_latent"])
    assert res["lr_latent"].shape == plain["lr_latent"].shape
    # by hand: the filter on each chunk at 48 kHz in the place of the round trip
    from jatsr_amd.resample import resample
    xg = torch.from_numpy(x).cuda()
    chunks = torch.stack([torch.nn.functional.pad(xg[a:b], (pl, pr)) for a, b, pl, pr in chunk_bounds(len(x), sr)])
    lr48 = LP.sosfiltfilt(resample(chunks, sr, HIGH_SR), LP.filter_sos(CHEBY, HIGH_SR))
    z = codec.encode(to_codec_rate(lr48, codec)[:, None])[0]
    md = res["metadata"]
    by_hand = torch.cat(list(z[..., md["trim_frames"]:md["trim_frames"] + md["valid_frames"]]), dim=-1)[..., :md["frames"]]
    assert torch.equal(res["lr_latent"], by_hand)
    sinc = prepare_audio(x, sr, codec, lr_filter={"kind": "sinc"})       # a `mix` draw of the round trip: today's latents, and the record
    assert torch.equal(sinc["lr_latent"], plain["lr_latent"]) and sinc["lr_filter"] == {"kind": "sinc", "low_sr": 16000}


def test_command_lines(tmp_path, dac_file):
    import json

    from jatsr_amd.infer import main as infer_main
    from jatsr_amd.prepare import main as prepare_main
    sr = 22050
    os.makedirs(tmp_path / "src")
    for i in range(3):
        jio.write_wav_float32(tmp_path / "src" / f"song{i}.wav", recipe.make_dac_audio(1, int(3.0 * sr), 50 + i, sample_rate=sr)[0, 0], sr)
    base = ["--source-dir", str(tmp_path / "src"), "--dac-weights", dac_file, "--val-fraction", "0"]
    rep = prepare_main(base + ["--output-dir", str(tmp_path / "mix"), "--lr-filter", "mix", "--lr-cutoff-hz", "2000,8000", "--lr-seed", "3"])
    assert len(rep["written"]) == 3 and sum(rep["lr_filters"].values()) == 3
    for i in range(3):
        got = torch.load(tmp_path / "mix" / "train" / f"song{i}.pt", weights_only=False)
        want = LP.random_filter(3, f"song{i}", ("sinc", "butter", "cheby1"), (2000.0, 8000.0), (4, 10), 1.0)
        assert {k: v for k, v in got["lr_filter"].items() if k != "low_sr"} == want
        assert got["lr_latent"].dtype == torch.float16 and got["lr_latent"].shape == got["hr_latent"].shape
    rep = prepare_main(base + ["--output-dir", str(tmp_path / "plain")])
    assert "lr_filters" not in rep and "lr_filter" not in torch.load(tmp_path / "plain" / "train" / "song0.pt", weights_only=False)
    # infer: one fixed filter for the evaluation input
    cfg = dict(recipe.CONFIGS["micro"], input_channels=1024, cond_channels=1024)
    torch.save({"model_state_dict": {k: torch.from_numpy(v) for k, v in recipe.make_state_dict(cfg).items()}, "config": dict(cfg)},
               tmp_path / "last.pt")
    ones, zeros = [1.0] * 1024, [0.0] * 1024
    (tmp_path / "stats.json").write_text(json.dumps({"hr_mean": zeros, "hr_std": ones, "lr_mean": zeros, "lr_std": ones}))
    common = ["--checkpoint", str(tmp_path / "last.pt"), "--stats-file", str(tmp_path / "stats.json"), "--steps", "2", "--seed", "3",
              "--dac-weights", dac_file, "--input-audio", str(tmp_path / "src" / "song0.wav"), "--simulate-lr"]
    infer_main(common + ["--output-dir", str(tmp_path / "o"), "--lr-filter", "butter", "--lr-cutoff-hz", "6000", "--lr-order", "8"])
    infer_main(common + ["--output-dir", str(tmp_path / "p")])
    out, ref = (torch.load(tmp_path / d / "song0_generated.pt", weights_only=False) for d in ("o", "p"))
    assert torch.equal(out["hr_latent"], ref["hr_latent"]) and not torch.equal(out["lr_latent"], ref["lr_latent"])
    assert out["generated_latent"].shape == out["lr_latent"].shape
    names = sorted(f for f in os.listdir(tmp_path / "o") if f.endswith(".wav"))
    assert names == ["song0_generated.wav", "song0_hr_gt.wav", "song0_lr_input.wav"]
    # the module's own command line
    LP.main(["--in", str(tmp_path / "src" / "song1.wav"), "--out", str(tmp_path / "lp.wav"), "--kind", "cheby1", "--order", "8",
             "--cutoff-hz", "4000"])
    y, sr2 = jio.read_wav(tmp_path / "lp.wav")
    x, _ = jio.read_wav(tmp_path / "src" / "song1.wav")
    want = LP.sosfiltfilt(cuda(x), LP.design_sos("cheby1", 8, 4000.0, sr)).cpu().numpy()
    assert sr2 == sr and y.tobytes() == want.tobytes()


def test_detected_cutoff_report():
    """a report, not a gate: splice.detect_cutoff (1 + the last bin within 60 dB of the loudest, in Hz; it can name the bin past
    Nyquist) on 4 s of filtered white noise, as it comes out and with 0.25 s raised-cosine fades at both ends.  The clip as it
    comes out starts and ends with a step inside the centred edge frames of the STFT; its 1 / f spectrum, averaged over the 375
    frames, lies within 60 dB of the passband up to the top of the band, and the detector reports that, not the filter:
    Butterworth 8 at 4000 Hz -> 21562 Hz, Chebyshev 8 at 8000 Hz -> 20789 Hz, Chebyshev 10 at 12000 Hz -> 24023 Hz (MI355X; the
    numpy restatement of tests/splice_ref.py on scipy's fp64 output gives the same three figures).  Faded, the detector finds the
    -60 dB points of the squared responses: 5953, 9141 and 12844 Hz."""
    from jatsr_amd import splice
    x = cuda(R.noise(4 * 48000, 77))
    fade = torch.ones_like(x)
    ramp = 0.5 - 0.5 * torch.cos(torch.pi * torch.arange(12000, device="cuda") / 12000)
    fade[:12000], fade[-12000:] = ramp, ramp.flip(0)
    for kind, order, cut in (("butter", 8, 4000.0), ("cheby1", 8, 8000.0), ("cheby1", 10, 12000.0)):
        y = LP.simulate_lr_filtered(x, 48000, {"kind": kind, "order": order, "cutoff_hz": cut})
        hz, faded = float(splice.detect_cutoff(y, sr=48000)), float(splice.detect_cutoff(y * fade, sr=48000))
        print(f"detect_cutoff: {kind} order {order} designed {cut:.0f} Hz -> detected {hz:.0f} Hz as it comes out, {faded:.0f} Hz faded")
        assert hz > 0.0 and faded > 0.0                                   # reported, not gated
