"""Inverse STFT, long-term spectrum and low-band splice on the GPU (csrc/splice.hip behind jat_istft, jat_ltas and
jat_band_splice; jatsr_amd.splice) against the fp64 restatement tests/splice_ref.py, at the smallest shapes at which each
mechanism can go wrong (splice_ref.GPU_SHAPES), each with B = 1 and B = 3.

Gates.  Every accuracy test computes the error of the fp32 restatement on the same inputs: that is the yardstick, and the
gate is 10x it, in rel-L2 and in max-abs over the signal's peak (the forward STFT alone sits at up to 3x its own yardstick,
DESIGN 12; the splice chains a second transform, the overlap-add and a divide).  Measured on MI355X, rel-L2, GPU / yardstick,
at 2048 / 512 / 132300: round trip 1.16e-7 / 9.5e-8, istft of a random spectrogram 1.31e-7 / 1.36e-7, splice 7.8e-8 / 6.6e-8,
unit gain 2.17e-7 / 1.78e-7, ltas 5.3e-8 / 5.7e-9 (the long-term spectrum averages the yardstick's random error away over
259 frames; what is left on the GPU is the fixed rounding of the fp32 twiddle tables, the same in every frame: 9.2x, the
closest any case comes to its gate).  The other shapes: DESIGN 14."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import metrics_ref as M  # noqa: E402
import splice_ref as S  # noqa: E402
import jatsr_amd.io as jio  # noqa: E402
import jatsr_amd.metrics as metrics  # noqa: E402
import jatsr_amd.recipe as recipe  # noqa: E402
import jatsr_amd.splice as splice  # noqa: E402
from jatsr_amd import _lib as L  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [pytest.param(n_fft, hop, n, B, id=f"{n_fft}-{hop}-{n}-B{B}") for n_fft, hop, n in S.GPU_SHAPES for B in (1, 3)]


def gate(what, got, ref, yard):
    """got (GPU) and yard (fp32 restatement) against ref (fp64): print every figure, then 10x the yardstick"""
    r, m = S.rel_l2(got, ref), S.max_over_peak(got, ref)
    ry, my = S.rel_l2(yard, ref), S.max_over_peak(yard, ref)
    print(f"{what}: rel-L2 {r:.2e} (fp32 restatement {ry:.2e}), max-abs/peak {m:.2e} ({my:.2e})")
    assert np.isfinite(np.asarray(got)).all()
    assert r <= 10 * ry and m <= 10 * my, (what, r, ry, m, my)


def cuda(a):
    return torch.from_numpy(np.array(a)).cuda()


@functools.lru_cache(maxsize=None)
def fixture(n_fft, hop, n):
    """three rows per shape, made once: signals, a random spectrogram, the splice pair and every fp64 / fp32 restatement"""
    x = S.noise((3, n), seed=n)
    X = S.random_spectrogram(3, n_fft, hop, n, seed=n + 1)
    g, s = S.noise((3, n + 37), seed=n + 2), S.noise((3, n), seed=n + 3, scale=0.2)
    a = S.band_gain(44100, n_fft, 6000.0, 1500.0)
    f = dict(x=x, X=X, g=g, s=s, a=a)
    f["rt32"] = S.istft(M.stft(x, n_fft, hop, np.float32), n, n_fft, hop, np.float32)
    f["inv64"], f["inv32"] = S.istft(X, n, n_fft, hop), S.istft(X, n, n_fft, hop, np.float32)
    f["sp64"], f["sp32"] = S.splice(g, s, a, n_fft, hop), S.splice(g, s, a, n_fft, hop, np.float32)
    f["back64"], f["back32"] = S.splice(s, g, a, n_fft, hop), S.splice(s, g, a, n_fft, hop, np.float32)
    ones = np.ones_like(a)
    f["one32"] = S.splice(g, s, ones, n_fft, hop, np.float32)
    f["lt64"], f["lt32"] = S.ltas(x, n_fft, hop), S.ltas(x, n_fft, hop, np.float32)
    for v in f.values():
        v.setflags(write=False)
    return f


# ---- accuracy against the fp64 restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,hop,n,B", CASES)
def test_round_trip(n_fft, hop, n, B):
    f = fixture(n_fft, hop, n)
    x = cuda(f["x"][:B])
    y = splice.istft(metrics.stft(x, n_fft, hop), n, n_fft, hop)
    assert y.shape == (B, n) and y.dtype == torch.float32
    gate("istft(stft(x))", y.cpu().numpy(), f["x"][:B].astype(np.float64), f["rt32"][:B])
    y1 = splice.istft(metrics.stft(x[0], n_fft, hop), n, n_fft, hop)                       # [L] in, [L] out
    assert y1.shape == (n,) and torch.equal(y1, y[0])


@pytest.mark.parametrize("n_fft,hop,n,B", CASES)
def test_istft_of_a_random_spectrogram(n_fft, hop, n, B):
    f = fixture(n_fft, hop, n)
    y = splice.istft(cuda(f["X"][:B]), n, n_fft, hop)
    gate("istft(X)", y.cpu().numpy(), f["inv64"][:B], f["inv32"][:B])


@pytest.mark.parametrize("n_fft,hop,n,B", CASES)
def test_splice(n_fft, hop, n, B):
    f = fixture(n_fft, hop, n)
    g, s = cuda(f["g"][:B]), cuda(f["s"][:B])
    out = splice.splice_gain(g, s, torch.from_numpy(f["a"].copy()), n_fft, hop)
    assert out.shape == g.shape
    gate("splice", out.cpu().numpy(), f["sp64"][:B], f["sp32"][:B])
    # exact properties: past the shorter signal the output is `generated`; a second run and a row alone give the same bits
    assert torch.equal(out[:, n:], g[:, n:])
    assert torch.equal(out, splice.splice_gain(g, s, torch.from_numpy(f["a"].copy()), n_fft, hop))
    alone = splice.splice_gain(g[B - 1], s[B - 1], torch.from_numpy(f["a"].copy()), n_fft, hop)
    assert alone.shape == (n + 37,) and torch.equal(alone, out[B - 1])
    # the signals the other way round: source longer than generated
    back = splice.splice_gain(s, g, torch.from_numpy(f["a"].copy()), n_fft, hop)
    gate("splice, source longer", back.cpu().numpy(), f["back64"][:B], f["back32"][:B])


@pytest.mark.parametrize("n_fft,hop,n,B", CASES)
def test_zero_gain_returns_generated_bit_for_bit(n_fft, hop, n, B):
    f = fixture(n_fft, hop, n)
    g, s = cuda(f["g"][:B]), cuda(f["s"][:B])
    out = splice.splice_gain(g, s, torch.zeros(1 + n_fft // 2), n_fft, hop)
    assert torch.equal(out.view(torch.int32), g.view(torch.int32))
    out, hz = splice.splice_lowband(g, s, cutoff_hz=0.0, n_fft=n_fft, hop_length=hop)
    assert hz == 0.0 and torch.equal(out.view(torch.int32), g.view(torch.int32))


@pytest.mark.parametrize("n_fft,hop,n,B", CASES)
def test_unit_gain_returns_source(n_fft, hop, n, B):
    f = fixture(n_fft, hop, n)
    g, s = cuda(f["g"][:B]), cuda(f["s"][:B])
    out = splice.splice_gain(g, s, torch.ones(1 + n_fft // 2), n_fft, hop)
    ref = np.concatenate([f["s"][:B], f["g"][:B, n:]], axis=1).astype(np.float64)
    gate("unit gain", out.cpu().numpy(), ref, f["one32"][:B])
    assert torch.equal(out[:, n:], g[:, n:])


@pytest.mark.parametrize("n_fft,hop,n,B", CASES)
def test_ltas(n_fft, hop, n, B):
    f = fixture(n_fft, hop, n)
    x = cuda(f["x"][:B])
    P = splice.ltas(x, n_fft, hop)
    assert P.shape == (B, 1 + n_fft // 2) and P.dtype == torch.float64
    gate("ltas", P.cpu().numpy(), f["lt64"][:B], f["lt32"][:B])
    assert torch.equal(P, splice.ltas(x, n_fft, hop)) and torch.equal(splice.ltas(x[B - 1], n_fft, hop), P[B - 1])


# ---- what the splice is for ------------------------------------------------------------------------------------------------------
def test_band_behaviour():
    s, g = S.band_fixture()
    out, hz = splice.splice_lowband(cuda(g), cuda(s), cutoff_hz=4000.0)
    out = out.cpu().numpy()
    a = splice.band_gain(44100, 2048, 4000.0, 500.0).numpy()
    assert hz == 4000.0
    gate("band splice", out, S.splice(g, s, a), S.splice(g, s, a, dtype=np.float32))
    k1, k12 = round(1000 * 2048 / 44100), round(12000 * 2048 / 44100)
    O, So, G = (np.abs(M.stft(v)[:, 4:-4]) for v in (out, s, g))             # frames that lie wholly inside the signal
    e1, e12 = np.abs(O[k1] / So[k1] - 1).max(), np.abs(O[k12] / G[k12] - 1).max()
    print(f"1 kHz bin vs source {e1:.1e}, 12 kHz bin vs generated {e12:.1e}")
    assert e1 < 1e-3 and e12 < 1e-3


def test_cutoff_detection():
    x = S.cutoff_fixture(rows=3)
    want = [S.cutoff_bin(S.ltas(row), S.CUTOFF_DB) for row in x]            # margins: tests/test_splice_cpu.py
    got = splice.detect_cutoff(cuda(x), threshold_db=S.CUTOFF_DB)
    assert got == [b * 44100 / 2048 for b in want]
    assert splice.detect_cutoff(cuda(x[0]), threshold_db=S.CUTOFF_DB) == got[0]
    assert splice.detect_cutoff(torch.zeros(3000, device="cuda")) == 0.0    # silence
    # the default threshold: the same decision as the restatement makes on the GPU's own spectrum, and auto-detection
    # hands that cutoff to the splice
    P = splice.ltas(cuda(x[0])).cpu().numpy()
    hz = splice.detect_cutoff(cuda(x[0]))
    assert hz == S.cutoff_bin(P) * 44100 / 2048
    g = cuda(S.noise((88200,), seed=5))
    out, used = splice.splice_lowband(g, cuda(x[0]))
    assert used == hz and torch.equal(out, splice.splice_lowband(g, cuda(x[0]), cutoff_hz=hz)[0])


def test_refusals():
    x = torch.zeros(2, 5000, device="cuda")
    with pytest.raises(ValueError, match="divide"):
        splice.splice_lowband(x, x, cutoff_hz=4000.0, hop_length=500)
    with pytest.raises(ValueError, match="n_fft / 4"):
        splice.istft(torch.zeros(1025, 5, dtype=torch.complex64, device="cuda"), 5000, 2048, 1024)
    with pytest.raises(ValueError, match="frames"):
        splice.istft(torch.zeros(1025, 9, dtype=torch.complex64, device="cuda"), 5000)
    with pytest.raises(L.JatError):
        splice.splice_lowband(x, x[:1], cutoff_hz=4000.0)
    with pytest.raises(L.JatError, match="gain"):
        splice.splice_gain(x, x, torch.zeros(100))
    # the calls on a handle: one whose hop the inverse cannot use, and a short workspace
    lib = L.lib()
    bad = metrics._handle(44100, 2048, 500, 0, x.device)
    y, work = torch.empty_like(x), torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    X = torch.zeros(2, 1025, 11, dtype=torch.complex64, device="cuda")
    assert lib.jat_istft(bad.ptr, L.ptr(X), 2, 5000, L.ptr(y), L.ptr(work), work.numel(), L.stream_ptr()) == L.JAT_E_INVALID
    h = metrics._handle(44100, 2048, 512, 0, x.device)
    a = torch.zeros(1025, device="cuda")
    assert lib.jat_istft(h.ptr, L.ptr(X[:, :, :10]), 2, 5000, L.ptr(y), L.ptr(work), 1000, L.stream_ptr()) == L.JAT_E_STATE
    assert lib.jat_band_splice(h.ptr, L.ptr(x), L.ptr(x), 2, 5000, 5000, L.ptr(a), L.ptr(y), L.ptr(work), 1000,
                               L.stream_ptr()) == L.JAT_E_STATE
    P = torch.empty(2, 1025, dtype=torch.float64, device="cuda")
    assert lib.jat_ltas(h.ptr, L.ptr(x), 2, 5000, L.ptr(P), L.ptr(work), 1000, L.stream_ptr()) == L.JAT_E_STATE
    assert lib.jat_ltas(h.ptr, L.ptr(x), 0, 5000, L.ptr(P), L.ptr(work), work.numel(), L.stream_ptr()) == L.JAT_E_INVALID
    assert lib.jat_band_splice(h.ptr, L.ptr(x), L.ptr(x), 2, 5000, 5000, None, L.ptr(y), L.ptr(work), work.numel(),
                               L.stream_ptr()) == L.JAT_E_INVALID
    torch.cuda.synchronize()


# ---- the fp16-operand library ------------------------------------------------------------------------------------------------
def both_builds_outputs():
    """what the child on libjat_hip_fp16.so and this process both compute: shape (512, 128, 1301), B = 3"""
    n_fft, hop, n = 512, 128, 1301
    f = fixture(n_fft, hop, n)
    out = dict(istft=splice.istft(cuda(f["X"]), n, n_fft, hop),
               splice=splice.splice_gain(cuda(f["g"]), cuda(f["s"]), torch.from_numpy(f["a"].copy()), n_fft, hop),
               ltas=splice.ltas(cuda(f["x"]), n_fft, hop))
    return {k: v.cpu().numpy() for k, v in out.items()}


def test_fp16_library_gives_the_same_bits(tmp_path):
    """splice.hip is fp32 in both builds (csrc/Makefile): libjat_hip_fp16.so, in a child process, computes the bits this process
    computes"""
    code = ("import sys, numpy as np\n"
            "sys.path.insert(0, 'tests')\n"
            "import jatsr_amd._lib as L\n"
            "from test_gpu_splice import both_builds_outputs\n"
            "assert L.operand_dtype() == 'fp16'\n"
            "np.savez(sys.argv[1], **both_builds_outputs())\n")
    env = dict(os.environ, JAT_OPERAND_DTYPE="fp16")
    env.pop("JAT_LIB_PATH", None)
    path = str(tmp_path / "fp16.npz")
    out = subprocess.run([sys.executable, "-c", code, path], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
    got, mine = dict(np.load(path)), both_builds_outputs()
    assert sorted(got) == sorted(mine) == ["istft", "ltas", "splice"]
    for k, v in mine.items():
        assert v.dtype == got[k].dtype and np.isfinite(v).all() and np.abs(v).max() > 0, k
        assert np.array_equal(v, got[k]) and v.tobytes() == got[k].tobytes(), k
    assert mine["istft"].shape == (3, 1301) and mine["splice"].shape == (3, 1338) and mine["ltas"].shape == (3, 257)


# ---- command lines -----------------------------------------------------------------------------------------------------------
def test_splice_cli(tmp_path, capsys):
    s, g = S.band_fixture(n=30000)
    jio.write_wav_float32(tmp_path / "gen.wav", g, 44100)
    jio.write_wav_float32(tmp_path / "low.wav", s[:29000], 44100)
    hz = splice.main(["--generated", str(tmp_path / "gen.wav"), "--source", str(tmp_path / "low.wav"),
                      "--out", str(tmp_path / "gen_lf.wav"), "--cutoff-hz", "4000", "--transition-hz", "500"])
    out, sr = jio.read_wav(tmp_path / "gen_lf.wav")
    assert hz == 4000.0 and sr == 44100 and out.shape == (30000,) and "4000.0 Hz (given)" in capsys.readouterr().out
    want = splice.splice_lowband(cuda(g), cuda(s[:29000]), cutoff_hz=4000.0)[0].cpu().numpy()
    assert np.array_equal(out, want) and np.array_equal(out[29000:], g[29000:])
    # a source at another rate is resampled; the cutoff is detected (a 1 kHz sine: just above 1 kHz)
    from jatsr_amd.resample import resample
    s16 = resample(cuda(s)[None], 44100, 16000)[0].cpu().numpy()
    jio.write_wav_float32(tmp_path / "low16.wav", s16, 16000)
    hz = splice.main(["--generated", str(tmp_path / "gen.wav"), "--source", str(tmp_path / "low16.wav"),
                      "--out", str(tmp_path / "auto.wav")])
    out, _ = jio.read_wav(tmp_path / "auto.wav")
    assert 1000.0 < hz < 8000.0 and out.shape == (30000,) and np.isfinite(out).all()


def _infer_setup(tmp_path):
    cfg = dict(recipe.CONFIGS["micro"], input_channels=1024, cond_channels=1024)
    torch.save({"model_state_dict": {k: torch.from_numpy(v) for k, v in recipe.make_state_dict(cfg).items()},
                "config": dict(cfg)}, tmp_path / "last.pt")
    ones, zeros = [1.0] * 1024, [0.0] * 1024
    (tmp_path / "stats.json").write_text(json.dumps({"hr_mean": zeros, "hr_std": ones, "lr_mean": zeros, "lr_std": ones}))
    full = {"decoder." + k: torch.from_numpy(v) for k, v in recipe.make_dac_state_dict().items()}
    full.update({k: torch.from_numpy(v) for k, v in recipe.make_dac_encoder_state_dict().items()})
    torch.save(full, tmp_path / "dac.pt")
    return ["--checkpoint", str(tmp_path / "last.pt"), "--stats-file", str(tmp_path / "stats.json"), "--steps", "2",
            "--seed", "3", "--dac-weights", str(tmp_path / "dac.pt")]


def _wav(path):
    raw = open(path, "rb").read()
    return np.frombuffer(raw[raw.index(b"data") + 8:], "<f4")


def test_infer_lf_replace(tmp_path):
    from jatsr_amd.infer import main as infer_main
    base = _infer_setup(tmp_path)
    x = recipe.make_dac_audio(1, 3 * 22050, 71, sample_rate=22050)[0, 0]
    jio.write_wav_float32(tmp_path / "song.wav", x, 22050)
    audio = ["--input-audio", str(tmp_path / "song.wav")]
    # --simulate-lr with --metrics: the source is the whole file through the LR simulation
    for name, extra in (("plain", []), ("lf", ["--lf-replace"])):
        infer_main(base + audio + ["--output-dir", str(tmp_path / name), "--simulate-lr", "--metrics"] + extra)
    names = sorted(f for f in os.listdir(tmp_path / "plain"))
    assert sorted(os.listdir(tmp_path / "lf")) == sorted(names + ["song_generated_lf.wav"])
    for f in names:
        if f.endswith(".wav"):
            assert (tmp_path / "plain" / f).read_bytes() == (tmp_path / "lf" / f).read_bytes(), f
    lf, gen = _wav(tmp_path / "lf" / "song_generated_lf.wav"), _wav(tmp_path / "lf" / "song_generated.wav")
    assert lf.shape == gen.shape and gen.size % 512 == 0 and np.isfinite(lf).all() and not np.array_equal(lf, gen)
    rep, plain = (json.load(open(tmp_path / d / "song_metrics.json")) for d in ("lf", "plain"))
    assert set(rep) == set(plain) | {"generated_lf"} and all(rep[k] == plain[k] for k in plain)
    assert set(rep["generated_lf"]) == set(rep["generated"]) and np.isfinite(rep["generated_lf"]["lsd"])
    # --input-audio alone with a given cutoff: the source is the 44.1 kHz waveform that was encoded
    infer_main(base + audio + ["--output-dir", str(tmp_path / "hz"), "--resample", "--lf-replace", "3000",
                               "--lf-transition-hz", "400"])
    from jatsr_amd.resample import resample
    src = resample(cuda(jio.read_wav(tmp_path / "song.wav")[0])[None], 22050, 44100)[0]
    gen = cuda(_wav(tmp_path / "hz" / "song_generated.wav").copy())
    want = splice.splice_lowband(gen, src, cutoff_hz=3000.0, transition_hz=400.0)[0].cpu().numpy()
    assert np.array_equal(_wav(tmp_path / "hz" / "song_generated_lf.wav"), want)
    # a latent file: the source is the decoded LR latent
    z = torch.load(tmp_path / "hz" / "song_generated.pt", weights_only=False)
    jio.save_latent_file(tmp_path / "clip.pt", hr_latent=None, lr_latent=z["lr_latent"])
    infer_main(base + ["--input-file", str(tmp_path / "clip.pt"), "--output-dir", str(tmp_path / "lat"), "--lf-replace"])
    lf, lr = _wav(tmp_path / "lat" / "clip_generated_lf.wav"), _wav(tmp_path / "lat" / "clip_lr_input.wav")
    assert lf.shape == lr.shape == (z["lr_latent"].shape[-1] * 512,) and np.isfinite(lf).all()
    with pytest.raises(SystemExit, match="--lf-replace"):
        infer_main(base[:-2] + ["--input-file", str(tmp_path / "clip.pt"), "--lf-replace"])
    with pytest.raises(SystemExit, match="not a frequency"):
        infer_main(base + ["--input-file", str(tmp_path / "clip.pt"), "--lf-replace", "high"])
