"""The sample-rate converter and the per-channel statistics on the GPU (csrc/resample.hip, jatsr_amd.resample) against
the fp64 restatement of their formula (tests/resample_ref.py): accuracy for every conversion the data preparation and the
inference tool use, edge cases, determinism, the LR simulation, the statistics kernel, the fp16-operand library.

Gates.  The same algorithm run in fp32 on the CPU (torch conv1d) is 0.7-1.1e-7 rel-L2 and 1.6-2.8e-7 max-abs against
fp64 on the accuracy signal; the gate is about 10x that, to allow another summation order over up to 475 taps:
rel-L2 <= 1e-6, max-abs <= 2e-6.  Measured on MI355X: rel-L2 6.6e-8 .. 1.04e-7, max-abs 1.5e-7 .. 2.6e-7 over the seven
conversions (B = 1 and B = 3)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import resample_ref as R  # noqa: E402
import jatsr_amd  # noqa: E402
from jatsr_amd import _lib as L  # noqa: E402
from jatsr_amd.resample import channel_stats, resample, simulate_lr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL_GATE, ABS_GATE = 1e-6, 2e-6
CONVERSIONS = [(44100, 48000), (48000, 44100), (48000, 16000), (16000, 48000), (16000, 44100), (44100, 16000),
               (96000, 44100)]


def signal(B, n, sr, seed=0):
    """rows of different content: two sines plus Gaussian noise"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    return np.stack([0.3 * np.sin(2 * np.pi * (220 + 130 * b) * t) + 0.2 * np.sin(2 * np.pi * (1500 + 410 * b) * t + 0.3)
                     + 0.05 * rng.standard_normal(n) for b in range(B)]).astype(np.float32)


def gpu(x, *args, **kw):
    return resample(torch.from_numpy(np.ascontiguousarray(x)).cuda(), *args, **kw).cpu().numpy()


def errors(y, ref):
    return float(np.linalg.norm(y - ref) / np.linalg.norm(ref)), float(np.abs(y - ref).max())


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("orig,new", CONVERSIONS)
def test_accuracy_against_fp64(orig, new, B):
    x = signal(B, 3 * orig, orig, seed=orig % 97 + B)
    y = gpu(x, orig, new)
    ref = R.resample(x, orig, new)
    assert y.shape == ref.shape == (B, R.out_length(3 * orig, orig, new)) and y.dtype == np.float32
    rel, mx = errors(y.astype(np.float64), ref)
    print(f"{orig} -> {new} B={B}: rel-L2 {rel:.2e} (gate {REL_GATE:.0e}), max-abs {mx:.2e} (gate {ABS_GATE:.0e})")
    assert rel <= REL_GATE and mx <= ABS_GATE


def test_codec_rate_step_parameters():
    # the 48 -> 44.1 kHz step of the data preparation: width 24, rolloff 0.945
    x = signal(2, 3 * 48000, 48000, seed=5)
    y = gpu(x, 48000, 44100, 24, 0.945)
    rel, mx = errors(y.astype(np.float64), R.resample(x, 48000, 44100, 24, 0.945))
    print(f"48000 -> 44100 (24, 0.945): rel-L2 {rel:.2e}, max-abs {mx:.2e}")      # measured: 1.3e-7, 3.6e-7
    assert rel <= REL_GATE and mx <= ABS_GATE


@pytest.mark.parametrize("orig,new", CONVERSIONS + [(8000, 44100), (22050, 44100)])
def test_short_and_ragged_lengths(orig, new):
    o, n, width, K, _ = R.dims(orig, new)
    rng = np.random.default_rng(3)
    for n_in in (1, max(1, width - 2), o, o + 1, 7 * o + 3, 1000):               # L = 1, L < width, L not a multiple of o
        x = rng.standard_normal((2, n_in)).astype(np.float32)
        y = gpu(x, orig, new)
        ref = R.resample(x, orig, new)
        assert y.shape == ref.shape == (2, -(-n * n_in // o)), (n_in, y.shape)
        assert np.abs(y - ref).max() <= 2e-6 * max(1.0, np.abs(ref).max()), n_in
    # leading dimensions are kept
    x = rng.standard_normal((2, 3, 500)).astype(np.float32)
    y = gpu(x, orig, new)
    assert y.shape == (2, 3, -(-n * 500 // o)) and np.array_equal(y[1, 2], gpu(x[1, 2], orig, new))


def test_equal_rates_copy_bit_exactly():
    x = torch.from_numpy(signal(2, 5000, 44100)).cuda()
    y = resample(x, 44100, 44100)
    assert torch.equal(x, y) and y.data_ptr() != x.data_ptr()
    assert torch.equal(resample(x, 48000, 48000, 24, 0.945), x)


@pytest.mark.parametrize("orig,new", [(16000, 44100), (44100, 16000), (48000, 16000), (16000, 48000)])
def test_impulses_at_the_edges(orig, new):
    # an impulse at sample 0 and at sample L - 1 reads the edge taps of every phase
    o, n, width, K, _ = R.dims(orig, new)
    n_in = 4 * o + 5
    x = np.zeros((2, n_in), np.float32)
    x[0, 0] = 1.0
    x[1, -1] = 1.0
    y = gpu(x, orig, new)
    ref = R.resample(x, orig, new)
    assert np.abs(y - ref).max() <= 1.2e-7 * np.abs(ref).max()                   # one product per output: fp32 rounding of h
    h = R.table(orig, new)
    assert np.allclose(y[0, :n], h[:, width], rtol=0, atol=1e-7)                 # frame 0 of an impulse at 0 is tap `width`


def test_ten_minutes_at_96k():
    n_in = 600 * 96000
    g = torch.Generator(device="cuda").manual_seed(7)
    x = 0.1 * torch.randn(1, n_in, device="cuda", generator=g)
    y = resample(x, 96000, 44100)
    assert y.shape == (1, 600 * 44100) and bool(torch.isfinite(y).all())
    rng = np.random.default_rng(8)
    idx = np.unique(np.concatenate([np.arange(64), y.shape[-1] - 1 - np.arange(64), rng.integers(0, y.shape[-1], 3968)]))
    ref = R.resample_at(x[0].cpu().numpy(), 96000, 44100, idx)
    got = y[0, torch.from_numpy(idx).cuda()].cpu().numpy().astype(np.float64)
    mx = np.abs(got - ref).max()
    print(f"10 min 96k -> 44.1k: {len(idx)} spot outputs, max-abs {mx:.2e}")       # measured: 4.6e-8
    assert mx <= ABS_GATE


def test_determinism_and_batch_independence():
    for orig, new in ((16000, 44100), (48000, 16000), (48000, 44100)):
        x = torch.from_numpy(signal(3, 2 * orig + 11, orig, seed=9)).cuda()
        a = resample(x, orig, new)
        b = resample(x, orig, new)
        assert torch.equal(a, b)
        for row in range(3):
            assert torch.equal(a[row], resample(x[row].clone(), orig, new)), (orig, new, row)
        # a row keeps its bits whatever the length of the launch it runs in
        assert torch.equal(a[0, :1000], resample(x[0, :orig].clone(), orig, new)[:1000])


def test_argument_errors():
    x = torch.zeros(2, 100, device="cuda")
    with pytest.raises(L.JatError):
        resample(x.cpu(), 16000, 44100)
    with pytest.raises(L.JatError):
        resample(x.double(), 16000, 44100)
    with pytest.raises(L.JatError):
        resample(x.half(), 16000, 44100)
    for bad in ((0, 44100), (16000, 0), (-1, 44100)):
        with pytest.raises(ValueError):
            resample(x, *bad)
    with pytest.raises(ValueError):
        resample(x, 44101, 44100)                                                  # a table of 2e9 taps
    with pytest.raises(ValueError):
        resample(x, 16000, 44100, lowpass_filter_width=0)
    assert resample(torch.zeros(2, 0, device="cuda"), 16000, 44100).shape == (2, 0)
    assert jatsr_amd.resample(x, 16000, 48000).shape == (2, 300)
    torch.cuda.synchronize()


# ---- LR simulation ----------------------------------------------------------------------------------------------------------------
def test_simulate_lr_against_the_two_stage_restatement():
    x = signal(2, 3 * 48000 + 7, 48000, seed=11)
    y = simulate_lr(torch.from_numpy(x).cuda()).cpu().numpy()
    ref = R.simulate_lr(x)
    assert y.shape == x.shape == ref.shape
    rel, mx = errors(y.astype(np.float64), ref)
    print(f"simulate_lr: rel-L2 {rel:.2e} (gate 2e-6), max-abs {mx:.2e}")          # measured: 1.2e-7, 2.6e-7
    assert rel <= 2e-6
    # the round trip rounds up twice, so it is never shorter than the input: it is cut to the input's length
    assert jatsr_amd.simulate_lr(torch.from_numpy(x).cuda(), 48000, 8000).shape == x.shape
    short = jatsr_amd.simulate_lr(torch.from_numpy(x[:, :1000]).cuda(), 44100, 16000)
    assert short.shape == (2, 1000) and np.allclose(short.cpu().numpy(), R.simulate_lr(x[:, :1000], 44100, 16000), atol=2e-6)


def test_simulate_lr_is_a_low_pass():
    rng = np.random.default_rng(12)
    x = rng.standard_normal(3 * 48000).astype(np.float32) * 0.1
    y = simulate_lr(torch.from_numpy(x).cuda()[None])[0].cpu().numpy().astype(np.float64)
    cut = 4800                                                                    # 0.1 s dropped at each end
    X, Y = (np.abs(np.fft.rfft(v[cut:-cut])) ** 2 for v in (x.astype(np.float64), y))
    f = np.fft.rfftfreq(len(x) - 2 * cut, 1 / 48000)
    hi = 10 * np.log10(Y[f > 10000].sum() / X[f > 10000].sum())
    lo = 10 * np.log10(Y[f < 7000].sum() / X[f < 7000].sum())
    print(f"energy above 10 kHz {hi:.1f} dB, below 7 kHz {lo:+.2f} dB")           # the fp64 formula: -56.3 dB, -0.17 dB
    assert hi <= -40.0 and abs(lo) < 0.5


# ---- per-channel statistics -------------------------------------------------------------------------------------------------------
def _stats_ref(z):
    v = z.astype(np.float16).astype(np.float64)
    return v.sum(axis=(0, 2)), (v * v).sum(axis=(0, 2)), np.abs(v).sum(axis=(0, 2))


@pytest.mark.parametrize("T", [603, 1])
def test_channel_stats_against_numpy(T):
    """fp64 sums of the fp16-rounded values.  The GPU and numpy add the same fp64 numbers in another order; the error of a
    reordered sum of N terms is below N 2^-53 sum|v| (N = B T = 1206: 1.3e-13), so the gate is 1e-12 relative to sum|v|
    (for the squares sum|v| is the sum itself).  Measured: 0 (sum) and 1.8e-16 (squares)."""
    rng = np.random.default_rng(13)
    z = (3.0 * rng.standard_normal((2, 1024, T)) + rng.standard_normal((1, 1024, 1))).astype(np.float32)
    s, q = channel_stats(torch.from_numpy(z).cuda())
    assert s.dtype == q.dtype == torch.float64 and s.shape == q.shape == (1024,)
    rs, rq, ra = _stats_ref(z)
    es = float((np.abs(s.cpu().numpy() - rs) / ra).max())
    eq = float((np.abs(q.cpu().numpy() - rq) / rq).max())
    print(f"T={T}: sum {es:.2e}, sq_sum {eq:.2e} (gate 1e-12)")
    assert es <= 1e-12 and eq <= 1e-12
    s2, q2 = channel_stats(torch.from_numpy(z).cuda())
    assert torch.equal(s, s2) and torch.equal(q, q2)                              # no atomics: the same bits
    # two calls into the same totals = one call on the concatenation
    a, b = torch.from_numpy(z[:1]).cuda(), torch.from_numpy(z[1:]).cuda()
    sa, qa = channel_stats(a)
    channel_stats(b, sa, qa)
    assert float((np.abs(sa.cpu().numpy() - rs) / ra).max()) <= 1e-12
    assert float((np.abs(qa.cpu().numpy() - rq) / rq).max()) <= 1e-12
    # [C, T] input; fp16 rounding is part of the definition
    s1, _ = channel_stats(torch.from_numpy(z[0]).cuda())
    assert float((np.abs(s1.cpu().numpy() - _stats_ref(z[:1])[0]) / ra).max()) <= 1e-12
    big = torch.full((1, 4, 8), 1.0 + 2.0 ** -12, device="cuda")                  # rounds to 1 in fp16
    assert channel_stats(big)[0].tolist() == [8.0] * 4
    with pytest.raises(L.JatError):
        channel_stats(torch.zeros(2, 4, 8))
    with pytest.raises(L.JatError):
        channel_stats(big, torch.zeros(4, device="cuda"))                         # totals must be fp64


# ---- the fp16-operand library -------------------------------------------------------------------------------------------------------
def test_fp16_library_gives_the_same_bits(tmp_path):
    code = ("import sys, numpy as np, torch\n"
            "sys.path.insert(0, 'tests')\n"
            "import jatsr_amd._lib as L\n"
            "from jatsr_amd.resample import resample\n"
            "from test_gpu_resample import signal\n"
            "assert L.operand_dtype() == sys.argv[2]\n"
            "out = {}\n"
            "for orig, new in ((16000, 44100), (48000, 16000), (47952, 44100)):    # the last: two phase slices\n"
            "    out[f'{orig}_{new}'] = resample(torch.from_numpy(signal(2, orig + 13, orig, 21)).cuda(), orig, new).cpu().numpy()\n"
            "np.savez(sys.argv[1], **out)\n")
    got = {}
    for dtype in ("bf16", "fp16"):
        env = dict(os.environ, JAT_OPERAND_DTYPE=dtype)
        env.pop("JAT_LIB_PATH", None)
        path = str(tmp_path / f"{dtype}.npz")
        out = subprocess.run([sys.executable, "-c", code, path, dtype], cwd=ROOT, env=env, capture_output=True, text=True,
                             timeout=600)
        assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
        got[dtype] = dict(np.load(path))
    assert sorted(got["bf16"]) == sorted(got["fp16"]) and len(got["bf16"]) == 3
    for k, v in got["bf16"].items():
        assert v.tobytes() == got["fp16"][k].tobytes(), k
        orig, new = map(int, k.split("_"))
        assert np.abs(v - R.resample(signal(2, orig + 13, orig, 21), orig, new)).max() <= ABS_GATE
