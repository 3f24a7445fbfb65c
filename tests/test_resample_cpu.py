"""Host side of the sample-rate converter and of the data preparation (no GPU): the fp64 restatement checks itself
(tests/resample_ref.py), `jat_resample_table` against it, argument validation, the chunk bounds against a literal
restatement of the reference loop, the command lines."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import jatsr_amd._lib as L
import resample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (orig, new) -> (o, n, K): the shapes the kernel has to handle well
SHAPES = {(44100, 48000): (147, 160, 161), (48000, 44100): (160, 147, 174), (48000, 16000): (3, 1, 41),
          (16000, 48000): (1, 3, 15), (16000, 44100): (160, 441, 174), (44100, 16000): (441, 160, 475),
          (96000, 44100): (320, 147, 348)}
EXTRA = [(8000, 44100), (22050, 44100)]


@pytest.fixture(scope="session")
def built_lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.lib()


# ---- the restatement checks itself ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", sorted(SHAPES))
def test_ref_table_shapes(pair):
    o, n, width, K, _ = R.dims(*pair)
    assert (o, n, K) == SHAPES[pair] and K == 2 * width + o
    assert R.table(*pair).shape == (n, K)


@pytest.mark.parametrize("orig,new,lpw,rolloff", [(16000, 44100, 6, 0.99), (48000, 16000, 6, 0.99), (44100, 48000, 6, 0.99),
                                                  (16000, 48000, 6, 0.99), (48000, 44100, 24, 0.945)])
def test_ref_constant_stays_constant(orig, new, lpw, rolloff):
    y = R.resample(np.ones(4 * orig // 10), orig, new, lpw, rolloff)
    m = len(y) // 4
    err = np.abs(y[m:-m] - 1).max()
    print(f"{orig}->{new} lpw {lpw}: constant deviates by {err:.2e}")
    assert err < 2e-3          # the window's ripple: 4.7e-4 .. 8.8e-4 for the defaults, 9e-6 for width 24 / rolloff 0.945


def test_ref_sine_matches_the_analytic_sine():
    t = np.arange(16000) / 16000
    y = R.resample(np.sin(2 * np.pi * 1000 * t), 16000, 44100)
    to = np.arange(len(y)) / 44100
    err = np.abs(y - np.sin(2 * np.pi * 1000 * to))[2000:-2000].max()
    print(f"1 kHz sine 16k -> 44.1k: {err:.2e}")
    assert err < 1e-3          # 6.9e-4


def test_ref_lengths_and_spot_values():
    rng = np.random.default_rng(1)
    for (orig, new), (o, n, _) in SHAPES.items():
        for L_in in (1, 5, o, o + 1, 1000, 4099):
            x = rng.standard_normal(L_in)
            y = R.resample(x, orig, new)
            assert y.shape == (-(-n * L_in // o),) == (R.out_length(L_in, orig, new),)
            idx = sorted({0, len(y) // 2, len(y) - 1})
            assert np.allclose(R.resample_at(x, orig, new, idx), y[idx], rtol=0, atol=1e-13)
    assert np.array_equal(R.resample(np.arange(7.0), 44100, 44100), np.arange(7.0))


def test_ref_matches_a_convolution():
    # an integer ratio is one plain FIR: 48k -> 16k is np.convolve with the reversed taps, every third output
    rng = np.random.default_rng(2)
    x = rng.standard_normal(3000)
    o, n, width, K, _ = R.dims(48000, 16000)
    full = np.convolve(np.concatenate([np.zeros(width), x, np.zeros(width + o)]), R.table(48000, 16000)[0][::-1], "valid")
    y = R.resample(x, 48000, 16000)
    assert np.allclose(full[::o][:len(y)], y, rtol=0, atol=1e-13)


# ---- jat_resample_table -------------------------------------------------------------------------------------------------------
def _table(lib, orig, new, lpw=6, rolloff=0.99, with_table=True):
    d = [C.c_int32() for _ in range(4)]
    rc = lib.jat_resample_table(orig, new, lpw, rolloff, None, *(C.byref(v) for v in d))
    if rc != 0:
        return rc, None, None
    o, n, width, K = (v.value for v in d)
    h = np.full((n, K), np.nan, np.float32)
    if with_table:
        assert lib.jat_resample_table(orig, new, lpw, rolloff, h.ctypes.data, *(C.byref(v) for v in d)) == 0
    return 0, (o, n, width, K), h


@pytest.mark.parametrize("orig,new,lpw,rolloff", [p + (6, 0.99) for p in sorted(SHAPES) + EXTRA] + [(48000, 44100, 24, 0.945)])
def test_table_matches_the_fp64_restatement(built_lib, orig, new, lpw, rolloff):
    rc, dims, h = _table(built_lib, orig, new, lpw, rolloff)
    assert rc == 0 and dims == R.dims(orig, new, lpw, rolloff)[:4]
    if (orig, new) in SHAPES and lpw == 6:
        assert (dims[0], dims[1], dims[3]) == SHAPES[(orig, new)]
    ref = R.table(orig, new, lpw, rolloff)
    err = np.abs(h.astype(np.float64) - ref.astype(np.float32).astype(np.float64)).max()
    print(f"{orig}->{new}: table {h.shape}, max |h - fp32(ref)| = {err:.2e}, max |h| = {np.abs(ref).max():.3f}")
    # libm and numpy may differ in the last fp64 bit, which can move an fp32 rounding: one fp32 ulp of max |h|
    assert err <= 1.2e-7 * np.abs(ref).max()


def test_table_argument_validation(built_lib):
    for args in ((0, 44100, 6, 0.99), (44100, 0, 6, 0.99), (-16000, 44100, 6, 0.99), (16000, -1, 6, 0.99),
                 (16000, 44100, 0, 0.99), (16000, 44100, -3, 0.99), (16000, 44100, 6, 0.0), (16000, 44100, 6, -0.5),
                 (16000, 44100, 6, 1.01), (16000, 44100, 6, float("nan")), (44101, 44100, 6, 0.99)):
        rc, _, _ = _table(built_lib, *args)
        assert rc == L.JAT_E_INVALID, args
        assert built_lib.jat_last_error()
    d = [C.c_int32() for _ in range(4)]
    for missing in range(4):
        ptrs = [None if i == missing else C.byref(v) for i, v in enumerate(d)]
        assert built_lib.jat_resample_table(16000, 44100, 6, 0.99, None, *ptrs) == L.JAT_E_INVALID
    assert _table(built_lib, 16000, 44100, 6, 1.0)[0] == 0                       # rolloff 1 is allowed
    assert built_lib.jat_resampler_create(16000, 44100, 6, 0.99, None, None) == L.JAT_E_INVALID
    out = C.c_int64()
    assert built_lib.jat_resample_out_length(None, 10, C.byref(out)) == L.JAT_E_INVALID
    assert built_lib.jat_resample(None, None, None, 1, 10, None) == L.JAT_E_INVALID
    assert built_lib.jat_channel_stats(None, 1, 1, 1, None, None, None, 0, None) == L.JAT_E_INVALID
    built_lib.jat_resampler_destroy(None)


def test_python_wrappers_validate_on_the_host(built_lib):
    import torch
    from jatsr_amd.resample import resample, sinc_table
    for bad in ((0, 44100), (44100, -1), (16000.5, 44100)):
        with pytest.raises(ValueError):
            resample(torch.zeros(8), *bad)
    with pytest.raises(ValueError):
        resample(torch.zeros(8), 16000, 44100, lowpass_filter_width=0)
    with pytest.raises(ValueError):
        resample(torch.zeros(8), 16000, 44100, rolloff=1.5)
    with pytest.raises(L.JatError, match="CUDA"):
        resample(torch.zeros(8), 16000, 44100)                                     # there is no CPU path
    h, o, n, width, K = sinc_table(48000, 16000)
    assert h.shape == (1, 41) and (o, n, width, K) == (3, 1, 19, 41)
    import jatsr_amd
    assert callable(jatsr_amd.resample) and callable(jatsr_amd.simulate_lr) and callable(jatsr_amd.prepare_audio)
    with pytest.raises(L.JatError, match="CUDA"):
        jatsr_amd.resample(torch.zeros(8), 16000, 44100)                           # the package attribute resamples too


# ---- chunk bounds ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr", [16000, 44100, 48000])
@pytest.mark.parametrize("seconds", [0.99, 1.0, 7.0, 7.01, 61.3])
def test_chunk_bounds_match_the_reference_loop(sr, seconds):
    from jatsr_amd.prepare import chunk_bounds
    total = int(round(seconds * sr))
    got = chunk_bounds(total, sr)
    assert got == R.chunk_bounds(total, sr)
    if seconds < 1.0:
        assert got == []
        return
    assert len(got) == int(np.ceil(total / sr / 7.0))
    assert got[0][0] == 0 and got[0][2] == int(0.5 * sr)                         # the first chunk is padded on the left
    for a, b, pl, pr in got:
        assert 0 <= a < b <= total and pl >= 0 and pr >= 0
        assert (b - a) + pl + pr == 8 * sr                                         # 7 s valid + 0.5 s a side


# ---- command lines ----------------------------------------------------------------------------------------------------------------
def test_infer_parser_has_the_new_flags():
    from jatsr_amd.infer import build_parser
    p = build_parser()
    a = p.parse_args([])
    assert a.resample is False and a.simulate_lr is None
    assert p.parse_args(["--resample"]).resample is True
    assert p.parse_args(["--simulate-lr"]).simulate_lr == 16000
    assert p.parse_args(["--simulate-lr", "8000"]).simulate_lr == 8000


def test_prepare_cli_help_runs_without_a_gpu():
    out = subprocess.run([sys.executable, "-m", "jatsr_amd.prepare", "--help"], cwd=ROOT, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr[-1000:]
    for flag in ("--source-dir", "--output-dir", "--dac-weights", "--val-fraction", "--seed", "--low-sr", "--dac-precision"):
        assert flag in out.stdout
    from jatsr_amd.prepare import build_parser
    a = build_parser().parse_args(["--source-dir", "a", "--source-dir", "b", "--output-dir", "o", "--dac-weights", "w"])
    assert a.source_dir == ["a", "b"] and a.low_sr == 16000 and a.dac_precision == "bf16x3"
