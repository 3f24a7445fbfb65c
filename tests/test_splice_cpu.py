"""Host side of the inverse STFT and the low-band splice (jatsr_amd.splice, csrc/jat_splice.cpp) and their fp64
restatement (tests/splice_ref.py): the restatement against torch.istft, the identities the kernels are built on, the host
entry points of the C ABI, every refusal that needs no device handle, and the fixtures of tests/test_gpu_splice.py.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import metrics_ref as M
import splice_ref as S
import jatsr_amd
import jatsr_amd.splice as splice
from jatsr_amd import _lib as L


@pytest.fixture(scope="module", autouse=True)
def built_lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.lib()


# ---- the restatement -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,hop,n", S.CPU_SHAPES)
def test_restatement_istft_equals_torch_istft(n_fft, hop, n):
    X = S.random_spectrogram(2, n_fft, hop, n, seed=n).astype(np.complex128)
    ours = S.istft(X, n, n_fft, hop)
    ref = torch.istft(torch.from_numpy(X), n_fft, hop, window=torch.hann_window(n_fft, periodic=True, dtype=torch.float64),
                      center=True, length=n).numpy()
    err = np.abs(ours - ref).max()
    print(f"{n_fft}/{hop}/{n}: max-abs {err:.1e}, envelope min {S.envelope_min(n, n_fft, hop):.3f}")
    assert ours.shape == ref.shape == (2, n) and err < 1e-12
    assert S.envelope_min(n, n_fft, hop) > 0.4                     # hop <= n_fft / 4: positive on all of [0, L)


@pytest.mark.parametrize("n_fft,hop,n", S.CPU_SHAPES)
def test_restatement_round_trip(n_fft, hop, n):
    x = S.noise((2, n), seed=n).astype(np.float64)
    assert np.abs(S.istft(M.stft(x, n_fft, hop), n, n_fft, hop) - x).max() < 1e-12


@pytest.mark.parametrize("n_fft,hop,n", S.CPU_SHAPES)
def test_the_two_splice_forms_agree(n_fft, hop, n):
    g, s = S.noise((2, n + 37), seed=n + 1), S.noise((2, n), seed=n + 2)
    a = S.band_gain(44100, n_fft, 6000.0, 1500.0)
    one, two = S.splice(g, s, a, n_fft, hop), S.splice_direct(g, s, a, n_fft, hop)
    assert np.abs(one - two).max() < 1e-12
    assert np.array_equal(one[:, n:], g[:, n:].astype(np.float64))          # past the shorter signal: generated itself


@pytest.mark.parametrize("N", [64, 512, 2048])
def test_two_real_frames_share_one_complex_transform(N):
    rng = np.random.default_rng(N)
    u, v = rng.standard_normal(N), rng.standard_normal(N)
    a = rng.uniform(0, 1, N // 2 + 1)
    full = np.concatenate([a, a[-2:0:-1]])                                  # a[N - k] = a[k]
    z = np.fft.ifft(full * np.fft.fft(u + 1j * v))
    assert np.abs(z.real - np.fft.irfft(a * np.fft.rfft(u), n=N)).max() < 1e-13
    assert np.abs(z.imag - np.fft.irfft(a * np.fft.rfft(v), n=N)).max() < 1e-13
    # the inverse through the forward transform, and the packing of two Hermitian spectra into one
    Z = np.fft.fft(u + 1j * v)
    assert np.abs(np.conj(np.fft.fft(np.conj(Z))) / N - (u + 1j * v)).max() < 1e-13
    Xa, Xb = np.fft.rfft(u), np.fft.rfft(v)
    packed = np.concatenate([Xa + 1j * Xb, (np.conj(Xa) + 1j * np.conj(Xb))[-2:0:-1]])
    assert np.abs(np.fft.ifft(packed) - (u + 1j * v)).max() < 1e-13


# ---- host entry points ---------------------------------------------------------------------------------------------------------
def _ulp_distance(a, b):
    ia, ib = (np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64) for v in (a, b))
    return np.abs(ia - ib).max()


@pytest.mark.parametrize("sr,n_fft,fc,tw", [(44100, 2048, 8000.0, 500.0), (44100, 512, 4000.0, 1234.5), (48000, 1024, 300.0, 500.0),
                                            (44100, 2048, 0.0, 500.0), (44100, 2048, -10.0, 500.0), (44100, 2048, 22550.0, 500.0),
                                            (44100, 2048, 30000.0, 500.0), (16000, 4096, 7999.0, 1.0)])
def test_band_gain_against_the_restatement(sr, n_fft, fc, tw):
    a = splice.band_gain(sr, n_fft, fc, tw).numpy()
    ref = S.band_gain(sr, n_fft, fc, tw)
    assert a.dtype == np.float32 and a.shape == ref.shape == (1 + n_fft // 2,)
    assert _ulp_distance(a, ref) <= 1
    assert a.min() >= 0.0 and a.max() <= 1.0 and np.all(np.diff(a) <= 0)
    if fc <= 0:
        assert not a.any()
    if fc - tw >= sr / 2:
        assert np.all(a == 1.0)


def test_band_gain_refusals():
    for sr, n_fft, fc, tw in [(0, 2048, 8000.0, 500.0), (44100, 1000, 8000.0, 500.0), (44100, 2048, 8000.0, -1.0),
                              (44100, 2048, float("nan"), 500.0), (44100, 2048, 8000.0, float("inf"))]:
        with pytest.raises(ValueError):
            splice.band_gain(sr, n_fft, fc, tw)


def test_workspace_sizes_and_argument_checks():
    lib, need = L.lib(), C.c_size_t()
    assert lib.jat_istft_workspace_bytes(2048, 512, 3, 132300, C.byref(need)) == 0
    assert need.value >= 3 * 259 * 2048 * 4
    assert lib.jat_band_splice_workspace_bytes(2048, 512, 1, 5000, 700, C.byref(need)) == 0
    assert need.value >= 2 * 2048 * 4                                       # cut to the shorter: 2 frames
    bad = [(2048, 500, 1, 5000),        # hop does not divide n_fft
           (2048, 1024, 1, 5000),       # hop > n_fft / 4
           (2048, 512, 0, 5000),        # B = 0
           (2048, 512, 65536, 5000), (2048, 512, 1, 0), (1000, 250, 1, 5000), (4096, 32, 1, 5000), (2048, 512, 1, 2 ** 31)]
    for n_fft, hop, B, n in bad:
        assert lib.jat_istft_workspace_bytes(n_fft, hop, B, n, C.byref(need)) == L.JAT_E_INVALID, (n_fft, hop, B, n)
        assert lib.jat_band_splice_workspace_bytes(n_fft, hop, B, n, 5000, C.byref(need)) == L.JAT_E_INVALID
        assert lib.jat_last_error()
    assert lib.jat_band_splice_workspace_bytes(2048, 512, 1, 5000, 0, C.byref(need)) == L.JAT_E_INVALID
    assert lib.jat_istft_workspace_bytes(2048, 512, 1, 5000, None) == L.JAT_E_INVALID
    # the calls themselves refuse a null handle before they touch anything
    assert lib.jat_istft(None, None, 1, 5000, None, None, 0, None) == L.JAT_E_INVALID
    assert lib.jat_ltas(None, None, 1, 5000, None, None, 0, None) == L.JAT_E_INVALID
    assert lib.jat_band_splice(None, None, None, 1, 5000, 5000, None, None, None, 0, None) == L.JAT_E_INVALID


def test_product_modules_import_without_a_gpu_and_fail_loudly():
    import jatsr_amd.infer as infer
    assert jatsr_amd.splice_lowband is splice.splice_lowband and jatsr_amd.istft is splice.istft
    x = torch.zeros(4096)
    with pytest.raises(L.JatError, match="CUDA"):
        splice.splice_lowband(x, x, cutoff_hz=4000.0)
    with pytest.raises(L.JatError, match="CUDA"):
        splice.ltas(x)
    with pytest.raises(L.JatError, match="CUDA"):
        splice.detect_cutoff(x)
    with pytest.raises(L.JatError, match="CUDA"):
        splice.istft(torch.zeros(1025, 9, dtype=torch.complex64), 4096)
    args = infer.build_parser().parse_args(["--lf-replace"])
    assert args.lf_replace == "auto" and args.lf_transition_hz == 500.0
    assert infer.build_parser().parse_args(["--lf-replace", "7000"]).lf_replace == "7000"
    assert infer.build_parser().parse_args([]).lf_replace is None
    with pytest.raises(SystemExit, match="--lf-replace"):
        infer.run(infer.build_parser().parse_args(["--lf-replace"]))        # needs --dac-weights
    assert splice.build_parser().parse_args(["--generated", "a", "--source", "b", "--out", "c"]).cutoff_hz is None
    assert splice.cutoff_bin(np.zeros(1025)) == 0 and splice.cutoff_bin(np.r_[np.ones(10), np.zeros(1015)]) == 10


# ---- fixtures of the GPU tests -----------------------------------------------------------------------------------------------
def test_cutoff_fixture_keeps_its_margin():
    """every bin within 3 bins of the decision lies at least 3 dB from the threshold, in fp64: the GPU's bin must then be
    the restatement's.  The decision is taken 15 dB down, on the steep flank of the window's main lobe (the two bins at the
    band edge lie near -7.5 and -24 dB).  At the default 60 dB no seed can keep the condition: the leakage of a band edge
    through a Hann window goes as distance^-5, about 2.6 dB per bin where it crosses -60 dB, and the cut-off first and last
    frames of a 2 s signal add a flat skirt near -35 dB, so neighbouring bins never lie 3 dB to either side of the threshold."""
    x = S.cutoff_fixture(rows=3)
    for row in x:
        P = S.ltas(row)
        b, margin = S.cutoff_bin(P, S.CUTOFF_DB), S.cutoff_margin_db(P, S.CUTOFF_DB)
        print(f"bin {b} = {b * 44100 / 2048:.0f} Hz, margin {margin:.2f} dB")
        assert margin >= 3.0
        assert abs(b * 44100 / 2048 - 8000.0) < 5 * 44100 / 2048
        assert S.cutoff_bin(S.ltas(row, dtype=np.float32), S.CUTOFF_DB) == b
    assert S.detect_cutoff(np.zeros(3000, np.float32)) == 0.0


def test_band_fixture_in_the_restatement():
    s, g = S.band_fixture()
    out = S.splice(g, s, S.band_gain(44100, 2048, 4000.0, 500.0))
    k1, k12 = round(1000 * 2048 / 44100), round(12000 * 2048 / 44100)
    O, So, G = (np.abs(M.stft(v)[:, 4:-4]) for v in (out, s, g))
    assert np.abs(O[k1] / So[k1] - 1).max() < 1e-3 and np.abs(O[k12] / G[k12] - 1).max() < 1e-3
