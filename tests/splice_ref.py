"""numpy restatement of the inverse STFT, the long-term average spectrum, the cutoff detection, the band gain and the
low-band splice of jatsr_amd.splice, written from their definitions (include/jat_hip.h), on the conventions of
tests/metrics_ref.py (periodic Hann w, center=True with n_fft / 2 zeros a side, frames = 1 + L // hop):

    istft   y_pad[f hop + i] += w[i] irfft(X[:, f])[i],  env[f hop + i] += w[i]^2,  y[t] = y_pad[t + n_fft/2] / env[t + n_fft/2]
    ltas    P[k] = mean_f |X[k, f]|^2
    cutoff  bin = 1 + max{k : P[k] >= max(P) 10^(-threshold_db / 10)},  hz = bin sr / n_fft;  silence gives 0
    gain    a[k] = 1 for f_k <= fc - tw, 0 for f_k >= fc, 0.5 + 0.5 cos(pi (f_k - (fc - tw)) / tw) between,  f_k = k sr / n_fft
    splice  out = g + istft(a stft(s - g)) on [0, n), n = min(len g, len s);  out = g from n on

Every transform takes `dtype`: np.float64 is the oracle, np.float32 the yardstick (numpy's pocketfft keeps single
precision).  Test infrastructure only."""
import numpy as np

from metrics_ref import hann, n_frames, stft

# (n_fft, hop, L): 259 frames (odd, several blocks, L no multiple of hop); frames side by side in a block; 3 frames; a single
# frame with L < n_fft / 2; 8-fold overlap; the smallest input
GPU_SHAPES = ((2048, 512, 132300), (512, 128, 1301), (1024, 256, 700), (2048, 512, 300), (2048, 256, 4097), (512, 128, 1))
CPU_SHAPES = ((2048, 512, 5000), (512, 128, 1301), (1024, 256, 700), (2048, 512, 300), (2048, 256, 4097), (512, 128, 1))


def istft(X, length, n_fft=2048, hop=512, dtype=np.float64):
    """X complex [..., bins, frames] -> y [..., length]"""
    cd = np.complex64 if dtype == np.float32 else np.complex128
    X = np.asarray(X).astype(cd)
    F = X.shape[-1]
    assert F == n_frames(length, hop) and X.shape[-2] == 1 + n_fft // 2
    w = hann(n_fft, dtype)
    fr = np.fft.irfft(np.swapaxes(X, -1, -2), n=n_fft, axis=-1)        # [..., F, n_fft]
    assert fr.dtype == dtype
    fr = fr * w
    y = np.zeros(X.shape[:-2] + (n_fft + (F - 1) * hop,), dtype)
    env = np.zeros(n_fft + (F - 1) * hop, dtype)
    for f in range(F):                                                   # ascending frame order
        y[..., f * hop:f * hop + n_fft] += fr[..., f, :]
        env[f * hop:f * hop + n_fft] += w * w
    h = n_fft // 2
    return y[..., h:h + length] / env[h:h + length]


def envelope_min(length, n_fft, hop):
    F = n_frames(length, hop)
    w = hann(n_fft)
    env = np.zeros(n_fft + (F - 1) * hop)
    for f in range(F):
        env[f * hop:f * hop + n_fft] += w * w
    return float(env[n_fft // 2:n_fft // 2 + length].min())


def ltas(x, n_fft=2048, hop=512, dtype=np.float64):
    """x [..., L] -> P fp64 [..., bins]: the transform in `dtype`, the powers and their mean in fp64"""
    X = stft(x, n_fft, hop, dtype)
    return np.mean(X.real.astype(np.float64) ** 2 + X.imag.astype(np.float64) ** 2, axis=-1)


def cutoff_bin(P, threshold_db=60.0):
    """P [bins] -> 1 + the last bin at or above max(P) 10^(-threshold_db / 10); 0 for silence"""
    P = np.asarray(P, np.float64)
    top = P.max()
    if not top > 0:
        return 0
    return 1 + int(np.nonzero(P >= top * 10.0 ** (-threshold_db / 10.0))[0].max())


def detect_cutoff(x, sr=44100, threshold_db=60.0, n_fft=2048, hop=512, dtype=np.float64):
    return cutoff_bin(ltas(x, n_fft, hop, dtype), threshold_db) * sr / n_fft


def band_gain(sr, n_fft, cutoff_hz, transition_hz):
    """-> fp32 [bins], computed in fp64"""
    f = np.arange(1 + n_fft // 2, dtype=np.float64) * sr / n_fft
    lo = cutoff_hz - transition_hz
    with np.errstate(divide="ignore", invalid="ignore"):
        mid = 0.5 + 0.5 * np.cos(np.pi * (f - lo) / transition_hz)
    return np.where(f >= cutoff_hz, 0.0, np.where(f <= lo, 1.0, mid)).astype(np.float32)


def splice(g, s, a, n_fft=2048, hop=512, dtype=np.float64):
    """out = g + istft(a stft(s - g)) on the common length, g beyond it"""
    g, s = np.asarray(g, dtype=dtype), np.asarray(s, dtype=dtype)
    n = min(g.shape[-1], s.shape[-1])
    D = stft(s[..., :n] - g[..., :n], n_fft, hop, dtype) * np.asarray(a, dtype)[:, None]
    out = g.copy()
    out[..., :n] += istft(D, n, n_fft, hop, dtype)
    return out


def splice_direct(g, s, a, n_fft=2048, hop=512):
    """the other form, fp64: istft(a S + (1 - a) G) on the common length"""
    g, s = np.asarray(g, np.float64), np.asarray(s, np.float64)
    n = min(g.shape[-1], s.shape[-1])
    a = np.asarray(a, np.float64)[:, None]
    out = g.copy()
    out[..., :n] = istft(a * stft(s[..., :n], n_fft, hop) + (1 - a) * stft(g[..., :n], n_fft, hop), n, n_fft, hop)
    return out


def rel_l2(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300))


def max_over_peak(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


def noise(shape, seed, scale=0.3):
    return (scale * np.random.default_rng(seed).standard_normal(shape)).astype(np.float32)


def random_spectrogram(B, n_fft, hop, L, seed):
    """complex64 [B, bins, frames] of unit-variance parts, DC and Nyquist with imaginary parts too (they are ignored)"""
    rng = np.random.default_rng(seed)
    shape = (B, 1 + n_fft // 2, n_frames(L, hop))
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


CUTOFF_SEED = 7
CUTOFF_DB = 15.0            # the threshold of the detection fixture: see test_cutoff_fixture_keeps_its_margin


def cutoff_fixture(n=88200, sr=44100, seed=CUTOFF_SEED, rows=1):
    """white noise brick-walled at 8 kHz in the FFT domain plus a -90 dB noise floor, float32 [rows, n]"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, n))
    X = np.fft.rfft(x, axis=-1)
    X[..., np.fft.rfftfreq(n, 1.0 / sr) > 8000.0] = 0
    y = np.fft.irfft(X, n=n, axis=-1)
    y = 0.25 * y / np.sqrt(np.mean(y ** 2))
    floor = 0.25 * 10.0 ** (-90.0 / 20.0)
    return (y + floor * rng.standard_normal((rows, n))).astype(np.float32)


def cutoff_margin_db(P, threshold_db=60.0, reach=3):
    """smallest distance in dB from the threshold of the bins within `reach` bins of the decision"""
    P = np.asarray(P, np.float64)
    b = cutoff_bin(P, threshold_db)
    thr = P.max() * 10.0 ** (-threshold_db / 10.0)
    near = P[max(0, b - 1 - reach):b + reach]
    return float(np.abs(10.0 * np.log10(np.maximum(near, 1e-300) / thr)).min())


def band_fixture(n=44100, sr=44100):
    """(source, generated): a 1 kHz sine; a phase-shifted 1 kHz sine at 0.8 amplitude plus a 12 kHz sine"""
    t = np.arange(n) / sr
    s = 0.5 * np.sin(2 * np.pi * 1000.0 * t)
    g = 0.8 * 0.5 * np.sin(2 * np.pi * 1000.0 * t + 0.4) + 0.2 * np.sin(2 * np.pi * 12000.0 * t)
    return s.astype(np.float32), g.astype(np.float32)
