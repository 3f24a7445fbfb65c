"""IIR low-pass families for the low-resolution simulation (C ABI: include/jat_hip_iir.h).

Host side, numpy only: Butterworth and Chebyshev-I designs as second-order sections (`design_sos`), scipy's `sosfilt_zi`
(`sos_zi`), the tables the kernel needs (`pad_sos`, `transition_powers`) and the per-recording draw (`random_filter`).
GPU side: `LowpassBank`, `sosfilt`, `sosfiltfilt` (scipy's, default padding) and `simulate_lr_filtered`, computed by
csrc/iir.hip.  There is no CPU path for the filtering and no scipy import.

    sos = design_sos("cheby1", 8, 4000.0, 48000)                    # float64 [4, 6]
    lr = sosfiltfilt(hr, sos)                                       # hr fp32 CUDA [..., n], zero phase: LR stays aligned with HR
    lr = simulate_lr_filtered(hr, 48000, {"kind": "butter", "order": 6, "cutoff_hz": 6000.0})
    python -m jatsr_amd.lowpass --in a.wav --out b.wav --kind cheby1 --order 8 --cutoff-hz 4000
"""
from __future__ import annotations

import argparse
import ctypes as C
import math

import numpy as np

from . import _lib as L
from ._lib import JatError

KINDS = ("butter", "cheby1")
MAX_ORDER = 10
SECTIONS = 5                   # JAT_IIR_SECTIONS
STATE = 2 * SECTIONS
POWERS = 9                     # JAT_IIR_POWERS
LANE_BLOCK, TILE = 32, 8192    # jat_iir_geometry (checked against the library when a bank is made)
MAX_RIPPLE_DB = 3.0
_M64 = (1 << 64) - 1


# ---- design ---------------------------------------------------------------------------------------------------------------------
def check_filter(kind, order, cutoff_hz, sr, ripple_db=1.0):
    """The limits of `design_sos`; raises JatError naming the limit."""
    if kind not in KINDS:
        raise JatError(f"lowpass: kind must be one of {KINDS}, got {kind!r}")
    if int(order) != order or not 1 <= order <= MAX_ORDER:
        raise JatError(f"lowpass: order {order!r} outside 1..{MAX_ORDER}")
    if not sr > 0:
        raise JatError(f"lowpass: sample rate {sr!r} must be positive")
    lo, hi = sr / 48.0, 0.49 * sr
    if not lo <= cutoff_hz <= hi:                                       # a NaN is outside
        raise JatError(f"lowpass: cutoff {cutoff_hz!r} Hz outside [sr / 48, 0.49 sr] = [{lo:g}, {hi:g}] Hz "
                       f"(below it the fp32 cascade loses accuracy)")
    if not 0.0 < ripple_db <= MAX_RIPPLE_DB:
        raise JatError(f"lowpass: ripple {ripple_db!r} dB outside (0, {MAX_RIPPLE_DB:g}]")


def design_sos(kind, order, cutoff_hz, sr, ripple_db=1.0):
    """-> float64 [ceil(order / 2), 6], scipy's sos layout (b0 b1 b2 1 a1 a2): the analog prototype's poles in closed form,
    pre-warped, through the bilinear transform.  An odd order has one first-order section; the pole pair nearest the unit
    circle comes last; the whole gain sits in the first section (Butterworth: DC gain 1; Chebyshev: passband maximum 1)."""
    check_filter(kind, order, cutoff_hz, sr, ripple_db)
    N = int(order)
    theta = np.pi * np.arange(-N + 1, N, 2) / (2 * N)
    if kind == "butter":
        p = -np.exp(1j * theta)
        k = 1.0
    else:
        eps = math.sqrt(10.0 ** (0.1 * ripple_db) - 1.0)
        mu = math.asinh(1.0 / eps) / N
        p = -np.sinh(mu + 1j * theta)
        k = float(np.prod(-p).real)
        if N % 2 == 0:
            k /= math.sqrt(1.0 + eps * eps)
    warped = 4.0 * math.tan(np.pi * (cutoff_hz / (0.5 * sr)) / 2.0)      # fs = 2, as scipy normalises
    p = p * warped
    k *= warped ** N
    k /= float(np.prod(4.0 - p).real)                                   # N zeros at infinity -> z = -1
    pz = (4.0 + p) / (4.0 - p)
    upper = sorted((q for q in pz if q.imag > 1e-14 * abs(q)), key=abs)
    real = [q.real for q in pz if abs(q.imag) <= 1e-14 * abs(q)]
    assert 2 * len(upper) + len(real) == N and len(real) == N % 2
    sections = [(abs(q), [1.0, 2.0, 1.0, 1.0, -2.0 * q.real, q.real * q.real + q.imag * q.imag]) for q in upper]
    sections += [(abs(r), [1.0, 1.0, 0.0, 1.0, -r, 0.0]) for r in real]
    sos = np.array([s for _, s in sorted(sections, key=lambda t: t[0])], np.float64)
    sos[0, :3] *= k
    return sos


def sos_zi(sos):
    """scipy.signal.sosfilt_zi: the state of the direct-form-II-transposed cascade that holds a unit step steady; [S, 2]."""
    sos = np.asarray(sos, np.float64)
    zi = np.zeros((sos.shape[0], 2))
    scale = 1.0
    for k, (b0, b1, b2, _, a1, a2) in enumerate(sos):
        B0, B1 = b1 - a1 * b0, b2 - a2 * b0
        z0 = (B0 + B1) / (1.0 + a1 + a2)
        zi[k] = scale * np.array([z0, (1.0 + a1) * z0 - B0])
        scale *= (b0 + b1 + b2) / (1.0 + a1 + a2)
    return zi


def dc_gain(sos):
    sos = np.asarray(sos, np.float64)
    return float(np.prod(sos[:, :3].sum(axis=1) / sos[:, 3:].sum(axis=1)))


def pad_sos(sos):
    """[S, 6], S <= 5 -> [5, 6] with identity sections (1 0 0 1 0 0) behind the filter's own."""
    sos = np.asarray(sos, np.float64)
    if sos.ndim != 2 or sos.shape[1] != 6 or not 0 <= sos.shape[0] <= SECTIONS:
        raise JatError(f"lowpass: sos must be [S, 6] with S <= {SECTIONS}, got {sos.shape}")
    if sos.shape[0] and not (sos[:, 3] == 1.0).all():
        raise JatError("lowpass: every section needs a0 = 1")
    out = np.tile(np.array([1.0, 0, 0, 1.0, 0, 0]), (SECTIONS, 1))
    out[:sos.shape[0]] = sos
    return out


def own_sections(sos5):
    """number of sections up to the last that is not an identity"""
    ident = np.array([1.0, 0, 0, 1.0, 0, 0])
    keep = [k for k in range(len(sos5)) if not np.array_equal(sos5[k], ident)]
    return keep[-1] + 1 if keep else 0


def padlen(sos):
    """scipy's default padlen of sosfiltfilt, from the filter's own sections"""
    sos = np.asarray(sos, np.float64)
    S = own_sections(sos)
    return 3 * (2 * S + 1 - min(int((sos[:S, 2] == 0).sum()), int((sos[:S, 5] == 0).sum())))


def transition_matrix(sos5):
    """The zero-input transition of the whole padded cascade in its state coordinates (s1, s2 per section), fp64 [10, 10]: the
    zero-input recurrence run on unit vectors."""
    A = np.zeros((STATE, STATE))
    for c in range(STATE):
        s = np.zeros(STATE)
        s[c] = 1.0
        x = 0.0
        for k, (b0, b1, b2, _, a1, a2) in enumerate(sos5):
            y = b0 * x + s[2 * k]
            s[2 * k] = (b1 * x - a1 * y) + s[2 * k + 1]
            s[2 * k + 1] = b2 * x - a2 * y
            x = y
        A[:, c] = s
    return A


def transition_powers(sos5, lane_block=LANE_BLOCK, count=POWERS):
    """fp64 [count, 10, 10]: P^(2^k) for k < count, with P = A^lane_block (the last, at 32 and 9, is A^8192)."""
    assert lane_block & (lane_block - 1) == 0
    P = transition_matrix(sos5)
    for _ in range(lane_block.bit_length() - 1):
        P = P @ P
    out = [P]
    for _ in range(count - 1):
        out.append(out[-1] @ out[-1])
    return np.stack(out)


# ---- the draw ---------------------------------------------------------------------------------------------------------------------
def _splitmix64(x):
    from .data import _splitmix64 as f
    return f(x)


def _draws(seed, name, n):
    h = _splitmix64(int(seed) & _M64)
    data = str(name).encode("utf-8")
    for i in range(0, len(data), 8):
        h = _splitmix64(h ^ int.from_bytes(data[i:i + 8], "little"))
    h = _splitmix64(h ^ len(data))
    out = []
    for _ in range(n):
        h = _splitmix64(h)
        out.append((h >> 11) / float(1 << 53))
    return out


def random_filter(seed, name, kinds=KINDS, cutoff_hz=(2000.0, 12000.0), order=(2, 10), ripple_db=1.0):
    """The filter of one recording, a function of (seed, name) alone: kind uniform over `kinds` (which may hold "sinc", the
    windowed-sinc round trip, drawn with nothing else), cutoff log-uniform on [lo, hi], order uniform on lo..hi.
    -> {"kind", "order", "cutoff_hz", "ripple_db"} (or {"kind": "sinc"})."""
    kinds = tuple(kinds)
    if not kinds or any(k not in KINDS + ("sinc",) for k in kinds):
        raise JatError(f"lowpass: kinds must come from {KINDS + ('sinc',)}, got {kinds!r}")
    (clo, chi), (olo, ohi) = cutoff_hz, order
    if not 0 < clo <= chi:
        raise JatError(f"lowpass: cutoff range {cutoff_hz!r} must be 0 < lo <= hi")
    if int(olo) != olo or int(ohi) != ohi or not 1 <= olo <= ohi <= MAX_ORDER:
        raise JatError(f"lowpass: order range {order!r} must lie in 1..{MAX_ORDER} with lo <= hi")
    u = _draws(seed, name, 3)
    kind = kinds[min(int(u[0] * len(kinds)), len(kinds) - 1)]
    if kind == "sinc":
        return {"kind": "sinc"}
    cut = float(clo * math.exp(u[1] * math.log(chi / clo)))
    n = int(olo) + min(int(u[2] * (int(ohi) - int(olo) + 1)), int(ohi) - int(olo))
    return {"kind": kind, "order": n, "cutoff_hz": min(max(cut, float(clo)), float(chi)), "ripple_db": float(ripple_db)}


def filter_sos(filt, sr):
    """{"kind", "order", "cutoff_hz"[, "ripple_db"]} -> design_sos at `sr`"""
    return design_sos(filt["kind"], filt["order"], filt["cutoff_hz"], sr, filt.get("ripple_db", 1.0))


# ---- the GPU ------------------------------------------------------------------------------------------------------------------------
class LowpassBank:
    """A table of R filters on the device: `filters` is a list of sos arrays [S <= 5, 6] (float64).  `padlen` is the largest
    padlen of the table, and `sosfiltfilt` refuses `n <= padlen` for every row, whichever filter the row names (the device
    reads the row's filter and cannot refuse): a bank that mixes a long and a short cascade refuses lengths scipy would take
    for the short one alone.  Give such rows a bank of their own."""

    def __init__(self, filters, device="cuda"):
        import torch
        L.require_gpu()
        if isinstance(filters, np.ndarray) and filters.ndim == 2:
            filters = [filters]
        self.sos = np.stack([pad_sos(f) for f in filters])
        self.R = self.sos.shape[0]
        self.zi = np.zeros((self.R, SECTIONS, 2))
        for r in range(self.R):
            S = own_sections(self.sos[r])
            self.zi[r, :S] = sos_zi(self.sos[r, :S])
        lb, tile = C.c_int32(), C.c_int32()
        L.check(L.lib().jat_iir_geometry(C.byref(lb), C.byref(tile)))
        if (lb.value, tile.value) != (LANE_BLOCK, TILE):
            raise JatError(f"lowpass: the library blocks by {lb.value} / {tile.value}, this module by {LANE_BLOCK} / {TILE}")
        self.powers = np.stack([transition_powers(s) for s in self.sos])
        self.device = torch.device(device if str(device) != "cuda" else f"cuda:{torch.cuda.current_device()}")
        self.ptr = C.c_void_p()
        dbl = C.POINTER(C.c_double)
        keep = [np.ascontiguousarray(a, np.float64) for a in (self.sos, self.zi, self.powers)]
        with torch.cuda.device(self.device):
            L.check(L.lib().jat_iir_create(*(a.ctypes.data_as(dbl) for a in keep), self.R, L.stream_ptr(), C.byref(self.ptr)))
        pl = C.c_int32()
        L.check(L.lib().jat_iir_padlen(self.ptr, C.byref(pl)))
        self.padlen = pl.value
        self._rows = {}

    def __del__(self):
        try:
            if self.ptr:
                L.lib().jat_iir_destroy(self.ptr)
        except Exception:
            pass

    def rows(self, rows, B):
        """row -> filter indices on the device, checked on the host (the device clamps, it cannot refuse)"""
        import torch
        if rows is None:
            if self.R != 1:
                raise ValueError(f"lowpass: a bank of {self.R} filters needs `rows`, one filter index per row")
            rows = (0,) * B
        key = tuple(int(r) for r in (rows.tolist() if hasattr(rows, "tolist") else rows))
        if len(key) != B:
            raise ValueError(f"lowpass: {len(key)} filter indices for {B} rows")
        if any(not 0 <= r < self.R for r in key):
            raise ValueError(f"lowpass: a filter index outside 0..{self.R - 1}")
        t = self._rows.get(key)
        if t is None:
            if len(self._rows) > 64:
                self._rows.clear()
            t = self._rows[key] = torch.tensor(key, dtype=torch.int32, device=self.device)
        return t


def workspace_bytes(B, n):
    out = C.c_size_t()
    L.check(L.lib().jat_iir_workspace_bytes(B, n, C.byref(out)))
    return out.value


def _run(entry, x, bank_or_sos, rows, out):
    import torch
    if not isinstance(x, torch.Tensor) or x.dim() < 1:
        raise JatError("lowpass: x must be a tensor [..., n]")
    if not x.is_cuda:
        raise JatError("lowpass: x must be a CUDA tensor (there is no CPU path)")
    if x.dtype != torch.float32:
        raise JatError(f"lowpass: x must be float32, got {x.dtype}")
    bank = bank_or_sos if isinstance(bank_or_sos, LowpassBank) else LowpassBank([bank_or_sos], x.device)
    if bank.device != x.device:
        raise JatError(f"lowpass: the bank is on {bank.device}, x on {x.device}")
    src = x.detach().contiguous()
    n = src.shape[-1]
    B = src.numel() // n if n else 0
    if B < 1:
        raise ValueError(f"lowpass: empty tensor {tuple(x.shape)}")
    if entry == "jat_iir_sosfiltfilt" and n <= bank.padlen:
        raise ValueError(f"lowpass: the length of the input ({n}) must be greater than padlen ({bank.padlen})")
    idx = bank.rows(rows, B)
    if out is None:
        out = torch.empty_like(src)
    elif out.shape != x.shape or out.dtype != torch.float32 or out.device != x.device or not out.is_contiguous():
        raise ValueError("lowpass: out must be a contiguous float32 tensor of x's shape on x's device")
    elif out.data_ptr() == x.data_ptr() and src.data_ptr() != x.data_ptr():
        raise ValueError("lowpass: in place needs a contiguous x")
    fn = getattr(L.lib(), entry)
    with torch.cuda.device(x.device):
        stream = L.stream_ptr()
        for b0 in range(0, B, 65535):                       # rows per launch: one grid dimension
            nb = min(B - b0, 65535)
            nbytes = workspace_bytes(nb, n)
            work = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
            L.check(fn(bank.ptr, C.c_void_p(idx.data_ptr() + 4 * b0), C.c_void_p(src.data_ptr() + 4 * b0 * n),
                       C.c_void_p(out.data_ptr() + 4 * b0 * n), nb, n, L.ptr(work), nbytes, stream))
    return out


def sosfilt(x, bank_or_sos, rows=None, out=None):
    """scipy.signal.sosfilt along the last axis from zero state: x fp32 CUDA [..., n]; a LowpassBank with `rows` (one filter
    index per row of x flattened to [B, n]) or one sos.  `out` may be x.  An sos builds a LowpassBank for this one call (a
    device allocation, a wait for the stream, a free when it is collected): on a hot path make the bank once and pass it."""
    return _run("jat_iir_sosfilt", x, bank_or_sos, rows, out)


def sosfiltfilt(x, bank_or_sos, rows=None, out=None):
    """scipy.signal.sosfiltfilt along the last axis with its default odd padding; n must exceed the bank's largest padlen.
    As with `sosfilt`, pass a LowpassBank on a hot path, not an sos."""
    return _run("jat_iir_sosfiltfilt", x, bank_or_sos, rows, out)


_banks: dict = {}


def simulate_lr_filtered(hr, sr, filt):
    """The low-resolution simulation with an IIR low-pass in the place of the resampling round trip: `hr` fp32 CUDA [..., n] at
    `sr` -> the same shape, zero phase.  `filt`: {"kind", "order", "cutoff_hz"[, "ripple_db"]}."""
    key = (filt["kind"], int(filt["order"]), float(filt["cutoff_hz"]), float(filt.get("ripple_db", 1.0)), int(sr), hr.device)
    bank = _banks.get(key)
    if bank is None:
        if len(_banks) > 256:
            _banks.clear()
        bank = _banks[key] = LowpassBank([filter_sos(filt, sr)], hr.device)
    return sosfiltfilt(hr, bank)


# ---- flags shared by prepare and infer ------------------------------------------------------------------------------------------------
def parse_range(text, what, cast=float):
    """"LO,HI" (or one value) -> (lo, hi)"""
    parts = str(text).split(",")
    try:
        vals = [cast(p) for p in parts]
    except ValueError:
        vals = []
    if len(vals) not in (1, 2):
        raise SystemExit(f"{what}: expected LO,HI, got {text!r}")
    return (vals[0], vals[-1])


def build_parser():
    p = argparse.ArgumentParser(description="zero-phase IIR low-pass of a WAV file on MI355X (scipy's sosfiltfilt)")
    p.add_argument("--in", dest="src", required=True, help="input WAV")
    p.add_argument("--out", dest="dst", required=True, help="output WAV (float32)")
    p.add_argument("--kind", choices=KINDS, default="butter")
    p.add_argument("--order", type=int, default=8)
    p.add_argument("--cutoff-hz", type=float, required=True)
    p.add_argument("--ripple-db", type=float, default=1.0, help="cheby1: passband ripple")
    p.add_argument("--device", default="cuda", help="an AMD GPU; there is no CPU path")
    return p


def main(argv=None):
    import torch

    from . import io as jio
    args = build_parser().parse_args(argv)
    x, sr = jio.read_wav(args.src)
    filt = {"kind": args.kind, "order": args.order, "cutoff_hz": args.cutoff_hz, "ripple_db": args.ripple_db}
    check_filter(args.kind, args.order, args.cutoff_hz, sr, args.ripple_db)
    y = simulate_lr_filtered(torch.as_tensor(np.asarray(x), dtype=torch.float32).to(args.device).contiguous(), sr, filt)
    jio.write_wav_float32(args.dst, y.cpu().numpy(), sr)
    print(f"{args.src} -> {args.dst}: {args.kind} order {args.order} at {args.cutoff_hz:g} Hz, {y.shape[-1]} samples at {sr} Hz")


if __name__ == "__main__":
    main()
