"""The resampler's launch shapes that no shipped conversion reaches (csrc/resample.hip: phase slices, the PH switch, K < 8,
K a multiple of 8, one frame group at a window near the LDS limit, pick_groups with want > 1, more rows than one launch, the
31-bit limits), over the case table of tests/resample_cases.py; and the small forms of the statistics kernel.  Each test asks
`jat_k_resample_geometry` for the launch it is about to run, so it places its edges where the launch has them.

(a) The table read back exactly.  One impulse per output window: every output is fmaf(h, a, 0) with a a power of two, so the
    whole output is compared with np.array_equal against the host table (`sinc_table`, pinned to fp64 by
    tests/test_resample_cpu.py).  No tolerance.

(b) Dense input against fp64 with a bound per output.  The kernel computes, for one output, s_K with s_0 = 0 and
    s_{k+1} = fl(h32[k] x[k] + s_k) (one fmaf each, ascending k), where h32[k] = h64[k] (1 + d_k) is the host's rounding of the
    fp64 table to fp32, |d_k| <= u = 2^-24.  Each fmaf rounds once: s_{k+1} = (h32[k] x[k] + s_k)(1 + e_k), |e_k| <= u.  Unrolled,
    the product of tap k carries (1 + d_k) and the factors (1 + e_j) for j >= k: at most K + 1 factors, so
        s_K = sum_k h64[k] x[k] (1 + t_k),  |t_k| <= g_{K+1},  g_m = m u / (1 - m u)        (Higham, Lemma 3.1)
    and  |s_K - y64| <= g_{K+1} sum_k |h64[k] x[k]|.  The sum of absolute products is computed in fp64 beside the reference
    (`resample_ref.resample`).  The bound comes from the arithmetic alone; the figures below only report how much of it is used.

Measured on MI355X (worst error / bound over both rows and all lengths of (b); worst row's rel-L2; max-abs), as in DESIGN.md
section 11, "Launch shapes under test":
    47952 -> 44100   0.003  7.3e-8  1.4e-7      44100 -> 47952   0.004  6.9e-8  1.5e-7      11025 -> 96000   0.029  6.8e-8  1.4e-7
    1000 -> 2049000  0.235  6.7e-8  8.6e-8      4000 -> 132300   0.090  6.9e-8  1.5e-7      1000 -> 31000    0.198  6.0e-8  6.2e-8
    1000 -> 32000    0.254  7.2e-8  7.9e-8      1000 -> 33000    0.232  6.9e-8  1.2e-7      8000 -> 48000    0.262  7.1e-8  9.4e-8
    48000 -> 32000   0.162  8.8e-8  1.3e-7      22050 -> 44100 (width 1)  0.296  3.7e-8  3.1e-8
    48000 -> 8000    0.053  1.6e-7  9.2e-8      5000 -> 220500   0.150  7.0e-8  1.2e-7      48000 -> 100   < 0.0005  1.2e-6  2.4e-8
    96000 -> 11025   0.004  1.9e-7  9.0e-8      16000 -> 44100   0.024  6.8e-8  1.1e-7      44100 -> 16000   0.012  1.1e-7  1.8e-7
    48000 -> 16000   0.100  1.2e-7  1.2e-7      44100 -> 48000   0.024  6.9e-8  1.4e-7      65539 rows of 48000 -> 16000: 0.097
The whole file takes 4 s.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import resample_cases as RC  # noqa: E402
import resample_ref as R  # noqa: E402
from jatsr_amd import _lib as L  # noqa: E402
from jatsr_amd.resample import _handle, channel_stats, resample, sinc_table  # noqa: E402

CASES = [c for c, _ in RC.CASES]
FRAMES = 8                        # RS_FRAMES: frames per frame group
GUARD = 4096
REL_GATE, ABS_GATE = 1e-6, 2e-6   # the file-level gates of tests/test_gpu_resample.py, sized for up to 475 taps
FIELDS = ("K", "ph", "pn", "slices", "lanes", "groups_max", "groups", "grid_x", "block", "lds_bytes")
U = 2.0 ** -24


def launch(case, n_in):
    """the launch `jat_resample` makes for rows of n_in samples (`jat_k_resample_geometry`), with fpb = frames per block"""
    v = [C.c_int32(-1) for _ in FIELDS]
    L.check(L.lib().jat_k_resample_geometry(case[0], case[1], case[2], case[3], n_in, *(C.byref(x) for x in v)))
    s = {f: x.value for f, x in zip(FIELDS, v)}
    s["fpb"] = s["groups"] * FRAMES
    return s


def raw(case, x):
    """x fp32 numpy or CUDA [B, L] -> y fp32 numpy [B, L_out] through the C ABI, into a buffer with NaN guard bands before and
    after it and NaN in place of every output: the guards must come back intact and no NaN may be left"""
    x = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    B, n_in = x.shape
    h = _handle(case[0], case[1], case[2], float(case[3]), x.device)
    n_out = C.c_int64()
    L.check(L.lib().jat_resample_out_length(h.ptr, n_in, C.byref(n_out)))
    n_out = n_out.value
    assert n_out == R.out_length(n_in, case[0], case[1])
    buf = torch.full((B * n_out + 2 * GUARD,), float("nan"), dtype=torch.float32, device=x.device)
    L.check(L.lib().jat_resample(h.ptr, L.ptr(x), C.c_void_p(buf.data_ptr() + 4 * GUARD), B, n_in, L.stream_ptr()))
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all()), "a write outside the output"
    y = buf[GUARD:GUARD + B * n_out].view(B, n_out).cpu().numpy()
    assert not np.isnan(y).any(), "an output was not written"
    return y


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and a.tobytes() == b.tobytes()


# ---- (a) the table read back through the kernel ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=RC.IDS)
def test_the_table_read_back_exactly(case):
    """Row 0: a comb of impulses i = 0 .. o at j_i = i s, s >= K and s = 1 (mod o), amplitude 2^(i % 5 - 2): no window of K
    samples holds two of them and j_i runs through every residue mod o, so between them they read every tap of every phase
    (impulse o repeats residue 0: the window that would read tap width + o of impulse 0 lies before the first frame).
    Row 1: an impulse at the last sample block b stages (its last frame, tap K - 1) and one at sample L - 1.
    Row 2: an impulse at the first sample block b + 1 stages (its first frame, tap 0).
    Expected: y[f n + p] = a_i h32[p][j_i - f o + width] where that tap exists, 0 elsewhere, compared exactly."""
    h32, o, n, width, K = sinc_table(*case)
    s = (K - 1 + o - 1) // o * o + 1
    assert s >= K and s % o == 1 % o
    comb = [(0, i * s, 2.0 ** (i % 5 - 2)) for i in range(o + 1)]
    # the block edge: the launch's frames per block changes with the length only beyond 6144 frames, which none of these reach
    n_in = o * s + K + o + 1
    fpb = launch(case, n_in)["fpb"]
    b = 0
    while (b + 1) * fpb * o - width < 0:
        b += 1
    last_of_b, first_of_next = ((b + 1) * fpb - 1) * o - width + K - 1, (b + 1) * fpb * o - width
    n_in = max(n_in, last_of_b + K + o + 2, first_of_next + K + o + 2) + 3
    shape = launch(case, n_in)
    assert shape["fpb"] == fpb and shape["grid_x"] >= b + 2 and (n_in - 1) - last_of_b >= K
    impulses = comb + [(1, last_of_b, 1.0), (1, n_in - 1, 0.5), (2, first_of_next, 2.0)]
    x = np.zeros((3, n_in), np.float32)
    for row, j, a in impulses:
        assert x[row, j] == 0
        x[row, j] = a
    assert x[0, 0] == 0.25

    n_out = R.out_length(n_in, case[0], case[1])
    want = np.zeros((3, n_out), np.float32)
    touched = np.zeros((n, K), bool)
    edge_taps = set()
    for row, j, a in impulses:
        f_lo, f_hi = max(0, -(-(j + width - K + 1) // o)), (j + width) // o          # frames whose window holds sample j
        for f in range(f_lo, f_hi + 1):
            k = j - f * o + width
            assert 0 <= k < K
            m = min(n, n_out - f * n)                                                # outputs of frame f inside L_out
            if m <= 0:
                continue
            assert not want[row, f * n:f * n + m].any(), "two impulses in one window"
            want[row, f * n:f * n + m] = np.float32(a) * h32[:m, k]                  # a power of two: exact
            touched[:m, k] = True
            if row > 0:
                edge_taps.add((row, f, k))
    assert touched.all(), f"{int((~touched).sum())} (p, k) of the table were not read"
    assert (1, (b + 1) * fpb - 1, K - 1) in edge_taps and (2, (b + 1) * fpb, 0) in edge_taps

    y = raw(case, x)
    if not np.array_equal(y, want):
        bad = np.argwhere(y != want)
        row, i = bad[0]
        pytest.fail(f"{len(bad)} outputs differ; first at row {row}, output {i} (frame {i // n}, phase {i % n}): "
                    f"{y[row, i]!r} != {want[row, i]!r}")


# ---- (b) dense input against fp64 --------------------------------------------------------------------------------------------
def reference(x, case):
    """-> (y64, sum_k |h64 x|) [B, L_out]"""
    o, n, width, K, _ = R.dims(*case)
    h = np.abs(R.table(*case))
    ax = np.abs(np.asarray(x, np.float64))
    n_in = x.shape[-1]
    n_out = R.out_length(n_in, case[0], case[1])
    F = -(-n_out // n)
    xp = np.zeros(x.shape[:-1] + (width + (F - 1) * o + K + o,))
    xp[..., width:width + n_in] = ax
    idx = (np.arange(F) * o)[:, None] + np.arange(K)[None, :]
    mag = (xp[..., idx] @ h.T).reshape(x.shape[:-1] + (F * n,))[..., :n_out]
    return R.resample(x, *case), mag


def gamma(m):
    return m * U / (1 - m * U)


def dense_lengths(case):
    """-> (input lengths, the residues L_out % n they end a row at): from the launch the library reports, lengths that make a
    last block with one live frame, a last block that is full, and L_out % n = 1, n - 1 and 0 — those of the three that
    ceil(n L / o) mod n can take at all (only 0 for o = 1 or n = 1)"""
    o, n = R.dims(*case)[:2]
    fpb = launch(case, 16 * o)["fpb"]
    props = {}
    reachable = {-(-n * r // o) % n for r in range(o)} & {1 % n, (n - 1) % n, 0}
    for n_in in range((fpb - 1) * o + 1, (2 * fpb + 3) * o):
        n_out = -(-n * n_in // o)
        frames = -(-n_out // n)
        for key, hit in ((("one live frame",), frames > fpb and frames % fpb == 1), (("full last block",), frames % fpb == 0),
                         (("L_out % n", n_out % n), n_out % n in reachable)):
            if hit:
                props.setdefault(key, n_in)
    assert ("one live frame",) in props and ("full last block",) in props
    assert {k[1] for k in props if k[0] == "L_out % n"} == reachable
    out = sorted(set(props.values()))
    for n_in in out:
        assert launch(case, n_in)["fpb"] == fpb
    return out, sorted(reachable)


@pytest.mark.parametrize("case", CASES, ids=RC.IDS)
def test_dense_input_within_the_derived_bound(case):
    o, n, width, K, _ = R.dims(*case)
    rng = np.random.default_rng(K + n)
    worst, worst_rel, worst_abs = 0.0, 0.0, 0.0
    lengths, residues = dense_lengths(case)
    for n_in in lengths:
        x = (rng.standard_normal((2, n_in)) * np.array([[0.25], [0.003]])).astype(np.float32)
        y = raw(case, x).astype(np.float64)
        ref, mag = reference(x, case)
        assert y.shape == ref.shape
        err = np.abs(y - ref)
        bound = gamma(K + 1) * mag
        ratio = float((err[bound > 0] / bound[bound > 0]).max())
        assert not (err[bound == 0] > 0).any()
        worst = max(worst, ratio)
        for row in range(2):
            worst_rel = max(worst_rel, float(np.linalg.norm(y[row] - ref[row]) / np.linalg.norm(ref[row])))
        worst_abs = max(worst_abs, float(err.max()))
    print(f"{case[0]} -> {case[1]} lpw {case[2]} (K {K}, lengths {lengths}, L_out % n in {residues}): worst error / bound "
          f"{worst:.3f}, rel-L2 {worst_rel:.2e}, max-abs {worst_abs:.2e}")
    assert worst < 1.0
    # The file-level gates of tests/test_gpu_resample.py too.  Where the filter is long the bound above is loose (a worst case
    # over K roundings; measured 0.003 of it at K = 1346), and these gates are what holds the error near its measured size.
    # One exception, the rel-L2 gate of 48000 -> 100: a 480-fold decimation of white noise keeps 1 / 480 of its power, so the
    # outputs are about 22 times smaller than the sums of products they are rounded from and rel-L2 grows by that factor
    # (measured 1.2e-6); its max-abs gate holds.
    assert worst_abs <= ABS_GATE
    if case[:2] != (48000, 100):
        assert worst_rel <= REL_GATE


# ---- (c) the bits do not depend on the launch shape ----------------------------------------------------------------------------
def two_lengths(case):
    """-> (short, long, differ): a short length and, where some length makes the launch take another number of frame groups
    (want = n_frames / 6144 > 1), the first such length; else a length with more blocks"""
    o, n, width, K, _ = R.dims(*case)
    first = launch(case, 6144 * o)
    short = (2 * first["fpb"] + 1) * o + K + 3
    assert launch(case, short)["groups"] == first["groups"]
    for m in range(2, first["groups_max"] + 1):
        if launch(case, m * 6144 * o)["groups"] != first["groups"]:
            return short, m * 6144 * o, True
    return short, (5 * first["fpb"] + 2) * o + K, False


@pytest.mark.parametrize("case", CASES, ids=RC.IDS)
def test_bits_do_not_depend_on_the_launch_shape(case):
    o, n, width, K, _ = R.dims(*case)
    short, long, differ = two_lengths(case)
    a, b = launch(case, short), launch(case, long)
    # which cases have lengths whose launches differ in frame groups is pinned on the host (tests/test_resample_geometry_cpu.py):
    # the four named here go through want > 1; the others are compared at two block counts
    assert differ == (a["groups"] != b["groups"]) and a["grid_x"] != b["grid_x"]
    if case[:2] in ((48000, 16000), (44100, 48000), (1000, 31000), (16000, 44100)):
        assert differ and b["groups"] > a["groups"]
    g = torch.Generator(device="cuda").manual_seed(K)
    x = 0.25 * torch.randn(1, long, device="cuda", generator=g)
    y_long = raw(case, x)
    y_short = raw(case, x[:, :short].contiguous())
    inside = min(((short + width - K) // o + 1) * n, y_short.shape[1])       # frames whose window ends within the short input
    assert inside > a["fpb"] * n                                              # more than one block of them
    assert same_bits(y_short[:, :inside], y_long[:, :inside])
    # a row alone = the same row in a batch of three
    x3 = 0.25 * torch.randn(3, short, device="cuda", generator=g)
    y3 = raw(case, x3)
    for row in range(3):
        assert same_bits(y3[row:row + 1], raw(case, x3[row:row + 1].contiguous())), row


# ---- (d) more rows than one launch takes -----------------------------------------------------------------------------------------
def test_more_rows_than_one_launch():
    case = (48000, 16000, 6, 0.99)
    B = 65536 + 3
    rng = np.random.default_rng(65539)
    x = (rng.standard_normal((B, 5)) * rng.choice([0.25, 0.003], (B, 1))).astype(np.float32)
    xg = torch.from_numpy(x).cuda()
    y = resample(xg, case[0], case[1])
    assert y.shape == (B, 2)
    ref, mag = reference(x, case)
    err = np.abs(y.cpu().numpy().astype(np.float64) - ref)
    ratio = float((err / (gamma(R.dims(*case)[3] + 1) * mag)).max())
    print(f"65539 rows: worst error / bound {ratio:.3f}")
    assert ratio < 1.0
    assert same_bits(y[-4:].cpu().numpy(), resample(xg[-4:].clone(), case[0], case[1]).cpu().numpy())
    assert same_bits(y[65533:65537].cpu().numpy(), resample(xg[65533:65537].clone(), case[0], case[1]).cpu().numpy())


# ---- (e) the 31-bit limits of jat_resample_out_length ------------------------------------------------------------------------------
def test_out_length_at_the_31_bit_limits():
    """include/jat_hip.h: "fails when L_out or L + K does not fit in 31 bits".  16 -> 48 kHz (n / o = 3): L_out = 3 L, and
    3 * 715827882 = 2^31 - 2 is the last multiple of 3 below 2^31.  48 -> 16 kHz (K = 41): L + 41 <= 2^31 - 1 up to
    L = 2147483606, where L_out = ceil(L / 3) is far below the limit."""
    lim = 2 ** 31 - 1
    dev = torch.device("cuda", torch.cuda.current_device())
    out = C.c_int64(-7)
    up = _handle(16000, 48000, 6, 0.99, dev)
    assert 3 * 715827882 == lim - 1 and 3 * 715827883 > lim
    assert L.lib().jat_resample_out_length(up.ptr, 715827882, C.byref(out)) == 0 and out.value == 2147483646
    out.value = -7
    assert L.lib().jat_resample_out_length(up.ptr, 715827883, C.byref(out)) == L.JAT_E_INVALID and out.value == -7
    down = _handle(48000, 16000, 6, 0.99, dev)
    assert R.dims(48000, 16000)[3] == 41 and 2147483606 + 41 == lim
    assert L.lib().jat_resample_out_length(down.ptr, 2147483606, C.byref(out)) == 0 and out.value == -(-2147483606 // 3)
    out.value = -7
    assert L.lib().jat_resample_out_length(down.ptr, 2147483607, C.byref(out)) == L.JAT_E_INVALID and out.value == -7
    assert L.lib().jat_resample_out_length(down.ptr, -1, C.byref(out)) == L.JAT_E_INVALID and out.value == -7
    # a refused length launches nothing
    x = torch.ones(64, device="cuda")
    y = torch.full((64,), 123.0, device="cuda")
    for h, bad in ((up, 715827883), (down, 2147483607), (down, -1)):
        assert L.lib().jat_resample(h.ptr, L.ptr(x), L.ptr(y), 1, bad, L.stream_ptr()) == L.JAT_E_INVALID
    torch.cuda.synchronize()
    assert bool((y == 123.0).all()) and bool((x == 1.0).all())


# ---- (f) the small forms of the statistics kernel ------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Cc,T", [(3, 4, 5), (1, 1, 1), (1, 3, 16 * 256 + 1), (17, 2, 241), (3, 1, 2731), (2, 1, 603)],
                         ids=["BT15", "BT1-C1", "BT4097-one-row", "BT4097-17-rows", "BT8193-C1", "C1"])
def test_channel_stats_small_forms(B, Cc, T):
    """Forms of stats_partial_kernel that B = 2, T in {603, 1}, C = 1024 do not reach: fewer elements than the 16 slices (empty
    slices), B T = 16 * 256 k + 1 (slices of 256 k + 1 elements: one past a whole pass of the block, cut across the rows),
    one channel.  The gate is the file's: 1e-12 relative to sum |v| (a reordered fp64 sum of N <= 8193 terms errs by less than
    N 2^-53 sum |v| = 9.1e-13 sum |v|)."""
    rng = np.random.default_rng(B * 1000 + T)
    z = (3.0 * rng.standard_normal((B, Cc, T)) + rng.standard_normal((1, Cc, 1))).astype(np.float32)
    s, q = channel_stats(torch.from_numpy(z).cuda())
    v = z.astype(np.float16).astype(np.float64)
    rs, rq, ra = v.sum(axis=(0, 2)), (v * v).sum(axis=(0, 2)), np.abs(v).sum(axis=(0, 2))
    es = float((np.abs(s.cpu().numpy() - rs) / ra).max())
    eq = float((np.abs(q.cpu().numpy() - rq) / rq).max())
    print(f"B={B} C={Cc} T={T}: sum {es:.2e}, sq_sum {eq:.2e} (gate 1e-12)")
    assert s.shape == q.shape == (Cc,) and es <= 1e-12 and eq <= 1e-12
