"""The voicing-aware index rates on the GPU (jat_f0_classes, jat_rate_track, jat_rate_mix, `retrieve` with a per-frame
track, sample_long(index_rates=), infer --index-protect / --index-unstable / --index-smooth) against the numpy twins of
tests/retrieval_rate_ref.py, bit for bit, and against the scalar blends the track has to reproduce when it is constant."""
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
import retrieval_rate_ref as RR  # noqa: E402
import retrieval_ref as R  # noqa: E402
import jatsr_amd  # noqa: E402
import jatsr_amd.io as jio  # noqa: E402
import jatsr_amd.recipe as recipe  # noqa: E402
from jatsr_amd import _lib as L  # noqa: E402
from jatsr_amd import pitch  # noqa: E402
from jatsr_amd import retrieval as RT  # noqa: E402
from jatsr_amd.retrieval import IVFBank, LatentBank, MultiScaleBank  # noqa: E402
from stream_check import Case, check_case  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV = L.JAT_E_INVALID
F32 = np.float32
SENTINEL = 0x5A


def cuda(a):
    return torch.from_numpy(np.array(a)).cuda()


def tstats(C_, salt=0):
    return {k: cuda(v) for k, v in R.stats(C_, salt).items()}


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(t, a):
    got = t.detach().cpu().numpy()
    return got.shape == a.shape and got.dtype == a.dtype and got.tobytes() == np.ascontiguousarray(a).tobytes()


def sentinel(shape, dtype):
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(torch.uint8).fill_(SENTINEL)
    return t


def untouched(t):
    return bool((t.view(torch.uint8) == SENTINEL).all())


# ---- raw entries ---------------------------------------------------------------------------------------------------------------------
def raw_classes(f0, voiced, W, ratio, m, cls, count, summary, B=None, F=None):
    b, f = f0.shape if f0 is not None else (1, 1)
    return L.lib().jat_f0_classes(L.ptr(f0), L.ptr(voiced), b if B is None else B, f if F is None else F, W, float(ratio), m,
                                  L.ptr(cls), L.ptr(count), L.ptr(summary), L.stream_ptr())


def raw_track(cls, T, table, S, r, B=None, F=None):
    b, f = cls.shape if cls is not None else (1, 1)
    tb = None if table is None else (C.c_float * 3)(*[float(v) for v in table])
    return L.lib().jat_rate_track(L.ptr(cls), b if B is None else B, f if F is None else F, T, tb, S, L.ptr(r), L.stream_ptr())


def raw_mix(x, v, rates, y, B=None, Cc=None, T=None):
    b, c, t = x.shape if x is not None else (1, 1, 1)
    return L.lib().jat_rate_mix(L.ptr(x), L.ptr(v), L.ptr(rates), L.ptr(y), b if B is None else B, c if Cc is None else Cc,
                                t if T is None else T, L.stream_ptr())


# ---- 1. classes -----------------------------------------------------------------------------------------------------------------------
RATIO = RR.cents_ratio(50.0)


def class_tracks(F=41):
    """B = 3: all unvoiced (the f0 values are there, the flags are not); a constant track with flags set on f0 = 0, +inf and NaN;
    a glide of 20 cents a frame (two neighbours inside the ratio, the third outside) with a pair exactly on the boundary and one
    a single ulp beyond it"""
    f0 = np.empty((3, F), F32)
    voiced = np.ones((3, F), np.uint8)
    f0[0] = 220.0
    voiced[0] = 0
    f0[1] = 200.0                                                        # the glide of the next row starts here: a window that runs on finds agreeing frames
    for t, v in ((3, 0.0), (17, np.inf), (18, np.nan), (F - 1, -5.0)):
        if t < F:
            f0[1, t] = v
    f0[2] = (200.0 * 2.0 ** (np.arange(F) * 20.0 / 1200.0)).astype(F32)
    if F > 13:
        f0[2, 10] = 300.0
        f0[2, 11] = F32(F32(300.0) * RATIO)                               # exactly on the boundary of frame 10
        f0[2, 13] = np.nextafter(f0[2, 11], F32(np.inf))                  # one ulp beyond it
        voiced[2, 30] = 0
    return f0, voiced


@pytest.mark.parametrize("W", [0, 1, 4])
@pytest.mark.parametrize("F", [41, 1, 3, 300])
def test_classes_equal_the_twin(F, W):
    f0, voiced = class_tracks(F)
    for m in sorted({1, RR.default_min_count(W), 2 * W + 1}):
        want = RR.f0_classes(f0, voiced, W, RATIO, m)
        d_f0, d_v = cuda(f0), cuda(voiced)
        cls, count, summary = sentinel((3, F), torch.uint8), sentinel((3, F), torch.int32), sentinel((3, 2), torch.int32)
        assert raw_classes(d_f0, d_v, W, RATIO, m, cls, count, summary) == 0
        assert same_bits(cls, want[0]) and same_bits(count, want[1]) and same_bits(summary, want[2]), (F, W, m)
        only = sentinel((3, F), torch.uint8)
        assert raw_classes(d_f0, d_v, W, RATIO, m, only, None, None) == 0   # both optional outputs NULL
        assert same_bits(only, want[0])
    if F == 41 and W == 4:
        assert want[0][0].tolist() == [0] * F and set(want[0][1].tolist()) == {0, 1, 2} and 1 in want[0][2]
        c7 = RR.f0_classes(f0, voiced, 4, RATIO, 7)[1]
        assert c7[2, 10] >= 2 and RR.f0_classes(f0, voiced, 1, RATIO, 1)[1][2, 10] == 2       # frame 11 agrees with frame 10
    # the Python wrapper: the same bits, with and without the batch axis
    cls, summary, count = RT.f0_classes(cuda(f0), cuda(voiced).view(torch.bool), half_window=W, counts=True)
    want = RR.f0_classes(f0, voiced, W, RATIO, RR.default_min_count(W))
    assert same_bits(cls, want[0]) and same_bits(count, want[1]) and same_bits(summary, want[2])
    one = RT.f0_classes(cuda(f0[2]), cuda(voiced[2]), half_window=W)
    assert same_bits(one[0], want[0][2]) and same_bits(one[1], want[2][2])


# ---- 2. rate track ----------------------------------------------------------------------------------------------------------------------
def class_rows(F=41):
    rng = np.random.default_rng(11)
    cls = rng.integers(0, 3, size=(3, F)).astype(np.uint8)
    cls[0] = np.repeat(rng.integers(0, 3, size=F // 8 + 1), 8)[:F]        # stretches: frames far from any change exist
    cls[1] = 1                                                            # a constant row
    cls[2, ::5] = 7                                                       # above 2 counts as 2
    return cls


TABLE = RR.rate_table(0.4, 0.33, 0.7)


@pytest.mark.parametrize("S", [0, 2, 16])
@pytest.mark.parametrize("T", [1, 30, 41, 50])
def test_rate_track_equals_the_twin(T, S):
    cls = class_rows()
    for table in (TABLE, np.array([0, 1, 1], F32), np.array([1 / 3, 0.0, 1.0], F32)):
        want = RR.rate_track(cls, T, table, S)
        r = sentinel((3, T), torch.float32)
        assert raw_track(cuda(cls), T, table, S, r) == 0
        assert same_bits(r, want), (T, S, table)
        assert ((want >= 0) & (want <= 1)).all()
        assert (want[1, :min(T, 41 - S)] == table[1]).all()                # the constant row: one value up to S before its end
        if S == 0:                                                        # the table entries; class 0 behind the pitch track
            padded = np.pad(cls, ((0, 0), (0, max(0, T - 41))))[:, :T]
            assert same_bits(r, np.asarray(table, F32)[np.minimum(padded, 2)])
    got = RT.rate_track(cuda(cls), T, 0.4, protect=0.33, unstable=0.7, smooth=S)
    assert same_bits(got, RR.rate_track(cls, T, TABLE, S))
    assert same_bits(RT.rate_track(cuda(cls[0]), T, 0.4, protect=0.33, unstable=0.7, smooth=S), RR.rate_track(cls[:1], T, TABLE, S)[0])
    # protect = unstable = 1: the scalar rate on every frame
    assert same_bits(RT.rate_track(cuda(cls), T, 0.4, smooth=S), np.full((3, T), F32(0.4), F32))


def test_rate_track_behind_the_pitch_track_is_unvoiced():
    cls = np.full((1, 41), 2, np.uint8)
    r = RT.rate_track(cuda(cls), 50, 0.5, protect=0.0, smooth=0).cpu().numpy()
    assert (r[0, :41] == 0.5).all() and (r[0, 41:] == 0.0).all()
    r2 = RT.rate_track(cuda(cls), 50, 0.5, protect=0.0, smooth=2).cpu().numpy()
    assert same_bits(torch.from_numpy(r2), RR.rate_track(cls, 50, RR.rate_table(0.5, 0.0), 2))
    assert (r2[0, :39] == 0.5).all() and (r2[0, 43:] == 0.0).all() and 0 < r2[0, 41] < 0.5
    # the window is cut at the end of the row: the last frames divide by their own number of taps
    edge = np.array([[2] * 6 + [0] * 2], np.uint8)
    got = RT.rate_track(cuda(edge), 8, 1.0, protect=0.0, smooth=2).cpu().numpy()[0]
    # c = 1 1 1 1 1 1 0 0: frame 7 sees frames 5..7 (1 / 3, not 1 / 5), frame 6 frames 4..7 (2 / 4), frame 5 frames 3..7 (1 - 2 / 5)
    assert got[7] == F32(F32(1) / F32(3)) and got[6] == 0.5 and got[5] == F32(1 + F32(F32(-2) / F32(5))) and got[0] == 1.0


# ---- 3. mix -------------------------------------------------------------------------------------------------------------------------------
def mix_inputs(B, Cc, T, salt=0):
    x = recipe.gaussian("rate_mix_x", (B, Cc, T), salt).astype(F32)
    v = recipe.gaussian("rate_mix_v", (B, Cc, T), salt).astype(F32)
    flat_x, flat_v = x.reshape(-1), v.reshape(-1)                          # views: zeros of both signs against each other
    for i, (a, b) in enumerate(((0.0, -0.0), (-0.0, 0.0), (0.0, 0.0), (-0.0, -0.0), (1.5, -0.0), (-1.5, -0.0), (-0.0, 2.0))):
        flat_x[i::23], flat_v[i::23] = a, b
    rates = np.random.default_rng(salt + 3).random((B, T)).astype(F32)
    rates[:, ::4] = 0.0
    rates[:, 1::4] = 1.0
    return x, v, rates


@pytest.mark.parametrize("T", [1, 37, 130, 300])
@pytest.mark.parametrize("Cc", [1, 32, 96])
def test_mix_equals_the_twin(Cc, T):
    B = 2
    x, v, rates = mix_inputs(B, Cc, T, Cc + T)
    want = RR.mix(x, v, rates)
    dx, dv, dr = cuda(x), cuda(v), cuda(rates)
    y = sentinel((B, Cc, T), torch.float32)
    assert raw_mix(dx, dv, dr, y) == 0
    assert same_bits(y, want) and same_bits(dx, x) and same_bits(dv, v)
    assert same_bits(RT.mix_rates(dx, dv, dr), want)
    ix = dx.clone()
    assert RT.mix_rates(ix, dv, dr, out=ix) is ix and same_bits(ix, want)                 # in place on x
    iv = dv.clone()
    assert RT.mix_rates(dx, iv, dr, out=iv) is iv and same_bits(iv, want)                 # in place on v
    if B == 2 and T > 1:
        assert same_bits(RT.mix_rates(dx[:1], dv[:1], dr[0]), want[:1])                     # [T] for B = 1


@pytest.mark.parametrize("norm", [False, True], ids=["plain", "stats"])
@pytest.mark.parametrize("Cc", [32, 96])
def test_constant_track_is_the_scalar_blend(Cc, norm):
    N, B, T = 50, 2, 37
    rows = recipe.gaussian("rate_blend_rows", (N, Cc), Cc).astype(np.float16)
    rows[::3, ::5] = 0.0
    rows[1::3, 1::5] = -0.0
    bank = LatentBank(Cc, N)
    bank.load_rows(cuda(rows))
    st = tstats(Cc, 4)
    ms = (st["hr_mean"], st["hr_std"]) if norm else (None, None)
    x, _, _ = mix_inputs(B, Cc, T, 9)
    dx = cuda(x)
    idx = cuda(np.random.default_rng(2).integers(0, N, size=(B, T)).astype(np.int32))
    v = bank.blend(dx, idx, 1.0, *ms)
    for rate in (0.0, 0.13, 0.4, 1.0):
        track = torch.full((B, T), rate, dtype=torch.float32, device="cuda")
        assert torch.equal(bits(RT.mix_rates(dx, v, track)), bits(bank.blend(dx, idx, rate, *ms))), (Cc, norm, rate)


# ---- 4. composition -------------------------------------------------------------------------------------------------------------------------
COMP_C, COMP_N, COMP_B, COMP_T = 32, 300, 2, 45


def comp_banks():
    st = tstats(COMP_C, 8)
    src = torch.from_numpy(recipe.gaussian("rate_comp_src", (COMP_C, COMP_N), 1) * 1.2 + 0.1)
    flat = LatentBank(COMP_C, COMP_N)
    flat.add(src, st)
    ms = MultiScaleBank(COMP_C, COMP_N, scales=(1, 2, 4))
    ms.add(src, st)
    cent = LatentBank(COMP_C, 6)
    cent.load_rows(flat.rows("keys")[0][::50].clone())
    ivf = IVFBank.from_centroids(flat, cent, nprobe=2)
    x = cuda((recipe.gaussian("rate_comp_x", (COMP_B, COMP_C, COMP_T), 2) * 1.2 + 0.1).astype(F32))
    x.view(-1)[::13] = 0.0
    x.view(-1)[5::17] = -0.0
    return st, {"flat_k1": (flat, 1), "flat_k8": (flat, 8), "ms": (ms, 1), "ms_k8": (ms, 8), "ivf": (ivf, 1), "ivf_k8": (ivf, 8)}, x


def test_retrieve_with_a_track():
    st, banks, x = comp_banks()
    values = (0.4, 0.0, float(F32(0.4 * 0.33)))
    which = np.random.default_rng(3).integers(0, 3, size=(COMP_B, COMP_T))
    three = cuda(np.asarray(values, F32)[which])
    for name, (bank, k) in banks.items():
        scalar = {r: bank.retrieve(x, r, stats=st, k=k, neighbours=True) for r in values + (1.0,)}
        for r in (0.4, 1.0):
            got = bank.retrieve(x, torch.full((COMP_B, COMP_T), r, dtype=torch.float32, device="cuda"), stats=st, k=k)
            assert torch.equal(bits(got), bits(scalar[r][0])), (name, r)
        y, idx, dist2 = bank.retrieve(x, three, stats=st, k=k, neighbours=True)
        for i, r in enumerate(values):                                    # the frames carrying each value: the scalar call's
            m = cuda(which == i)[:, None, :].expand_as(y)
            assert torch.equal(bits(y)[m], bits(scalar[r][0])[m]), (name, r)
        assert not torch.equal(bits(y), bits(scalar[0.4][0]))
        ref_i, ref_d = scalar[0.4][1], scalar[0.4][2]                     # neighbours: what the scalar call returns
        if isinstance(idx, list):
            assert all(torch.equal(a, b) for a, b in zip(idx, ref_i)) and all(torch.equal(bits(a), bits(b)) for a, b in zip(dist2, ref_d))
        else:
            assert torch.equal(idx, ref_i) and torch.equal(bits(dist2), bits(ref_d))
        assert torch.equal(bits(bank.retrieve(x[:1], three[0], stats=st, k=k)), bits(y[:1])), name   # [T] for B = 1


def test_a_float_takes_the_existing_path():
    st, banks, x = comp_banks()
    flat = banks["flat_k1"][0]
    idx, _ = flat.search(x, st["hr_mean"], st["hr_std"])
    want = flat.blend(x, idx, 0.4, st["hr_mean"], st["hr_std"])
    assert torch.equal(bits(flat.retrieve(x, 0.4, stats=st)), bits(want))
    assert torch.equal(bits(flat.retrieve(x, torch.tensor(0.4), stats=st)), bits(want))      # a 0-d tensor is a scalar, as before


# ---- 5. independence, streams, both libraries ---------------------------------------------------------------------------------------------------
def small_run():
    """every entry once, on the inputs of the tests above"""
    f0, voiced = class_tracks()
    cls, summary, count = RT.f0_classes(cuda(f0), cuda(voiced), counts=True)
    r = RT.rate_track(cuda(class_rows()), 50, 0.4, protect=0.33, unstable=0.7, smooth=2)
    x, v, rates = mix_inputs(2, 96, 130, 1)
    y = RT.mix_rates(cuda(x), cuda(v), cuda(rates))
    return {"cls": cls.cpu().numpy(), "summary": summary.cpu().numpy(), "count": count.cpu().numpy(), "r": r.cpu().numpy(),
            "y": y.cpu().numpy()}


def test_independent_of_batch_and_run():
    a, b = small_run(), small_run()
    assert all(a[k].tobytes() == b[k].tobytes() for k in a)
    f0, voiced = class_tracks()
    for i in range(3):
        cls, summary, count = RT.f0_classes(cuda(f0[i:i + 1]), cuda(voiced[i:i + 1]), counts=True)
        assert same_bits(cls, a["cls"][i:i + 1]) and same_bits(summary, a["summary"][i:i + 1]) and same_bits(count, a["count"][i:i + 1])
        r = RT.rate_track(cuda(class_rows()[i:i + 1]), 50, 0.4, protect=0.33, unstable=0.7, smooth=2)
        assert same_bits(r, a["r"][i:i + 1])
    x, v, rates = mix_inputs(2, 96, 130, 1)
    for i in range(2):
        assert same_bits(RT.mix_rates(cuda(x[i:i + 1]), cuda(v[i:i + 1]), cuda(rates[i:i + 1])), a["y"][i:i + 1])


def stream_cases():
    f0, voiced = class_tracks()
    other_v = np.roll(voiced, 5, axis=1) ^ (np.arange(41) % 3 == 0).astype(np.uint8)
    cls = class_rows()
    x, v, rates = mix_inputs(2, 96, 130, 1)

    def classes():
        def call(st, i, o):
            assert raw_classes(i["f0"], i["voiced"], 4, RATIO, 7, o["cls"], o["count"], o["summary"]) == 0
            c, s = RT.f0_classes(i["f0"], i["voiced"])
            return {"w_cls": c, "w_summary": s}
        return Case({"f0": cuda(f0), "voiced": cuda(voiced)}, call,
                    outputs={"cls": torch.empty(3, 41, dtype=torch.uint8, device="cuda"),
                             "count": torch.empty(3, 41, dtype=torch.int32, device="cuda"),
                             "summary": torch.empty(3, 2, dtype=torch.int32, device="cuda")}, decoys={"voiced": cuda(other_v)})

    def track():
        def call(st, i, o):
            assert raw_track(i["cls"], 50, TABLE, 2, o["r"]) == 0
            return {"w_r": RT.rate_track(i["cls"], 50, 0.4, protect=0.33, unstable=0.7, smooth=2)}
        return Case({"cls": cuda(cls)}, call, outputs={"r": torch.empty(3, 50, device="cuda")},
                    decoys={"cls": cuda(np.roll(cls, 3, axis=1) % 3)})

    def mix():
        def call(st, i, o):
            assert raw_mix(i["x"], i["v"], i["rates"], o["y"]) == 0
        return Case({"x": cuda(x), "v": cuda(v), "rates": cuda(rates)}, call, outputs={"y": torch.empty(2, 96, 130, device="cuda")})

    return {"jat_f0_classes": classes, "jat_rate_track": track, "jat_rate_mix": mix}


def test_every_stream_taking_entry_has_a_case():
    header = open(os.path.join(ROOT, "include", "jat_hip_rate.h")).read()
    takes = set(re.findall(r"\bint (jat_[a-z0-9_]+)\([^;]*void\* stream\)", header))
    assert takes == set(stream_cases()) == set(L.RATE_SIGNATURES) and len(takes) == 3


@pytest.mark.parametrize("name", ["jat_f0_classes", "jat_rate_track", "jat_rate_mix"])
def test_side_stream(name):
    check_case(stream_cases()[name](), name, synchronises=False)


def test_graph_capture():
    """the three entries captured into one graph and replayed after every input changed: no allocation, synchronisation or copy"""
    f0a, va = class_tracks()
    f0b, vb = np.roll(f0a, 7, axis=1), np.roll(va, 3, axis=1)
    B, Cc, T, F = 3, 32, 50, 41
    xa, vva, _ = mix_inputs(B, Cc, T, 1)
    xb, vvb, _ = mix_inputs(B, Cc, T, 2)
    f0, voiced, x, v = cuda(f0a), cuda(va), cuda(xa), cuda(vva)
    cls, count, summary = (torch.zeros(s, dtype=d, device="cuda") for s, d in (((B, F), torch.uint8), ((B, F), torch.int32),
                                                                               ((B, 2), torch.int32)))
    r, y = torch.zeros(B, T, device="cuda"), torch.zeros(B, Cc, T, device="cuda")

    def run():
        assert raw_classes(f0, voiced, 4, RATIO, 7, cls, count, summary) == 0
        assert raw_track(cls, T, TABLE, 2, r) == 0
        assert raw_mix(x, v, r, y) == 0
    run()                                                                 # eagerly once: what the first launch of a kernel sets up
    torch.cuda.synchronize()
    first = y.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    for dst, src in ((f0, f0b), (voiced, vb), (x, xb), (v, vvb)):
        dst.copy_(cuda(src))
    g.replay()
    torch.cuda.synchronize()
    wc = RR.f0_classes(f0b, vb, 4, RATIO, 7)
    wr = RR.rate_track(wc[0], T, TABLE, 2)
    assert same_bits(cls, wc[0]) and same_bits(count, wc[1]) and same_bits(summary, wc[2]) and same_bits(r, wr)
    assert same_bits(y, RR.mix(xb, vvb, wr)) and not torch.equal(bits(y), bits(first))


def test_fp16_library_gives_the_same_bits(tmp_path):
    """retrieval_rate.hip is fp32 and integers in both builds: libjat_hip_fp16.so (a child process) computes what this process
    computes"""
    code = ("import sys, numpy as np\n"
            "sys.path.insert(0, 'tests')\n"
            "import jatsr_amd._lib as L\n"
            "from test_retrieval_rate_gpu import small_run\n"
            "assert L.operand_dtype() == 'fp16'\n"
            "np.savez(sys.argv[1], **small_run())\n")
    env = dict(os.environ, JAT_OPERAND_DTYPE="fp16")
    env.pop("JAT_LIB_PATH", None)
    path = str(tmp_path / "fp16.npz")
    out = subprocess.run([sys.executable, "-c", code, path], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
    other, here = dict(np.load(path)), small_run()
    assert sorted(other) == sorted(here) and len(here) == 5
    for k, v in here.items():
        assert v.tobytes() == other[k].tobytes(), k


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_through_the_raw_abi_write_nothing():
    f0, voiced = (cuda(a) for a in class_tracks())
    cls, count, summary = sentinel((3, 41), torch.uint8), sentinel((3, 41), torch.int32), sentinel((3, 2), torch.int32)
    ok = dict(f0=f0, voiced=voiced, W=4, ratio=RATIO, m=7, cls=cls, B=None, F=None)
    for bad in (dict(f0=None), dict(voiced=None), dict(cls=None), dict(B=0), dict(B=-1), dict(F=0), dict(W=-1), dict(W=33), dict(m=0),
                dict(m=10), dict(W=1, m=4), dict(ratio=1.0), dict(ratio=0.9), dict(ratio=float("inf")), dict(ratio=float("nan"))):
        a = dict(ok, **bad)
        assert raw_classes(a["f0"], a["voiced"], a["W"], a["ratio"], a["m"], a["cls"], count, summary, B=a["B"], F=a["F"]) == INV, bad
    torch.cuda.synchronize()
    assert untouched(cls) and untouched(count) and untouched(summary)
    dcls, r = cuda(class_rows()), sentinel((3, 50), torch.float32)
    ok = dict(cls=dcls, T=50, table=TABLE, S=2, r=r, B=None, F=None)
    for bad in (dict(cls=None), dict(table=None), dict(r=None), dict(B=0), dict(F=0), dict(T=0), dict(T=-3), dict(S=-1), dict(S=17),
                dict(table=[0.1, 1.0000001, 0.3]), dict(table=[-1e-9, 0.5, 0.3]), dict(table=[0.1, 0.5, float("nan")]),
                dict(table=[float("inf"), 0.5, 0.3])):
        a = dict(ok, **bad)
        assert raw_track(a["cls"], a["T"], a["table"], a["S"], a["r"], B=a["B"], F=a["F"]) == INV, bad
    torch.cuda.synchronize()
    assert untouched(r)
    x, v, rates = (cuda(a) for a in mix_inputs(2, 32, 37, 0))
    y = sentinel((2, 32, 37), torch.float32)
    ok = dict(x=x, v=v, rates=rates, y=y, B=None, Cc=None, T=None)
    for bad in (dict(x=None), dict(v=None), dict(rates=None), dict(y=None), dict(B=0), dict(Cc=0), dict(T=0), dict(Cc=-1)):
        a = dict(ok, **bad)
        assert raw_mix(a["x"], a["v"], a["rates"], a["y"], B=a["B"], Cc=a["Cc"], T=a["T"]) == INV, bad
    big = sentinel((2 * 32 * 37 + 8,), torch.float32)                     # y overlapping x without being x
    assert raw_mix(big[:2 * 32 * 37].view(2, 32, 37), v, rates, big[8:].view(2, 32, 37)) == INV
    torch.cuda.synchronize()
    assert untouched(y) and untouched(big)


def test_refusals_in_python():
    st, banks, x = comp_banks()
    flat = banks["flat_k1"][0]
    good = torch.full((COMP_B, COMP_T), 0.4, dtype=torch.float32, device="cuda")
    for bad, what in ((good[:, :-1], "shape"), (good[0], "shape"), (good.double(), "dtype"), (good.cpu(), "expected cuda"),
                      (good + 0.7, "outside"), (good - 0.5, "outside"), (good * float("nan"), "outside")):
        for bank, k in banks.values():
            with pytest.raises(ValueError, match=what):
                bank.retrieve(x, bad, stats=st, k=k)
        with pytest.raises(ValueError, match=what):
            RT.mix_rates(x, x, bad)
    with pytest.raises(ValueError, match="does not match"):
        RT.mix_rates(x, x[:, :16].contiguous(), good)
    with pytest.raises(ValueError, match="out must be"):
        RT.mix_rates(x, x, good, out=torch.empty(1, device="cuda"))
    f0, voiced = (cuda(a) for a in class_tracks())
    for kw, what in ((dict(half_window=33), "half_window"), (dict(min_count=10), "min_count"), (dict(min_count=0), "min_count"),
                     (dict(cents=0.0), "cents"), (dict(cents=-3.0), "cents")):
        with pytest.raises(ValueError, match=what):
            RT.f0_classes(f0, voiced, **kw)
    with pytest.raises(ValueError, match="one shape"):
        RT.f0_classes(f0, voiced[:, :-1])
    with pytest.raises(ValueError, match="CUDA"):
        RT.f0_classes(f0.cpu(), voiced.cpu())
    cls = cuda(class_rows())
    for kw, what in ((dict(smooth=17), "smooth"), (dict(protect=1.5), "protect"), (dict(unstable=-0.1), "unstable")):
        with pytest.raises(ValueError, match=what):
            RT.rate_track(cls, 50, 0.4, **kw)
    with pytest.raises(ValueError, match="index_rate"):
        RT.rate_track(cls, 50, 1.4)
    with pytest.raises(ValueError, match="frames"):
        RT.rate_track(cls, 0, 0.4)
    with pytest.raises(ValueError, match="uint8"):
        RT.rate_track(cls.int(), 50, 0.4)


# ---- 7. the fixture through the GPU's tracker -------------------------------------------------------------------------------------------------------
def test_fixture_through_yin_on_the_gpu():
    """tone / noise / glide: the inner frames of tests/test_retrieval_rate_cpu.py::test_fixture_in_fp64 get the classes shown there;
    the frames left out are the ones left out there (36 of 104)"""
    f0, voiced, _ = pitch.yin(cuda(RR.fixture_signal()), sr=RR.SR, hop_length=RR.HOP)
    seg = RR.fixture_inner()
    assert f0.shape == (RR.fixture_frames(),) and int((seg < 0).sum()) == 36
    cls, summary, count = RT.f0_classes(f0, voiced, half_window=RR.FIXTURE_W, counts=True)
    want = np.array(RR.FIXTURE_CLASSES)[seg[seg >= 0]]
    got = cls.cpu().numpy()
    print("classes:", "".join(str(c) for c in got), "left out:", int((seg < 0).sum()), "of", len(seg))
    assert (got[seg >= 0] == want).all()
    tw = RR.f0_classes(f0.cpu().numpy()[None], voiced.cpu().numpy()[None], RR.FIXTURE_W)
    assert same_bits(cls, tw[0][0]) and same_bits(count, tw[1][0]) and same_bits(summary, tw[2][0])
    r = RT.rate_track(cls, len(seg), 0.4, protect=0.33, unstable=0.7, smooth=2).cpu().numpy()
    inner2 = RR.fixture_inner(RR.FIXTURE_W + 2)                           # farther than S = 2 from any frame that is left out
    for s, rate in enumerate((F32(0.4), F32(0.4 * 0.33), F32(0.4 * 0.7))):
        assert (inner2 == s).sum() >= 15 and (r[inner2 == s] == rate).all()


# ---- 8. the sampler and the command line --------------------------------------------------------------------------------------------------------------
def micro_model(**over):
    cfg = dict(recipe.CONFIGS["micro"], **over)
    m = jatsr_amd.JaT_AudioSR_V3(**cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in recipe.make_state_dict(cfg).items()}, strict=False)
    return m.cuda().eval()


def test_sample_long_with_a_track():
    cfg = recipe.CONFIGS["micro"]
    Cc = cfg["input_channels"]
    st = tstats(Cc, 31)
    bank = LatentBank(Cc, 200)
    bank.add(torch.from_numpy(recipe.gaussian("rate_sl_bank", (Cc, 200), 1)), st)
    m = micro_model()
    total, chunk, ov = 70, 40, 8
    plan = jatsr_amd.chunk_plan(total, chunk, ov)
    lr = cuda(recipe.gaussian("rate_sl_lr", (Cc, total), 1) * 1.3 + 0.2)
    noise = [cuda(recipe.gaussian("rate_sl_noise", (1, Cc, e - s), i)) for i, (s, e) in enumerate(plan)]
    args = (m, lr, st["hr_mean"], st["hr_std"], st["lr_mean"], st["lr_std"])
    kw = dict(num_steps=3, cfg_scale=2.0, chunk_frames=chunk, overlap_frames=ov, noise=noise)
    plain = jatsr_amd.sample_long(*args, **kw)
    scalar = jatsr_amd.sample_long(*args, bank=bank, index_rate=0.4, **kw)
    cls = cuda(np.repeat(np.array([2, 0, 1, 2], np.uint8), 16))           # 64 class frames for 70 latent frames
    rates = RT.rate_track(cls, total, 0.4, protect=0.0, unstable=0.5, smooth=2)
    for k in (1, 4):
        got = jatsr_amd.sample_long(*args, bank=bank, index_rate=0.9, index_k=k, index_rates=rates, **kw)   # the track replaces the scalar
        assert torch.equal(bits(got), bits(bank.retrieve(plain, rates, stats=st, k=k)))
    got = jatsr_amd.sample_long(*args, bank=bank, index_rates=rates[None], **kw)            # index_rate 0 and a track: the track
    assert torch.equal(bits(got)[:, :, :14], bits(scalar)[:, :, :14])     # stable frames farther than S from a change
    assert torch.equal(bits(got)[:, :, 18:30], bits(plain)[:, :, 18:30])  # protect 0: the plain output
    assert torch.equal(bits(got)[:, :, 66:], bits(plain)[:, :, 66:])      # behind the pitch track: unvoiced
    assert not torch.equal(bits(got)[:, :, 34:46], bits(plain)[:, :, 34:46])
    const = jatsr_amd.sample_long(*args, bank=bank, index_rates=torch.full((total,), 0.4, device="cuda"), **kw)
    assert torch.equal(bits(const), bits(scalar))
    assert torch.equal(bits(jatsr_amd.sample_long(*args, bank=bank, index_rates=None, **kw)), bits(plain))
    with pytest.raises(ValueError, match="frames"):
        jatsr_amd.sample_long(*args, bank=bank, index_rates=rates[:-1], **kw)
    with pytest.raises(ValueError, match="needs a bank"):
        jatsr_amd.sample_long(*args, index_rates=rates, **kw)


def test_infer_flags(tmp_path):
    """`--index-protect 1 --index-unstable 1`: every file the run without the flags writes is there with the same bytes, except
    `_idx.pt`, which the issue lets gain `rates`, `f0_classes` and metadata: every entry the plain file holds is in it with the
    same bits.  `--index-protect 0`: the frames classed not live and farther than S from a change hold the plain generated latent."""
    import json

    from jatsr_amd.infer import main as infer_main
    Cc = 1024
    cfg = dict(recipe.CONFIGS["micro"], input_channels=Cc, cond_channels=Cc)
    torch.save({"model_state_dict": {k: torch.from_numpy(v) for k, v in recipe.make_state_dict(cfg).items()},
                "config": dict(cfg)}, tmp_path / "last.pt")
    ones, zeros = [1.0] * Cc, [0.0] * Cc
    stats = {"hr_mean": zeros, "hr_std": ones, "lr_mean": zeros, "lr_std": ones}
    (tmp_path / "stats.json").write_text(json.dumps(stats))
    full = {"decoder." + k: torch.from_numpy(v) for k, v in recipe.make_dac_state_dict().items()}
    full.update({k: torch.from_numpy(v) for k, v in recipe.make_dac_encoder_state_dict().items()})
    torch.save(full, tmp_path / "dac.pt")
    bank = LatentBank(Cc, 120)
    bank.add(torch.from_numpy(recipe.gaussian("rate_inf_bank", (Cc, 120), 1)), {k: torch.tensor(v) for k, v in stats.items()})
    bank.save(tmp_path / "bank.pt")
    # the fixture, then 2 s more of a 220 Hz tone: a file must be longer than the 2 s crossfade to make a chunk
    tail = (0.5 * np.sin(2 * np.pi * 220.0 * np.arange(2 * RR.SR) / RR.SR)).astype(F32)
    jio.write_wav_float32(tmp_path / "song.wav", np.concatenate([RR.fixture_signal(), tail]), RR.SR)
    base = ["--checkpoint", str(tmp_path / "last.pt"), "--stats-file", str(tmp_path / "stats.json"), "--steps", "2", "--seed", "3",
            "--dac-weights", str(tmp_path / "dac.pt"), "--input-audio", str(tmp_path / "song.wav"), "--index-bank",
            str(tmp_path / "bank.pt"), "--index-rate", "0.5"]
    infer_main(base + ["--output-dir", str(tmp_path / "plain")])
    infer_main(base + ["--output-dir", str(tmp_path / "one"), "--index-protect", "1", "--index-unstable", "1"])
    infer_main(base + ["--output-dir", str(tmp_path / "zero"), "--index-protect", "0", "--index-f0-method", "yin"])
    names = sorted(os.listdir(tmp_path / "plain"))
    assert "song_generated_idx.pt" in names and "song_generated_idx.wav" in names
    for d in ("one", "zero"):
        assert sorted(os.listdir(tmp_path / d)) == names
    same = [f for f in names if f != "song_generated_idx.pt" and not f.endswith("_generated.pt")]   # _generated.pt records seconds
    for f in same:
        assert (tmp_path / "plain" / f).read_bytes() == (tmp_path / "one" / f).read_bytes(), f
    load = lambda d, f: torch.load(tmp_path / d / f, weights_only=False)   # noqa: E731
    p, one, zero = (load(d, "song_generated_idx.pt") for d in ("plain", "one", "zero"))
    gen = load("plain", "song_generated.pt")["generated_latent"]
    assert torch.equal(load("one", "song_generated.pt")["generated_latent"], gen)
    for k, v in p.items():
        if k == "metadata":
            assert all(one[k][a] == b for a, b in v.items())
        else:
            assert (torch.equal(one[k], v) if isinstance(v, torch.Tensor) else one[k] == v), k
    T = gen.shape[-1]
    for f in (one, zero):
        assert f["rates"].shape == (T,) and f["rates"].dtype == torch.float32 and f["f0_classes"].shape == (T,)
        assert f["f0_classes"].dtype == torch.uint8
        md = f["metadata"]
        assert set(md) >= {"index_protect", "index_unstable", "index_smooth", "index_f0_method", "voiced_share", "stable_share"}
        assert md["index_smooth"] == 2 and md["index_f0_method"] == "yin" and 0.0 < md["stable_share"] <= md["voiced_share"] < 1.0
        assert not any("speech" in str(k) or "music" in str(k) for k in md)
    assert one["metadata"]["index_protect"] == 1.0 and zero["metadata"]["index_protect"] == 0.0
    assert (one["rates"] == 0.5).all()
    assert "rates" not in p and "index_protect" not in p["metadata"]
    cls = zero["f0_classes"].numpy()
    inner = RR.fixture_inner(RR.FIXTURE_W + 2)                            # farther than S = 2 from a frame that may change class
    seg = np.full(T, -1, np.int64)
    seg[:min(T, len(inner))] = inner[:T]
    assert (cls[seg == 1] == 0).all() and (cls[seg == 0] == 2).all() and (seg == 1).sum() >= 15
    z, rates = zero["generated_latent"], zero["rates"].numpy()
    noise, tone = torch.from_numpy(seg == 1), torch.from_numpy(seg == 0)
    assert torch.equal(z[:, noise], gen[:, noise]) and (rates[seg == 1] == 0).all()
    assert torch.equal(z[:, tone], p["generated_latent"][:, tone]) and (rates[seg == 0] == 0.5).all()
    assert not torch.equal(z[:, tone], gen[:, tone])
