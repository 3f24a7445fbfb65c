"""The pYIN tracker on the GPU (csrc/pyin.hip, jatsr_amd.pitch.pyin) against its fp64 statement (tests/pyin_ref.py).

pYIN ends in discrete decisions, so the stages are gated apart, each on the GPU's OWN output of the stage before it
(u = 2^-24, N = n_thresholds):
  prob     reference stage 2 on the GPU's cmndf (comparisons of fp32 heights and thresholds are exact in fp64).  The support
           (the trough set) must match with no tolerance.  Values: a term is beta_m A[p] / D[n] from three tables rounded once
           (3 u) and two products (2 u); a sum of at most N non-negative terms in any order adds (N - 1) u; the no-trough
           term has a rounded table entry, a rounded factor, a product and an add (4 u):  |err| <= (N + 9) u P + 1e-35, the
           last for products that leave the normal range (N 2^-126 at most).
  bin      |bin - clip(unrounded fp64 position)| <= 0.5 + 1e-9 on every trough of every frame.  The kernel takes the shift
           and the position in fp64 on the fp32 cmndf with the statement's own operations (sums of two fp32 values, a scaling
           by 2, one divide: the same roundings as numpy's), so the |b| < |a| decision cannot differ; what remains is log2's
           last place, 2^-52 |position| <= 2.3e-13 at position 1024.  1e-9 leaves room for a log2 of a few ulp.
  obs      the scatter of the GPU's own prob and bin (largest lag wins), bit for bit
  voiced_prob  fp64 sum of the GPU's obs: a sum of nnz non-negative terms in any order, |err| <= nnz u sum (adding 0 is exact)
  log_obs  voiced: log(o + FLT_MIN) with one rounded add (u relative in the argument = u absolute in the log) and a logf of
           at most 1.5 ulp (3 u |log|): |err| <= 2 u + 3 u |log|.  unvoiced: the interval that the voiced_prob bound, a
           subtract, a divide and an add (3 u) leave for the argument, widened by the same logf error.
  state    the numpy fp32 replica of stage 5 on the GPU's own log_obs and the library's own tables: every frame, no tolerance
  f0       freqs[state] bit for bit, 0 and unvoiced for the upper half
  fp64     end to end against the fp64 statement the decoded (voiced, bin) may differ on at most 1 % of a case's frames
           (tests/test_pyin_cpu.py shows the fp32 statement differing on none).  voiced_prob: with the trough memberships
           under[i, m] of both sides, every threshold m whose column is the same gives every trough the same term up to
           rounding; a threshold whose column differs moves at most beta_m on either side (its terms sum to beta_m); a bin
           whose winning trough differs moves at most what either side observes there:
             |vp_gpu - vp_64| <= (N + nnz + 12) u + 2 sum_{m differs} beta_m + sum_{b: winner differs} (obs_gpu[b] + obs_64[b])
Every test prints its figures before it asserts.  Measured on MI355X: see DESIGN.md section 21.

The file is named test_pyin_gpu.py, not test_gpu_pyin.py, because tests/fp16_matrix.py needs a row for every
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
import pyin_ref as Y  # noqa: E402
import jatsr_amd._lib as L  # noqa: E402
import jatsr_amd.io as jio  # noqa: E402
import jatsr_amd.pitch as pitch  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
TINY = Y.TINY
NAMES = sorted(P.CASES)
_gpu = {}


def cuda(a):
    return torch.from_numpy(np.array(a)).cuda()            # a copy: the shared cases are read-only


def params(name):
    return Y.params(name) if name != "octave" else {}


def lib_tables(T, **kw):
    """T with the library's own fp64 beta table (`jat_pyin_tables`) in place of the statement's: beta_m is a difference of two
    CDF values near 1 for the upper thresholds, so its last bits are rounding noise of whichever routine made it (both are
    within 1e-13 absolute of each other, tests/test_pyin_cpu.py), and stage 2 is checked against the table the kernel was given"""
    beta = pitch.pyin_handle(**kw).tables()["beta"]
    return dict(T, beta=beta, cum_beta=np.concatenate([[0.0], np.cumsum(beta)]))


def gpu(name):
    """the GPU's outputs for a case, as numpy [B, ...]; computed once"""
    if name not in _gpu:
        r = pitch.pyin_full(cuda(Y.case(name)[0]), want=pitch.PYIN_WANT, **params(name))
        _gpu[name] = {k: v.cpu().numpy() for k, v in r.items()}
    return _gpu[name]


@pytest.mark.parametrize("name", NAMES)
def test_prob_and_bin_on_the_gpus_own_cmndf(name):
    T = lib_tables(Y.case_tables(name), **params(name))
    g = gpu(name)
    N, nb = T["N"], T["n_bins"]
    for b in range(g["cmndf"].shape[0]):
        c = g["cmndf"][b]
        tr = Y.troughs(c[:, T["lo"]:T["hi"] + 1].astype(np.float64))
        want = Y.probs(c, T, np.float64)
        got = g["prob"][b].astype(np.float64)
        err = np.abs(got - want)
        rel = float((err[tr] / np.maximum(want[tr], 1e-300)).max()) if tr.any() else 0.0
        pos = np.clip(Y.bin_positions(c, T), 0, nb - 1)
        off = float(np.abs(g["bin"][b] - pos)[tr].max()) if tr.any() else 0.0
        print(f"{name}[{b}]: {int(tr.sum())} troughs, at most {int(tr.sum(axis=1).max())} a frame; prob rel {rel:.2e} (gate "
              f"{(N + 9) * U:.2e}); |bin - position| {off:.6f} (gate 0.5 + 1e-9)")
        assert g["prob"][b].dtype == np.float32 and g["bin"][b].dtype == np.int32
        assert np.array_equal(g["bin"][b] >= 0, tr) and (got[~tr] == 0).all() and (got >= 0).all()     # the support, exactly
        assert (err <= (N + 9) * U * want + 1e-35).all()
        assert (np.abs(g["bin"][b] - pos)[tr] <= 0.5 + 1e-9).all()
        assert (g["bin"][b][tr] >= 0).all() and (g["bin"][b][tr] < nb).all() and (g["bin"][b][~tr] == -1).all()


@pytest.mark.parametrize("name", NAMES)
def test_obs_voiced_prob_and_log_obs_on_the_gpus_own_stage_before(name):
    T = Y.case_tables(name)
    g = gpu(name)
    nb = T["n_bins"]
    for b in range(g["obs"].shape[0]):
        obs = g["obs"][b]
        assert obs.tobytes() == Y.scatter(g["prob"][b], g["bin"][b], nb).tobytes()                   # bit for bit
        o64 = obs.astype(np.float64)
        s64, nnz = o64.sum(axis=1), (obs != 0).sum(axis=1)
        vp64 = np.clip(s64, 0, 1)
        dv = nnz * U * s64
        vp = g["voiced_prob"][b].astype(np.float64)
        lo = g["log_obs"][b].astype(np.float64)
        ref_v = np.log(o64 + TINY)
        err_v = np.abs(lo[:, :nb] - ref_v)
        hi_arg = (1 - np.maximum(vp64 - dv, 0)) / nb * (1 + 3 * U) + TINY * (1 + U)
        lo_arg = np.maximum((1 - np.minimum(vp64 + dv, 1)) / nb * (1 - 3 * U), 0) + TINY * (1 - U)
        slack = lambda v: 2 * U + 3 * U * np.abs(v)  # noqa: E731
        print(f"{name}[{b}]: voiced_prob err {np.abs(vp - vp64).max():.2e} (gate {dv.max():.2e}); log_obs voiced err "
              f"{err_v.max():.2e} (gate {slack(ref_v).max():.2e}); unvoiced in [{np.log(lo_arg).min():.3f}, {np.log(hi_arg).max():.3f}]")
        assert (np.abs(vp - vp64) <= dv).all() and (vp >= 0).all() and (vp <= 1).all()
        assert (err_v <= slack(ref_v)).all()
        assert (lo[:, nb] >= np.log(lo_arg) - slack(np.log(lo_arg))).all() and (lo[:, nb] <= np.log(hi_arg) + slack(np.log(hi_arg))).all()


@pytest.mark.parametrize("name", NAMES + ["octave"])
def test_state_is_the_fp32_replica_on_the_gpus_own_log_obs(name):
    T = Y.case_tables(name)
    g = gpu(name)
    t = pitch.pyin_handle(**params(name)).tables()
    nb = T["n_bins"]
    for b in range(g["state"].shape[0]):
        want = Y.viterbi(g["log_obs"][b], T, np.float32, (t["logw"], t["logZ"], t["lk"], t["ls"], t["logpi"]))
        st = g["state"][b]
        print(f"{name}[{b}]: {st.shape[0]} frames, {int((st < nb).sum())} voiced, state differs on {int((st != want).sum())}")
        assert st.dtype == np.int32 and np.array_equal(st, want)
        assert np.array_equal(g["voiced"][b], (st < nb).astype(np.uint8))
        f0 = np.where(st < nb, t["freqs"][np.minimum(st, nb - 1)], np.float32(0)).astype(np.float32)
        assert g["f0"][b].tobytes() == f0.tobytes()


def _vp_bound(c_gpu, obs_gpu, bin_gpu, ref, c64, T):
    """the end-to-end voiced_prob bound of the module docstring, per frame"""
    lo, hi, N, nb = T["lo"], T["hi"], T["N"], T["n_bins"]
    out = np.zeros(c_gpu.shape[0])
    for f in range(c_gpu.shape[0]):
        ya, yb = c_gpu[f:f + 1, lo:hi + 1].astype(np.float64), c64[f:f + 1, lo:hi + 1]
        ua = (Y.troughs(ya)[0] & True)[:, None] & (ya[0][:, None] < T["theta"][None, :])
        ub = Y.troughs(yb)[0][:, None] & (yb[0][:, None] < T["theta"][None, :])
        cols = (ua != ub).any(axis=0)
        wa, wb = np.full(nb, -1), np.full(nb, -1)
        for w, bins in ((wa, bin_gpu[f]), (wb, ref["bin"][f])):
            idx = np.flatnonzero(bins >= 0)
            np.maximum.at(w, bins[idx], idx)
        moved = wa != wb
        nnz = int((obs_gpu[f] != 0).sum())
        out[f] = (N + nnz + 12) * U + 2 * T["beta"][cols].sum() + (obs_gpu[f].astype(np.float64) + ref["obs"][f])[moved].sum()
    return out


@pytest.mark.parametrize("name", NAMES + ["octave"])
def test_end_to_end_against_the_fp64_statement(name):
    T = Y.case_tables(name)
    x, r64, _ = Y.case(name)
    y64 = P.case(name)[1] if name != "octave" else [P.yin(x[0])]
    g = gpu(name)
    nb = T["n_bins"]
    for b, a in enumerate(r64):
        st = g["state"][b]
        mine = dict(voiced=st < nb, track_bin=np.where(st < nb, st, -1))
        frames = st.shape[0]
        differ = Y.same_track(mine, a)
        bound = _vp_bound(g["cmndf"][b], g["obs"][b], g["bin"][b], a, y64[b]["cmndf"], T)
        err = np.abs(g["voiced_prob"][b].astype(np.float64) - a["voiced_prob"])
        print(f"{name}[{b}]: (voiced, bin) differs on {differ} of {frames} frames (cap {0.01 * frames:.2f}); voiced_prob err "
              f"{err.max():.2e}, {int((bound > 1e-4).sum())} frames with a structural term, worst err / bound {float((err / bound).max()):.3f}")
        assert differ <= 0.01 * frames
        assert (err <= bound).all()


def test_octave_signal_pyin_holds_where_yin_drops():
    x = cuda(Y.octave_signal())
    f0, voiced, vp = pitch.pyin(x)
    fy, _, _ = pitch.yin(x)
    inner = slice(3, -3)
    f0, voiced, fy = f0.cpu().numpy(), voiced.cpu().numpy(), fy.cpu().numpy()
    off = np.abs(P.cents(np.where(voiced, f0, 1.0), 220.0))[inner]
    off_yin = np.abs(P.cents(fy, 220.0))[inner]
    print(f"{off.shape[0]} inner frames: yin > 600 cents on {int((off_yin > 600).sum())}; pyin voiced on {int(voiced[inner].sum())}, "
          f"worst {off.max():.4f} cents")
    assert off.shape[0] == 38 and (off_yin > 600).sum() >= 3
    assert voiced[inner].all() and (off < 5.05).all()                    # half a bin: see tests/test_pyin_cpu.py
    assert vp.dtype == torch.float32 and float(vp.min()) >= 0 and float(vp.max()) <= 1


def _raw(h, x, B, n, guard=96, short_by=0, null=()):
    """jat_pyin_track straight through the ABI into buffers with guard bands on both sides -> (rc, payloads, guards_intact,
    untouched)"""
    frames, ny = 1 + n // h.hop_length, h.max_period - h.min_period + 1
    BF = B * frames
    spec = {"f0": (torch.float32, BF), "voiced": (torch.uint8, BF), "voiced_prob": (torch.float32, BF),
            "cmndf": (torch.float32, BF * (h.max_period + 1)), "prob": (torch.float32, BF * ny), "bin": (torch.int32, BF * ny),
            "obs": (torch.float32, BF * h.n_bins), "log_obs": (torch.float32, BF * (h.n_bins + 1)), "state": (torch.int32, BF),
            "work": (torch.uint8, h.workspace_bytes(B, n) - short_by)}
    bufs = {}
    for k, (dt, m) in spec.items():
        t = torch.empty(m + 2 * guard, dtype=dt, device="cuda")
        t.fill_(77)
        bufs[k] = t
    ptr = {k: (C.c_void_p(t.data_ptr() + guard * t.element_size()) if k not in null else None) for k, t in bufs.items()}
    assert (bufs["work"].data_ptr() + guard) % 16 == 0
    order = ("f0", "voiced", "voiced_prob") + pitch.PYIN_WANT
    rc = L.lib().jat_pyin_track(h.h, L.ptr(x) if "x" not in null else None, B, n, *(ptr[k] for k in order), ptr["work"],
                                spec["work"][1], L.stream_ptr())
    torch.cuda.synchronize()
    intact = all(bool((t[:guard] == 77).all()) and bool((t[-guard:] == 77).all()) for t in bufs.values())
    untouched = all(bool((t == 77).all()) for t in bufs.values())
    return rc, {k: t[guard:-guard].cpu().numpy() for k, t in bufs.items() if k != "work"}, intact, untouched


def test_determinism_batch_independence_guard_bands_and_zeros():
    name = "defaults"
    x = cuda(Y.case(name)[0])
    n = x.shape[1]
    g = gpu(name)
    again = pitch.pyin_full(x, want=pitch.PYIN_WANT, **params(name))
    for k, v in again.items():
        assert v.cpu().numpy().tobytes() == g[k].tobytes(), k               # run to run
    alone = pitch.pyin_full(x[1].clone(), want=pitch.PYIN_WANT, **params(name))
    for k, v in alone.items():
        assert v.cpu().numpy().tobytes() == g[k][1].tobytes(), k            # a row alone and inside a batch
    f0, voiced, vp = pitch.pyin(x, **params(name))
    assert voiced.dtype == torch.bool and f0.shape == voiced.shape == vp.shape == (3, 1 + n // 512)
    assert f0.cpu().numpy().tobytes() == g["f0"].tobytes() and vp.cpu().numpy().tobytes() == g["voiced_prob"].tobytes()
    plain = pitch.pyin_full(x, **params(name))                              # the nullable outputs left out
    assert sorted(plain) == ["f0", "voiced", "voiced_prob"] and plain["f0"].cpu().numpy().tobytes() == g["f0"].tobytes()
    # guard bands around every output and the workspace
    h = pitch.pyin_handle(**params(name))
    rc, out, intact, _ = _raw(h, x, 3, n)
    assert rc == 0 and intact
    for k, v in out.items():
        assert v.tobytes() == g[k].tobytes(), k
    short = "short"
    hs = pitch.pyin_handle(**params(short))
    xs = cuda(Y.case(short)[0])
    rc, out, intact, _ = _raw(hs, xs, 1, xs.shape[1])
    assert rc == 0 and intact and out["state"].tobytes() == gpu(short)["state"].tobytes()
    # zeros: no trough anywhere, every frame unvoiced; one frame only (L < hop): the decoder's first step alone
    z = pitch.pyin_full(torch.zeros(5000, device="cuda"), want=("prob", "bin", "obs", "state"))
    assert not z["voiced"].any() and (z["f0"] == 0).all() and (z["voiced_prob"] == 0).all()
    assert (z["prob"] == 0).all() and (z["bin"] == -1).all() and (z["obs"] == 0).all() and (z["state"] >= h.n_bins).all()
    one = pitch.pyin_full(cuda(P.mix(44100, 300, 0)), want=("state", "log_obs"))
    lo1 = one["log_obs"][0].cpu().numpy()
    v0 = np.concatenate([lo1[:-1], np.full(h.n_bins, lo1[-1], np.float32)]) + h.tables()["logpi"]          # fp32, one add
    assert one["state"].shape == (1,) and v0.dtype == np.float32 and int(one["state"][0]) == int(np.argmax(v0))


def test_refusals_through_the_abi():
    """every refusal of jat_pyin_track: a code and a message, never a fault, and nothing is written"""
    h = pitch.pyin_handle()
    x = torch.zeros(2, 4096, device="cuda")
    assert _raw(h, x, 2, 4096)[0] == 0
    for B, n in ((0, 4096), (-1, 4096), (65536, 4096), (1, 0), (1, -4), (1, 2 ** 40)):
        sz = C.c_size_t(7)
        assert L.lib().jat_pyin_workspace_bytes(h.h, B, n, C.byref(sz)) == L.JAT_E_INVALID and sz.value == 7
        f = torch.full((64,), 5.0, device="cuda")
        rc = L.lib().jat_pyin_track(h.h, L.ptr(x), B, n, L.ptr(f), L.ptr(f), L.ptr(f), None, None, None, None, None, None, L.ptr(f),
                                    256, L.stream_ptr())
        torch.cuda.synchronize()
        assert rc == L.JAT_E_INVALID and bool((f == 5).all()) and L.lib().jat_last_error(), (B, n)
    for null in ("x", "f0", "voiced", "voiced_prob", "work"):
        rc, _, _, untouched = _raw(h, x, 2, 4096, null=(null,))
        assert rc == L.JAT_E_INVALID and untouched, null
    rc, _, _, untouched = _raw(h, x, 2, 4096, short_by=1)
    assert rc == L.JAT_E_STATE and untouched and b"workspace" in L.lib().jat_last_error()
    with pytest.raises(ValueError, match="resolution"):
        pitch.pyin(x, resolution=0.0)
    with pytest.raises(ValueError, match="n_thresholds"):
        pitch.pyin(x, n_thresholds=0)
    with pytest.raises(TypeError, match="unknown"):
        pitch.pyin(x, trough_threshold=0.1)
    with pytest.raises(L.JatError, match="float32"):
        pitch.pyin(x.double())
    with pytest.raises(L.JatError, match="CUDA"):
        pitch.pyin(x.cpu())
    with pytest.raises(ValueError, match="method"):
        pitch.f0_metrics(x[0], x[1], method="crepe")
    with pytest.raises(TypeError, match="pyin"):
        pitch.f0_metrics(x[0], x[1], resolution=0.2)


def test_a_second_parameter_set_through_the_public_function():
    """other prior parameters (fewer thresholds, a coarser grid, a flatter prior) against the statement, stage by stage"""
    kw = dict(n_thresholds=37, beta_parameters=(1.5, 6.0), boltzmann_parameter=0.7, resolution=0.25, max_transition_rate=20.0,
              switch_prob=0.05, no_trough_prob=0.03)
    x = P.mix(44100, 20000, 5)
    T = lib_tables(Y.tables(**kw), **kw)
    r = {k: v.cpu().numpy() for k, v in pitch.pyin_full(cuda(x), want=pitch.PYIN_WANT, **kw).items()}
    h = pitch.pyin_handle(**kw)
    t = h.tables()
    assert (h.n_bins, h.H) == (T["n_bins"], T["H"])
    want = Y.probs(r["cmndf"], T, np.float64)
    assert (np.abs(r["prob"] - want) <= (37 + 9) * U * want + 1e-35).all()
    assert np.array_equal(r["bin"] >= 0, Y.troughs(r["cmndf"][:, T["lo"]:T["hi"] + 1].astype(np.float64))) and (r["bin"] >= 0).any()
    assert r["obs"].tobytes() == Y.scatter(r["prob"], r["bin"], T["n_bins"]).tobytes()
    st = Y.viterbi(r["log_obs"], T, np.float32, (t["logw"], t["logZ"], t["lk"], t["ls"], t["logpi"]))
    assert np.array_equal(r["state"], st) and (r["state"] < T["n_bins"]).any() and (r["state"] >= T["n_bins"]).any()


def _decode(lo, T, t):
    """the Viterbi stage alone on constructed log observations: the GPU's states, which must be the fp32 replica's"""
    got = pitch.pyin_decode(cuda(lo))
    st = got["state"].cpu().numpy()
    want = Y.viterbi(lo, T, np.float32, (t["logw"], t["logZ"], t["lk"], t["ls"], t["logpi"]))
    assert np.array_equal(st, want), (st, want)
    nb = T["n_bins"]
    assert np.array_equal(got["voiced"].cpu().numpy(), (st < nb).astype(np.uint8))
    assert got["f0"].cpu().numpy().tobytes() == np.where(st < nb, t["freqs"][np.minimum(st, nb - 1)], np.float32(0)).astype(np.float32).tobytes()
    return st


def test_viterbi_tie_rules_on_constructed_log_obs():
    """Exact ties do not occur on the test signals, so the three tie rules of stage 5 are driven by constructed log
    observations through `jat_pyin_decode`, and the expected states are written out, not only taken from the replica.
      window     logw is symmetric and logZ is the same for interior bins, so two equal sources at b - d and b + d tie
                 exactly for the target b: the lowest source, b - d, must be followed back
      halves     the voiced value a of frame 0 is searched (a few fp32 neighbours of c + ls - lk) until
                 M_same + lk == M_other + ls holds in fp32 for the target that the track ends in: a voiced target, then an
                 unvoiced one; the voiced source must win both"""
    T = Y.case_tables("octave")
    t = pitch.pyin_handle().tables()
    nb, H = T["n_bins"], T["H"]
    f32, LOW = np.float32, np.float32(-80.0)
    logw, logZ, lk, ls, logpi = t["logw"], t["logZ"], t["lk"], t["ls"], t["logpi"]
    b, d = 260, 7
    lo = np.full((2, nb + 1), LOW, f32)
    lo[0, b - d] = lo[0, b + d] = lo[1, b] = -1.0
    assert logw[H - d] == logw[H + d] and logZ[b - d] == logZ[b + d]
    st = _decode(lo, T, t)
    print("window tie:", st)
    assert st.tolist() == [b - d, b]

    def search(fn, other, start):
        """-> (a, below): fp32 a near `start` with fn(a) == other, and the next fp32 value under it with fn(below) < other"""
        a = f32(start)
        for _ in range(4000):
            v = fn(a)
            if v == other:
                below = a
                while fn(below) == other:
                    below = np.nextafter(below, f32(-np.inf))
                return a, below
            a = np.nextafter(a, f32(np.inf) if v < other else f32(-np.inf))
        raise AssertionError("no fp32 value gives an exact tie")

    c = f32(-3.0)
    # voiced target b: same = ((a + logpi) - logZ[b]) + lk against other = ((c + logpi) - logZ[b]) + ls
    other = ((c + logpi) - logZ[b]) + ls
    a, below = search(lambda v: ((v + logpi) - logZ[b]) + lk, other, ((other - lk) + logZ[b]) - logpi)
    lo = np.full((2, nb + 1), LOW, f32)
    lo[0, b], lo[0, nb], lo[1, b] = a, c, -1.0
    st = _decode(lo, T, t)
    print("halves tie, voiced target: a =", a, st)
    assert st.tolist() == [b, b]
    lo[0, b] = below                                         # the next value lower and the unvoiced source wins: the tie was exact
    assert _decode(lo, T, t).tolist() == [nb + b, b]
    # unvoiced target s: the track ends in the unvoiced state the replica names; same = M_1[s] + lk, other = M_0[s] + ls
    lo = np.full((2, nb + 1), LOW, f32)
    lo[0, nb], lo[1, nb] = c, -1.0
    s_end = int(_decode(lo, T, t)[1]) - nb
    U1 = np.full(nb + 2 * H, -np.inf, f32)
    U1[H:H + nb] = (c + logpi) - logZ
    same = (U1[s_end:s_end + 2 * H + 1] + logw[::-1]).max() + lk
    a, below = search(lambda v: ((v + logpi) - logZ[s_end]) + ls, same, ((same - ls) + logZ[s_end]) - logpi)
    lo[0, s_end] = a
    st = _decode(lo, T, t)
    print("halves tie, unvoiced target:", s_end, "a =", a, st)
    assert 0 <= s_end < nb and st.tolist() == [s_end, nb + s_end]
    lo[0, s_end] = below
    assert int(_decode(lo, T, t)[0]) >= nb


def test_a_handle_serves_one_device():
    assert pitch.pyin_handle(device="cuda") is pitch.pyin_handle(device=f"cuda:{torch.cuda.current_device()}")
    assert pitch.pyin_handle(device="cuda") is not pitch.pyin_handle()
    x = torch.zeros(4096, device="cuda")
    pitch.pyin(x)
    if torch.cuda.device_count() > 1:                         # the library refuses a handle whose tables are elsewhere
        h = pitch.pyin_handle(device="cuda")
        other = (torch.cuda.current_device() + 1) % torch.cuda.device_count()
        with torch.cuda.device(other):
            y = torch.zeros(1, 4096, device="cuda")
            out = torch.zeros(3, 16, device="cuda")
            work = torch.zeros(h.workspace_bytes(1, 4096), dtype=torch.uint8, device="cuda")
            rc = L.lib().jat_pyin_track(h.h, L.ptr(y), 1, 4096, L.ptr(out[0]), L.ptr(out[1]), L.ptr(out[2]), None, None, None, None,
                                        None, None, L.ptr(work), work.numel(), L.stream_ptr())
            assert rc == L.JAT_E_STATE and b"device" in L.lib().jat_last_error()
            f0, voiced, _ = pitch.pyin(y[0])                  # the public function takes that device's own handle
            assert f0.device.index == other and not voiced.any()


def test_fp16_library_gives_the_same_bits(tmp_path):
    code = ("import sys, numpy as np, torch\n"
            "sys.path.insert(0, 'tests')\n"
            "import jatsr_amd._lib as L\n"
            "import jatsr_amd.pitch as pitch\n"
            "import pitch_ref as P\n"
            "assert L.operand_dtype() == sys.argv[2]\n"
            "x = torch.from_numpy(np.stack([P.mix(16000, 16000 + 5, s, 1024) for s in (0, 1)])).cuda()\n"
            "r = pitch.pyin_full(x, 16000, 40.0, 800.0, 1024, 256, want=pitch.PYIN_WANT)\n"
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
    assert sorted(got["bf16"]) == sorted(got["fp16"]) and len(got["bf16"]) == 9
    for k, v in got["bf16"].items():
        assert v.tobytes() == got["fp16"][k].tobytes(), k
    assert (got["fp16"]["state"] < 519).any()


def test_f0_metrics_with_pyin_and_the_command_line(tmp_path, capsys):
    sr, n = 44100, 44100
    gt = P.mix(sr, n, 0)
    pred = (gt + 0.02 * np.random.default_rng(3).standard_normal(n)).astype(np.float32)
    low = P.mix(sr, n - 300, 1)
    tracks = {}
    rep = pitch.f0_metrics(cuda(pred), cuda(gt), cuda(low), method="pyin", tracks=tracks)
    assert sorted(rep) == ["generated", "lr_input"] and sorted(tracks) == ["gt", "lr", "pred"]
    tp, tg = (pitch.pyin(cuda(v[:n])) for v in (pred, gt))
    assert torch.equal(tracks["pred"][0].reshape(-1), tp[0]) and torch.equal(tracks["gt"][0].reshape(-1), tg[0])   # one launch for the pair
    counts = P.compare_counts(tp[0].cpu().numpy(), tp[1].cpu().numpy(), tg[0].cpu().numpy(), tg[1].cpu().numpy())
    want = pitch.report_from_counts(counts, 1 + n // 512)
    print("pyin generated:", rep["generated"])
    for k in pitch.COUNT_KEYS:
        assert rep["generated"][k] == want[k], k
    for k in pitch.RATE_KEYS:
        assert abs(rep["generated"][k] - want[k]) <= 1e-6 * abs(want[k]), k
    assert rep["generated"]["raw_pitch_accuracy"] > 0.9 and 0 < rep["generated"]["n_ref_voiced"] < rep["generated"]["n_frames"]
    assert rep["lr_input"]["n_frames"] == 1 + (n - 300) // 512
    yin_rep = pitch.f0_metrics(cuda(pred), cuda(gt), cuda(low))
    assert yin_rep == pitch.f0_metrics(cuda(pred), cuda(gt), cuda(low), method="yin") and yin_rep != rep
    for name, v in (("pred", pred), ("gt", gt), ("low", low)):
        jio.write_wav_float32(tmp_path / f"{name}.wav", v, sr)
    argv = ["--pred", str(tmp_path / "pred.wav"), "--gt", str(tmp_path / "gt.wav"), "--lr", str(tmp_path / "low.wav")]
    capsys.readouterr()
    out = pitch.main(argv + ["--method", "pyin", "--json", str(tmp_path / "rep.json"), "--track", str(tmp_path / "track.npy")])
    text = capsys.readouterr().out
    assert out == rep and json.loads((tmp_path / "rep.json").read_text()) == rep and "F0 (pYIN) vs GT" in text
    track = np.load(tmp_path / "track.npy")
    assert track.shape == (6, 1 + (n - 300) // 512) and np.array_equal(track[2], tg[0].cpu().numpy()[:track.shape[1]])
    assert pitch.main(argv) == yin_rep
    plain = capsys.readouterr().out
    assert pitch.main(argv + ["--method", "yin"]) == yin_rep and capsys.readouterr().out == plain and "F0 (YIN) vs GT" in plain


def test_infer_f0_method_flag(tmp_path):
    """the synthetic codec and checkpoint of tests/test_gpu_metrics.py: the flag changes the "f0" entry and nothing else"""
    from test_gpu_metrics import _infer_setup
    from jatsr_amd.infer import main as infer_main
    from jatsr_amd import metrics
    base = _infer_setup(tmp_path)
    infer_main(base + ["--output-dir", str(tmp_path / "y"), "--metrics", "--f0-metrics"])
    infer_main(base + ["--output-dir", str(tmp_path / "yy"), "--metrics", "--f0-metrics", "--f0-method", "yin"])
    infer_main(base + ["--output-dir", str(tmp_path / "p"), "--metrics", "--f0-metrics", "--f0-method", "pyin"])
    infer_main(base + ["--output-dir", str(tmp_path / "n"), "--metrics", "--f0-method", "pyin"])          # no --f0-metrics: no effect
    infer_main(base + ["--output-dir", str(tmp_path / "m"), "--metrics"])
    names = sorted(os.listdir(tmp_path / "y"))
    for d in ("yy", "p", "n", "m"):
        assert sorted(os.listdir(tmp_path / d)) == names
    for name in (n for n in names if not n.endswith(".pt")):                # a saved tensor file is not byte-stable from run to run
        assert (tmp_path / "yy" / name).read_bytes() == (tmp_path / "y" / name).read_bytes(), name
        assert (tmp_path / "n" / name).read_bytes() == (tmp_path / "m" / name).read_bytes(), name
        if not name.endswith(".json"):
            assert (tmp_path / "p" / name).read_bytes() == (tmp_path / "y" / name).read_bytes(), name
    y, p = (json.loads((tmp_path / d / "song_metrics.json").read_text()) for d in ("y", "p"))
    assert "method" not in y["f0"] and p["f0"]["method"] == "pyin" and {k: v for k, v in p.items() if k != "f0"} == {k: v for k, v in y.items() if k != "f0"}
    gen, hr, lr = (metrics.load_audio(tmp_path / "p" / n)[0] for n in ("song_generated.wav", "song_hr_gt.wav", "song_lr_input.wav"))
    assert {k: v for k, v in p["f0"].items() if k != "method"} == pitch.f0_metrics(gen, hr, lr, method="pyin")
    assert sorted(p["f0"]) == ["generated", "lr_input", "method"]


def test_prepare_f0_method_flag(tmp_path):
    """the WAVs and the synthetic codec of tests/test_gpu_prepare.py: `--f0 --f0-method pyin` stores the pYIN track and
    hr_voiced_prob; the readers ignore the new key; `--f0-method` without `--f0`, or `yin`, changes nothing"""
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
    prepare_main(argv + ["--output-dir", str(tmp_path / "noeffect"), "--f0-method", "pyin"])
    prepare_main(argv + ["--output-dir", str(tmp_path / "yin"), "--f0"])
    prepare_main(argv + ["--output-dir", str(tmp_path / "yin2"), "--f0", "--f0-method", "yin"])
    prepare_main(argv + ["--output-dir", str(tmp_path / "pyin"), "--f0", "--f0-method", "pyin"])
    codec = load_dac_codec(str(tmp_path / "dac.pt"))
    for stem in ("a", "b"):
        load = lambda d: torch.load(tmp_path / d / "train" / f"{stem}.pt", weights_only=False)  # noqa: E731
        a, ne, y, y2, b = (load(d) for d in ("plain", "noeffect", "yin", "yin2", "pyin"))
        assert sorted(ne) == sorted(a) and sorted(y2) == sorted(y) == sorted(list(a) + ["hr_f0", "hr_voiced"])
        assert all(torch.equal(y[k], y2[k]) for k in ("hr_latent", "lr_latent", "hr_f0", "hr_voiced"))
        assert sorted(b) == sorted(list(y) + ["hr_voiced_prob"])
        assert all(torch.equal(a[k], b[k]) for k in ("hr_latent", "lr_latent")) and a["metadata"] == b["metadata"]
        T = a["hr_latent"].shape[1]
        assert b["hr_voiced_prob"].shape == (T,) and b["hr_voiced_prob"].dtype == torch.float32 and not b["hr_voiced_prob"].is_cuda
        assert b["hr_f0"].dtype == torch.float32 and b["hr_voiced"].dtype == torch.uint8
        x, sr = jio.read_wav(tmp_path / "wav" / f"{stem}.wav")
        f0, voiced, prob = hr_pitch_track(torch.from_numpy(x).cuda(), sr, codec, T, "pyin")
        assert torch.equal(f0.cpu(), b["hr_f0"]) and torch.equal(voiced.cpu(), b["hr_voiced"]) and torch.equal(prob.cpu(), b["hr_voiced_prob"])
        assert ((b["hr_f0"] == 0) == (b["hr_voiced"] == 0)).all()
        hr, lr = jio.load_latent_file(tmp_path / "pyin" / "train" / f"{stem}.pt")
        assert torch.equal(hr, a["hr_latent"].float()) and torch.equal(lr, a["lr_latent"].float())
    store = LatentStore(tmp_path / "pyin", "train", frames=8)
    assert len(store) == 2 and store.lengths == LatentStore(tmp_path / "plain", "train", frames=8).lengths
