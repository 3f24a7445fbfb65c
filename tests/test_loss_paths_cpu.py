"""Which kernel the v3mod2 loss launches at a sequence length (csrc/train.hip `plan_latent_loss`, reported by
`jat_k_latent_loss_plan`), against a Python restatement of the rule; and proof that the cases of
tests/test_gpu_loss_paths.py (tests/loss_path_cases.py) reach every path and meet their input preconditions.  No GPU."""
import ctypes as C
import os
import subprocess
import sys

import pytest

import jatsr_amd._lib as L
import loss_path_cases as K
from jatsr_amd.io import frames_for_seconds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the A/B switch of the library (read once per process) moves every length to the direct kernel; these tests describe the
# default and say so if the environment differs
DIRECT = os.environ.get("JAT_LOSS_DIRECT_DFT", "0").strip() not in ("", "0")


@pytest.fixture(scope="module", autouse=True)
def built_lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.lib()


def plan(T):
    kind, a, b, lds = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1), C.c_int64(-1)
    L.check(L.lib().jat_k_latent_loss_plan(T, C.byref(kind), C.byref(a), C.byref(b), C.byref(lds)))
    return kind.value, a.value, b.value, lds.value


def test_plan_matches_the_rule_for_every_length_to_7000():
    assert not DIRECT, "unset JAT_LOSS_DIRECT_DFT"
    bad = [(T, plan(T), K.expected_plan(T)) for T in range(1, 7001) if plan(T) != K.expected_plan(T)]
    assert not bad, bad[:10]
    # the landmarks the rule implies: the first composite length whose factored image does not fit, the first rejected one
    composite_direct = [T for T in range(1, 7001) if plan(T)[0] == 1 and not K.is_prime(T) and T > 1]
    assert composite_direct[0] == 3418 and plan(3418)[:3] == (1, 3, 6)
    assert [T for T in range(1, 7001) if plan(T)[0] == 0][0] == K.REJECT_T
    assert all(plan(T)[0] == 0 for T in range(K.REJECT_T, 7001))
    assert all(0 < plan(T)[3] <= K.LDS_LIMIT for T in range(1, K.REJECT_T))
    assert max(plan(T)[3] for T in range(1, K.REJECT_T) if plan(T)[0] == 2) >= plan(4096)[3] == 149128
    # bad arguments are an error, not a plan
    out = [C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()]
    assert L.lib().jat_k_latent_loss_plan(0, *[C.byref(o) for o in out]) == L.JAT_E_INVALID
    assert L.lib().jat_k_latent_loss_plan(8, None, C.byref(out[1]), C.byref(out[2]), C.byref(out[3])) == L.JAT_E_INVALID


def test_length_table_reaches_every_path():
    """Coverage is asserted, not assumed: the plan the LIBRARY reports for each length of the GPU test's table is the path the
    table names, and the union of the classes reached is every launch path and every factor class."""
    assert not DIRECT, "unset JAT_LOSS_DIRECT_DFT"
    reached = {}
    for T, path, _ in K.LENGTHS + K.EXTRA:
        p = plan(T)
        assert p[:3] == ({"direct": 1, "fft": 2}[path[0]],) + path[1:], (T, p, path)
        for c in K.classes_of(T, p):
            reached.setdefault(c, []).append(T)
    for c in K.classes_of(K.REJECT_T, plan(K.REJECT_T)):
        reached.setdefault(c, []).append(K.REJECT_T)
    print({c: reached[c] for c in sorted(reached)})
    assert K.REQUIRED_CLASSES <= set(reached), K.REQUIRED_CLASSES - set(reached)
    table = [T for T, _, _ in K.LENGTHS]
    assert table[-1] == 3418 and 4096 in table and all(T in table for T in K.SWEEP_T)
    assert 1543 == min(T for T in range(2, 7001) if K.is_prime(T)
                       and "direct<3,6> two or more chunks in both loops" in K.classes_of(T, plan(T)))
    # the sweep covers a factored, a one-chunk direct and a chunked direct length
    assert [plan(T)[0] for T in K.SWEEP_T] == [2, 1, 1] and plan(1543)[1:3] == (3, 6)


def test_default_crop_durations_reach_the_direct_kernels():
    """`fit --frames` defaults to frames_for_seconds(target_duration): whole-second crops land on every direct instance."""
    assert not DIRECT, "unset JAT_LOSS_DIRECT_DFT"
    got = {s: plan(frames_for_seconds(s))[:3] for s in (11, 12, 15, 16, 20, 25)}
    assert [frames_for_seconds(s) for s in (11, 12, 15, 16, 20, 25)] == [947, 1033, 1291, 1378, 1722, 2153]
    assert got == {11: (1, 2, 4), 12: (1, 3, 6), 15: (1, 3, 6), 16: (2, 26, 53), 20: (2, 41, 42), 25: (1, 3, 6)}


@pytest.mark.parametrize("T", [T for T, _, _ in K.LENGTHS + K.EXTRA])
def test_case_inputs_meet_the_preconditions(T):
    """The recorded salt is the first one at which the inputs meet the preconditions (for every set of cut-offs the GPU tests
    run the length at), and the special rows are what the table says."""
    import numpy as np
    pred, target, lr = K.make_inputs(T, K.SALT[T])
    for cuts in K.cuts_of_case(T):
        pre = K.preconditions(pred, target, lr, cuts=cuts)
        assert K.preconditions_hold(pre), (T, cuts, pre)
    assert K.search_salt(T) == K.SALT[T]
    assert pred.dtype == target.dtype == lr.dtype == np.float32 and pred.shape == (1, K.rows_for(T), T)
    assert np.array_equal(pred[0, K.TIE], target[0, K.TIE]) and not pred[0, K.ZERO].any()
    assert np.abs(pred[0, K.LOUD]).max() > 100 * np.abs(pred[0, 0]).max() or T < 4


def test_direct_dft_switch_moves_composite_lengths_to_the_direct_kernel():
    """JAT_LOSS_DIRECT_DFT=1 (read once per process): every length plans as the direct kernel, on the same brackets."""
    code = ("import ctypes as C, jatsr_amd._lib as L\n"
            "for T in (8, 128, 1378, 4096, 6822):\n"
            "    o = [C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()]\n"
            "    L.check(L.lib().jat_k_latent_loss_plan(T, *[C.byref(x) for x in o]))\n"
            "    print(T, *[x.value for x in o])\n")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, JAT_LOSS_DIRECT_DFT="1"),
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-1000:]
    got = [tuple(int(v) for v in line.split()) for line in out.stdout.strip().splitlines()]
    assert got == [(T,) + K.expected_plan(T, direct_switch=True) for T in (8, 128, 1378, 4096, 6822)]
    assert [g[1:4] for g in got] == [(1, 1, 2), (1, 1, 2), (1, 3, 6), (1, 3, 6), (0, 0, 0)]
