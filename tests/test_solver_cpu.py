"""Solvers and time grids of the sampler, host side (no GPU): the fp64 twin (tests/solver_ref.py) against the oracle's Euler
sampler and against hand-written one-step formulas, `jat_solver_plan` against the twin's plan field by field, the grids it must
reject, and the conditioning of the inputs that tests/test_gpu_solvers.py runs on the GPU."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import jatsr_amd._lib as L
import jatsr_amd.recipe as recipe
from jatsr_amd.sampler import SOLVERS, SolverEval, solver_plan
from oracle import jat_oracle as O

import solver_ref as R


@pytest.fixture(scope="module", autouse=True)
def built_lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.lib()


@pytest.mark.parametrize("cfg_scale", [3.0, 1.0])
def test_twin_euler_is_the_oracle_sampler(cfg_scale):
    cfg = recipe.CONFIGS["micro"]
    model = O.OracleModel(cfg, recipe.make_state_dict(cfg), "rms", np.float64)
    lr = recipe.gaussian("lr_latent", (1, 32, 16), 910)
    z0 = recipe.gaussian("z0", (1, 32, 16), 911)
    want = O.flow_matching_sample(model, lr, z0, 3, cfg_scale)
    got = R.flow_matching_sample(model, lr, z0, O.linspace_f32(0.0, 1.0, 4), "euler", cfg_scale)
    assert np.array_equal(got, want)
    assert np.array_equal(R.flow_matching_sample(model, lr, z0, None, "euler", cfg_scale, num_steps=3), want)


def test_one_step_midpoint_and_heun_by_hand():
    """Toy scalar predictor x^(z, t) = 0.3 z + t + 1 in fp64; every time and coefficient is the fp32 value of the definitions."""
    f32 = np.float32

    def pred(z, t):
        return 0.3 * z + float(t) + 1.0

    def den(t):
        return float(f32(f32(f32(1) - f32(t)) + f32(1e-5)))

    z0 = np.array([0.7, -1.25])
    # midpoint, one step over [0, 1]: t = 0, dt = 1, h = 0.5, t2 = 0.5 < 0.999
    zt = z0 + 0.5 * (pred(z0, 0.0) - z0) / den(0.0)
    want = z0 + 1.0 * (pred(zt, 0.5) - zt) / den(0.5)
    got = R.sample(pred, z0, np.array([0, 1], f32), "midpoint")
    assert np.array_equal(got, want)
    # heun over [0, 0.5, 1]: the first step in two stages (t2 = 0.5), the second (t2 = 1) is the reference's Euler step at t = 0.5
    zt = z0 + 0.5 * (pred(z0, 0.0) - z0) / den(0.0)
    z1 = 0.5 * z0 + 0.5 * zt + 0.25 * (pred(zt, 0.5) - zt) / den(0.5)
    want = z1 + (pred(z1, 0.5) - z1) / den(0.5) * 0.5
    got = R.sample(pred, z0, np.array([0, 0.5, 1], f32), "heun")
    assert np.array_equal(got, want)
    # one Heun step over [0, 1] has t2 = 1: the reference's Euler step, one evaluation
    assert np.array_equal(R.sample(pred, z0, np.array([0, 1], f32), "heun"), z0 + (pred(z0, 0.0) - z0) / den(0.0) * 1.0)
    # and the last-steps branch of the reference: from t >= 0.999 on, z' = x^
    ts = np.array([0, 0.9995, 1], f32)
    z1 = z0 + (pred(z0, 0.0) - z0) / den(0.0) * float(ts[1])
    assert np.array_equal(R.sample(pred, z0, ts, "euler"), pred(z1, ts[1]))


FALLBACK = np.array([0.0, 0.5, 0.9988, 0.9996, 1.0], np.float32)   # the last two steps have t2 >= 0.999 for both two-stage solvers
GRIDS = {f"linspace{n}": O.linspace_f32(0.0, 1.0, n + 1) for n in (1, 2, 4, 50)}
GRIDS.update(nonuniform=R.NONUNIFORM, fallback=FALLBACK)
FIELDS = [n for n, _ in SolverEval._fields_]


def _bits(v):
    return np.asarray(v, np.float32).view(np.uint32).tolist()


@pytest.mark.parametrize("solver", sorted(SOLVERS))
@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_library_plan_equals_the_twin(grid, solver):
    ts = GRIDS[grid]
    want, want_distinct = R.plan(ts, solver)
    got, got_distinct = solver_plan(solver, ts)
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        for f in FIELDS:
            if isinstance(w[f], np.float32):
                assert _bits(getattr(g, f)) == _bits(w[f]), (k, f, getattr(g, f), w[f])
            else:
                assert getattr(g, f) == w[f], (k, f)
    assert _bits(got_distinct) == _bits(want_distinct)
    N = len(ts) - 1
    if grid.startswith("linspace"):
        assert len(got) == {"euler": N, "midpoint": 2 * N, "heun": 2 * N - 1}[solver]
        # the default grid (times == NULL) is the same pinned linspace
        dflt, dflt_distinct = solver_plan(solver, None, N)
        assert [[getattr(e, f) for f in FIELDS] for e in dflt] == [[getattr(e, f) for f in FIELDS] for e in got]
        assert _bits(dflt_distinct) == _bits(got_distinct)
    if grid == "fallback":
        assert len(got) == {"euler": 4, "midpoint": 6, "heun": 6}[solver]
        assert [e.stage for e in got][-2:] == [0, 0] and got[-1].direct == 1 and got[-2].direct == 0
    euler_distinct = solver_plan("euler", ts)[1]
    assert _bits(euler_distinct) == _bits(ts[:-1])
    if solver == "heun":       # Heun's second time is the next step's first
        assert _bits(got_distinct) == _bits(euler_distinct)
    if solver == "midpoint" and grid != "fallback":
        assert len(got_distinct) == 2 * N
    # every stage 1 is followed by its stage 2, and no stage ever takes the direct branch
    for a, b in zip(got, got[1:] + [None]):
        if a.stage == 1:
            assert b is not None and b.stage == 2 and a.save == 1 and a.t < b.t < np.float32(0.999)
        assert a.direct == 0 or a.stage == 0


BAD_GRIDS = {
    "one value": [0.0],
    "first not 0": [0.1, 0.5, 1.0],
    "last not 1": [0.0, 0.5, 0.9],
    "repeated": [0.0, 0.5, 0.5, 1.0],
    "decreasing": [0.0, 0.6, 0.4, 1.0],
    "nan": [0.0, float("nan"), 1.0],
    "nan first": [float("nan"), 0.5, 1.0],
    "nan last": [0.0, 0.5, float("nan")],
}


@pytest.mark.parametrize("case", sorted(BAD_GRIDS))
def test_invalid_grids_are_rejected(case):
    ts = BAD_GRIDS[case]
    arr = (C.c_float * len(ts))(*ts)
    ne, nd = C.c_int32(-7), C.c_int32(-7)
    for solver in (0, 1, 2):
        assert L.lib().jat_solver_plan(arr, len(ts), solver, None, 0, C.byref(ne), None, C.byref(nd)) == L.JAT_E_INVALID, (case, solver)
        assert L.lib().jat_last_error()
    with pytest.raises(ValueError):
        solver_plan("midpoint", ts)


def test_invalid_solver_and_default_grid_length_are_rejected():
    good = (C.c_float * 3)(0.0, 0.5, 1.0)
    for solver in (-1, 3, 99):
        assert L.lib().jat_solver_plan(good, 3, solver, None, 0, None, None, None) == L.JAT_E_INVALID
    for n in (1, 0, -3):
        assert L.lib().jat_solver_plan(None, n, 0, None, 0, None, None, None) == L.JAT_E_INVALID
    with pytest.raises(ValueError):
        solver_plan("rk4", [0.0, 1.0])
    # too little room for the list is an error, not an overrun; a count alone needs no room
    ne = C.c_int32(0)
    assert L.lib().jat_solver_plan(good, 3, 1, None, 0, C.byref(ne), None, None) == 0 and ne.value == 4
    room = (SolverEval * 3)()
    assert L.lib().jat_solver_plan(good, 3, 1, room, 3, None, None, None) == L.JAT_E_INVALID


GATES = {"euler": 3e-2, "midpoint": 6e-2, "heun": 3e-2}      # the rel-L2 gates of tests/test_gpu_solvers.py


@pytest.mark.parametrize("name", ["micro", "tiny"])
def test_gpu_case_tells_the_solvers_apart(name):
    """The inputs of tests/test_gpu_solvers.py: the fp64 results of any two solvers differ by rel-L2 > 0.09 (the later solver of
    euler, midpoint, heun against the earlier one; the smallest figure is Heun against Euler at micro, 0.092; against Heun's own
    norm it is 0.090).  That is more than the sum of any two gates, so passing a gate rules out having run another solver.
    The exact form of that argument is asserted as well: a result within gate g_a of solver a's twin and within g_b of solver
    b's would need |a - b| <= g_a |a| + g_b |b|."""
    order = ["euler", "midpoint", "heun"]
    res = {s: R.case_reference(name, s) for s in order}
    for a, b in itertools.combinations(order, 2):
        diff = float(np.linalg.norm(res[b] - res[a]))
        na, nb = float(np.linalg.norm(res[a])), float(np.linalg.norm(res[b]))
        print(f"{name}: {b} against {a}: rel-L2 {diff / na:.4f} (against {b}'s own norm {diff / nb:.4f})")
        assert diff / na > 0.09
        assert diff > GATES[a] * na + GATES[b] * nb
