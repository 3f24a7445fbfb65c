"""fp64 twin of the sampler's solvers and of their evaluation plan (include/jat_hip.h `jat_solver_plan`).

Definitions, shared with the kernels (csrc/jat_cfg_euler.h) and with the host plan (csrc/jat_api.cpp):

    x^(z, t)  CFG combine of the two predictions: xu + s (xc - xu)  (one prediction when s == 1)
    den(t)    fp32(fp32(1 - t) + 1e-5)
    v(z, t)   (x^ - z) / den(t)
    grid      fp32, strictly increasing, ts[0] == 0, ts[-1] == 1; default `linspace_f32(0, 1, steps + 1)`
    step i    t = ts[i], dt = fp32(ts[i+1] - t), h = fp32(0.5 dt)

    euler     the reference's step: z' = z + v(z, t) dt for t < 0.999, else z' = x^
    midpoint  t2 = fp32(t + h);  z~ = z + h v(z, t)  (z kept as z_base);  z' = z_base + dt v(z~, t2)
    heun      t2 = ts[i+1];      z~ = z + dt v(z, t) (z kept as z_base);  z' = z_base / 2 + z~ / 2 + h v(z~, t2)
    fallback  a step whose t2 is not < 0.999 is the reference's Euler step, one evaluation
    stage 2   z_out = a z_base + b z_cur + c (x^ - z_cur) / den;  stage 1 is the Euler formula with step length c

Evaluation times that are bit-equal fp32 values share one index (`time_index`) in order of first appearance.

The times and coefficients are fp32 (what the kernels receive); the state and the model are fp64.
"""
import numpy as np

from oracle import jat_oracle as O

SOLVERS = {"euler": 0, "midpoint": 1, "heun": 2}
F = np.float32


def den(t):
    return F(F(F(1) - F(t)) + F(1e-5))


def plan(ts, solver):
    """-> (evals, distinct): evals = list of dicts t, time_index, den, a, b, c, stage, save, direct (fp32 / int)."""
    ts = np.asarray(ts, np.float32)
    assert solver in SOLVERS
    evals, distinct, index = [], [], {}

    def push(t, stage, a, b, c):
        key = F(t).tobytes()
        if key not in index:
            index[key] = len(distinct)
            distinct.append(F(t))
        evals.append(dict(t=F(t), time_index=index[key], den=den(t), a=F(a), b=F(b), c=F(c), stage=stage,
                          save=int(stage == 1), direct=int(stage == 0 and not (F(t) < F(0.999)))))

    for i in range(len(ts) - 1):
        t = ts[i]
        dt = F(ts[i + 1] - t)
        h = F(F(0.5) * dt)
        t2 = F(t + h) if solver == "midpoint" else ts[i + 1]
        if solver == "euler" or not (t2 < F(0.999)):
            push(t, 0, 0, 1, dt)
        elif solver == "midpoint":
            push(t, 1, 0, 1, h)
            push(t2, 2, 1, 0, dt)
        else:
            push(t, 1, 0, 1, dt)
            push(t2, 2, 0.5, 0.5, h)
    return evals, np.asarray(distinct, np.float32)


def x_hat(model, z, t, lr, cfg_scale):
    """The CFG combine exactly as oracle.jat_oracle.flow_matching_sample forms it."""
    dt_ = model.dtype
    B = z.shape[0]
    tb = np.full((B,), t, dtype=np.float32)
    if cfg_scale != 1.0:
        both = model.forward(np.concatenate([z, z], 0), np.concatenate([tb, tb], 0), np.concatenate([lr, np.zeros_like(lr)], 0))
        xc, xu = both[:B], both[B:]
        return xu + dt_(cfg_scale) * (xc - xu)
    return model.forward(z, tb, lr)


def sample(predict, z0, ts, solver, dtype=np.float64):
    """Walk the plan over `predict(z, t) -> x^`.  The Euler step is written as the oracle writes it."""
    z = np.asarray(z0).astype(dtype).copy()
    z_base = None
    for e in plan(ts, solver)[0]:
        x = predict(z, e["t"])
        if e["stage"] == 0:
            if e["direct"]:
                z = x
            else:
                v = (x - z) / dtype(e["den"])
                z = z + v * dtype(e["c"])
        elif e["stage"] == 1:
            z_base = z
            v = (x - z) / dtype(e["den"])
            z = z + v * dtype(e["c"])
        else:
            z = dtype(e["a"]) * z_base + dtype(e["b"]) * z + dtype(e["c"]) * (x - z) / dtype(e["den"])
    return z


def flow_matching_sample(model, lr_latent, z0, ts=None, solver="euler", cfg_scale=1.0, num_steps=None):
    """The twin of jatsr_amd.flow_matching_sample(solver=, timesteps=) over OracleModel.forward."""
    if ts is None:
        ts = O.linspace_f32(0.0, 1.0, num_steps + 1)
    lr = np.asarray(lr_latent).astype(model.dtype)
    return sample(lambda z, t: x_hat(model, z, t, lr, cfg_scale), z0, ts, solver, model.dtype)


# ---- the shared case of tests/test_solver_cpu.py (conditioning) and tests/test_gpu_solvers.py (sampler against the twin) --------
CASE_B, CASE_T, CASE_STEPS, CASE_CFG = 2, 64, 4, 3.0
NONUNIFORM = np.array([0.0, 0.1, 0.3, 0.6, 1.0], np.float32)      # 4 steps, growing
_case_cache = {}


def case_inputs(name):
    import jatsr_amd.recipe as recipe
    Cin = recipe.CONFIGS[name]["input_channels"]
    return (recipe.gaussian("lr_latent", (CASE_B, Cin, CASE_T), 900), recipe.gaussian("z0", (CASE_B, Cin, CASE_T), 901))


def case_reference(name, solver, grid="linspace"):
    """fp64 twin result of the shared case; computed once per process and handed out read-only."""
    key = (name, solver, grid)
    if key not in _case_cache:
        import jatsr_amd.recipe as recipe
        if ("model", name) not in _case_cache:
            cfg = recipe.CONFIGS[name]
            _case_cache[("model", name)] = O.OracleModel(cfg, recipe.make_state_dict(cfg), "rms", np.float64)
        lr, z0 = case_inputs(name)
        ts = O.linspace_f32(0.0, 1.0, CASE_STEPS + 1) if grid == "linspace" else NONUNIFORM
        out = flow_matching_sample(_case_cache[("model", name)], lr, z0, ts, solver, CASE_CFG)
        out.setflags(write=False)
        _case_cache[key] = out
    return _case_cache[key]
