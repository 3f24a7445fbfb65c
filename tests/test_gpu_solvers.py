"""Midpoint and Heun solvers and custom time grids of the sampler on the GPU.

  1. the sampler (`Sampler(solver=, timesteps=)`, graph replay) against the fp64 twin tests/solver_ref.py;
  2. `solver="euler"` is today's sampler, bit for bit;
  3. the fused tail (EPI_CFG_STAGE inside the final Linear, csrc/gemm.hip) against the separate launches, bit for bit;
  4. the kernel `jat_k_gemm_cfg_stage`, fused against un-fused on caller buffers, bit for bit, and against the fp64 formula;
  5. `jat_cfg_stage_step` against the fp64 formula;
  6. the folded-weight table keyed by the list of distinct times;
  7. the key mask of short rows under midpoint.

Gates of 1.  Heun: rel-L2 < 3e-2, the project's gate for the Euler sampler (SAMPLER_TOL of tests/test_gpu_model.py): Heun's second
stage multiplies the error of x^ by h / den(t2) <= 1/2.  Midpoint: rel-L2 < 6e-2 = 2 x SAMPLER_TOL, derived, not measured:
Euler's last step multiplies the error of x^ by dt / den <= 1, midpoint's last step by dt / den(t2) = dt / (dt / 2) = 2.
tests/test_solver_cpu.py shows that the twin's results of any two solvers on these inputs lie further apart than any two gates.
Measured on an MI355X (bf16 operands; printed by the test):
    micro: heun 5.6e-3, midpoint 1.07e-2;  tiny: heun 6.0e-3, midpoint 1.15e-2
    non-uniform grid: micro euler 5.3e-3, midpoint 1.04e-2;  tiny euler 5.8e-3, midpoint 1.14e-2
    un-fused paths (micro, midpoint): cfg_scale 1: 6.5e-3;  T = 62: 1.12e-2

Bound of 4 and 5.  z' is compared with an fp64 evaluation of the same formula on the fp32 preds the un-fused launch stored.  The
kernels evaluate the chain written in csrc/jat_cfg_euler.h:
    stage 1 (save): 5 fp32 roundings: c - u; the fused s * . + u; x - z; the correctly rounded quotient; the fused . * c + z
    stage 2:        7 fp32 roundings: c - u; the fused s * . + u; x - z; the quotient; b z; the fused a z_base + .; the fused . * c + .
(2 fewer without CFG), each at most half an ulp, so the bound is R * 2^-24 * mag with mag = max |.| over z, z_base and z' of the
case.  "At the magnitude of the latent" holds because the cases keep c / den <= 0.08: the roundings in front of the quotient
are taken at the magnitude of the preds (O(1) like z, times s = 3 at most) and reach z' multiplied by c / den; the last two or
three are taken at the magnitude of z itself.  The bit-for-bit comparisons do not depend on that choice, and the sampler cases of 3
run c / den up to 2.
"""

import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import jatsr_amd  # noqa: E402
import jatsr_amd._lib as L  # noqa: E402
import jatsr_amd.recipe as recipe  # noqa: E402
from jatsr_amd.model import JaT_AudioSR_V3  # noqa: E402
from oracle import jat_oracle as O  # noqa: E402

import solver_ref as R  # noqa: E402

OP = torch.float16 if L.OPERAND_DTYPE == "fp16" else torch.bfloat16
SAMPLER_TOL = 3e-2
GATE = {"euler": SAMPLER_TOL, "heun": SAMPLER_TOL, "midpoint": 2 * SAMPLER_TOL}
DEFAULTS = {"fold_norm": 1, "fuse_qkv_attn": 1, "fuse_euler": 1}
_models = {}


def fresh_model(name):
    L.require_gpu()
    cfg = recipe.CONFIGS[name]
    sd = recipe.make_state_dict(cfg)
    m = JaT_AudioSR_V3(**cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    return m.to("cuda").eval()


def model(name):
    """One model per configuration with recipe weights; at most one resident."""
    if name not in _models:
        _models.clear()
        _models[name] = fresh_model(name)
    return _models[name]


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def rel_l2(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b) / np.linalg.norm(b))


# ---- 1. the sampler against the twin ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["micro", "tiny"])
def test_sampler_against_the_fp64_twin(name):
    m = model(name)
    lr, z0 = R.case_inputs(name)
    B, T, steps, scale = R.CASE_B, R.CASE_T, R.CASE_STEPS, R.CASE_CFG
    runs = [("heun", None), ("midpoint", None), ("euler", R.NONUNIFORM), ("midpoint", R.NONUNIFORM)]
    for solver, grid in runs:
        s = jatsr_amd.Sampler(m, B, T, steps, scale, solver=solver, timesteps=grid)
        assert s.tail_fused()
        evals = {"euler": steps, "midpoint": 2 * steps, "heun": 2 * steps - 1}[solver]
        assert s.evaluations() == evals
        got = s.run(cuda(lr), cuda(z0), use_graph=True).cpu().numpy()
        want = R.case_reference(name, solver, "linspace" if grid is None else "nonuniform")
        r = rel_l2(got, want)
        print(f"{name} {solver} {'linspace' if grid is None else 'non-uniform'}: rel-L2 {r:.3e} (gate {GATE[solver]:.0e})")
        assert np.isfinite(got).all() and r < GATE[solver], (solver, r)
    # through the public function, cached by (solver, grid)
    a = jatsr_amd.flow_matching_sample(m, cuda(lr), num_steps=steps, cfg_scale=scale, verbose=False, z0=cuda(z0), solver="heun")
    assert rel_l2(a.cpu().numpy(), R.case_reference(name, "heun")) < GATE["heun"]
    e = jatsr_amd.flow_matching_sample(m, cuda(lr), num_steps=steps, cfg_scale=scale, verbose=False, z0=cuda(z0))
    assert rel_l2(e.cpu().numpy(), R.case_reference(name, "euler")) < GATE["euler"] and not torch.equal(a, e)


@pytest.mark.parametrize("T,scale", [(64, 1.0), (62, 3.0)], ids=["no-cfg", "T62"])
def test_midpoint_on_the_unfused_paths_against_the_twin(T, scale):
    """cfg_scale == 1 and T % 4 != 0 keep the separate launches (cfg_stage_kernel)."""
    m = model("micro")
    cfg = recipe.CONFIGS["micro"]
    lr = recipe.gaussian("lr_latent", (2, 32, T), 900)
    z0 = recipe.gaussian("z0", (2, 32, T), 901)
    s = jatsr_amd.Sampler(m, 2, T, 4, scale, solver="midpoint")
    assert not s.tail_fused() and s.evaluations() == 8
    got = s.run(cuda(lr), cuda(z0), use_graph=True).cpu().numpy()
    oracle = O.OracleModel(cfg, recipe.make_state_dict(cfg), "rms", np.float64)
    want = R.flow_matching_sample(oracle, lr, z0, None, "midpoint", scale, num_steps=4)
    r = rel_l2(got, want)
    print(f"micro midpoint T={T} cfg={scale}: rel-L2 {r:.3e}")
    assert np.isfinite(got).all() and r < GATE["midpoint"]


# ---- 2. solver="euler" is today's sampler ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,B,T,switches", [("micro", 7, 64, {}), ("wide2", 2, 512, {"fold_norm": 2, "fuse_qkv_attn": 2})],
                         ids=["micro", "wide2"])
def test_euler_solver_is_the_existing_sampler(name, B, T, switches):
    m = model(name)
    h = m._get_handle()
    Cin = recipe.CONFIGS[name]["input_channels"]
    lr, z0 = cuda(recipe.gaussian("eq_lr", (B, Cin, T), 700 + B)), cuda(recipe.gaussian("eq_z0", (B, Cin, T), 800 + B))
    steps, scale = 3, 3.0
    try:
        for k, v in switches.items():
            h.set_switch(k, v)
        ref = jatsr_amd.Sampler(m, B, T, steps, scale).run(lr, z0)
        a = jatsr_amd.Sampler(m, B, T, steps, scale, solver="euler", timesteps=None).run(lr, z0)
        b = jatsr_amd.Sampler(m, B, T, 999, scale, solver="euler", timesteps=O.linspace_f32(0.0, 1.0, steps + 1)).run(lr, z0)
    finally:
        for k, v in DEFAULTS.items():
            h.set_switch(k, v)
    assert bool(torch.isfinite(ref).all()) and not torch.equal(ref, z0)
    assert torch.equal(a, ref) and torch.equal(b, ref)


# ---- 3. the fused tail equals the separate launches ---------------------------------------------------------------------------
# (config, B, T, lengths, extra switches)
TAIL_CASES = [
    ("micro", 1, 64, None, {}),
    ("micro", 7, 64, None, {}),
    ("micro", 9, 64, None, {}),
    ("micro", 3, 100, None, {}),
    ("micro", 3, 64, [64, 40, 12], {}),
    ("micro", 7, 64, None, {"fold_norm": 2}),
    ("wide2", 2, 512, None, {"fold_norm": 2, "fuse_qkv_attn": 2}),
]


@pytest.mark.parametrize("solver", ["midpoint", "heun"])
@pytest.mark.parametrize("name,B,T,lengths,switches", TAIL_CASES,
                         ids=[f"{c[0]}-B{c[1]}-T{c[2]}" + ("-len" if c[3] else "") + ("-sw" if c[4] else "") for c in TAIL_CASES])
def test_fused_stage_tail_equals_separate_launches(name, B, T, lengths, switches, solver):
    """3 steps; "fuse_euler" 1 against 0 on the same model: graph replay, a second graph replay and an eager replay, all
    `torch.equal`.  Heun's third step ends at t = 1 and is the Euler step, so both epilogues run in one graph."""
    m = model(name)
    h = m._get_handle()
    Cin = recipe.CONFIGS[name]["input_channels"]
    lr = recipe.gaussian("tail_lr", (B, Cin, T), 500 + B)
    z0 = recipe.gaussian("tail_z0", (B, Cin, T), 600 + B)
    if lengths:
        for b, n in enumerate(lengths):
            lr[b, :, n:] = 0
            z0[b, :, n:] = 0
    lr, z0 = cuda(lr), cuda(z0)
    outs = {}
    try:
        for k, v in switches.items():
            h.set_switch(k, v)
        for fuse in (0, 1):
            h.set_switch("fuse_euler", fuse)
            s = jatsr_amd.Sampler(m, B, T, 3, 3.0, solver=solver)
            assert s.tail_fused() == (fuse == 1), (fuse, s.info())
            assert s.evaluations() == (6 if solver == "midpoint" else 5)
            if "fuse_qkv_attn" in switches:
                assert s.info()["fused_attn"]
            if name == "micro" and "fold_norm" in switches:
                assert s.info()["folded"]
            outs[fuse] = [s.run(lr, z0, use_graph=True, lengths=lengths), s.run(lr, z0, use_graph=True, lengths=lengths),
                          s.run(lr, z0, use_graph=False, lengths=lengths)]
            torch.cuda.synchronize()
            del s
    finally:
        for k, v in DEFAULTS.items():
            h.set_switch(k, v)
    ref = outs[0][0]
    assert bool(torch.isfinite(ref).all()) and not torch.equal(ref, z0)
    for fuse in (0, 1):
        for i, o in enumerate(outs[fuse]):
            assert torch.equal(o, ref), (fuse, ["graph", "graph again", "eager"][i], float((o - ref).abs().max()))


# ---- 4. the kernel ------------------------------------------------------------------------------------------------------------
def _to_patch(z, ntok):
    B, Cc, _ = z.shape
    return z.view(B, Cc, ntok, 4).permute(0, 2, 1, 3).reshape(B * ntok, Cc * 4).contiguous()


def _stage64(xpred, z, zb, B, s_cfg, t, a, b, c, save):
    """The definition in fp64 on fp32 inputs; -> z'."""
    if s_cfg != 1.0:
        cc, u = xpred[:B].double(), xpred[B:].double()
        x = u + s_cfg * (cc - u)
    else:
        x = xpred[:B].double()
    den = float(np.float32(np.float32(1.0) - np.float32(t)) + np.float32(1e-5))
    z, zb = z.double(), zb.double()
    c = float(np.float32(c))
    if save:
        return z + (x - z) / den * c
    return float(np.float32(a)) * zb + float(np.float32(b)) * z + c * (x - z) / den


KERNEL_SHAPES = [(M, N, 256) for M in (32, 224, 288) for N in (128, 4096)]
NTOK = 16       # divides M / 2 = 16, 112, 144: 1, 7 and 9 samples
# (save, a, b, c) at t = 0.5 (den = 0.50001): stage 1 with h, midpoint's and Heun's second stages
MODES = [(1, 0.0, 1.0, 0.02), (0, 1.0, 0.0, 0.04), (0, 0.5, 0.5, 0.02)]


@pytest.mark.parametrize("M,N,K", KERNEL_SHAPES)
def test_kernel_fused_stage_equals_composition(M, N, K):
    """`jat_k_gemm_cfg_stage` fused against the launches it replaces (unpatchify store, cfg_stage_kernel, patchify), bit for bit
    on the latent, on z_base and on the next evaluation's bf16 patch operand, on every tile that has the epilogue (28, 20; for
    N % 256 == 0 also 35 and 33), in the three modes, with and without row partials (then also with a frame mask); plus the fp64
    bound of the module docstring: 5 roundings for stage 1, 7 for stage 2."""
    idx = KERNEL_SHAPES.index((M, N, K))
    Mh, B, Cc, T = M // 2, M // 2 // NTOK, N // 4, NTOK * 4
    A = cuda(recipe.gaussian("stage_a", (M, K), idx)).to(OP)
    W = cuda(recipe.gaussian("stage_w", (N, K), idx) * np.float32(1.0 / np.sqrt(K))).to(OP)
    bias = cuda(recipe.gaussian("stage_b", (N,), idx) * np.float32(0.1))
    z_start = cuda(recipe.gaussian("stage_z", (B, Cc, T), idx))
    zb_start = cuda(recipe.gaussian("stage_zb", (B, Cc, T), idx))
    np_slots = (4, 8, 16)[idx % 3]
    part = (cuda(recipe.gaussian("stage_p", (M, np_slots), idx)).abs() + 0.5) * (K / np_slots)    # row sums of x^2: rstd = O(1)
    frames = torch.tensor([T - 5 * (b + 1) for b in range(B)], dtype=torch.int32, device="cuda")
    s_cfg, t = 3.0, 0.5
    variants = [28, 20] + ([35, 33] if N % 256 == 0 else [])
    for save, ca, cb, cc in MODES:
        for with_part in (False, True):
            p_in, p_np, fr = (part, np_slots, frames) if with_part else (None, 0, None)

            def run(variant, fused):
                z = _to_patch(z_start, NTOK) if fused else z_start.clone()
                if save:     # the store must come from the kernel
                    zb = torch.full_like(z, float("nan"))
                else:
                    zb = _to_patch(zb_start, NTOK) if fused else zb_start.clone()
                a_patch = torch.full((Mh, N), -1, dtype=torch.int16, device="cuda")
                xpred = torch.full((2 * B, Cc, T), float("nan"), device="cuda")
                L.check(L.lib().jat_k_gemm_cfg_stage(L.ptr(A), L.ptr(W), L.ptr(bias), M, N, K, NTOK, L.ptr(p_in), p_np, L.ptr(z),
                                                     L.ptr(zb), L.ptr(a_patch), L.ptr(xpred), L.ptr(fr), s_cfg, t, ca, cb, cc, save,
                                                     variant, 1 if fused else 0, L.stream_ptr()))
                torch.cuda.synchronize()
                return (z, zb, a_patch, xpred) if fused else (_to_patch(z, NTOK), _to_patch(zb, NTOK), a_patch, xpred)

            for v in variants:
                z_ref, zb_ref, a_ref, xpred = run(v, False)
                z_got, zb_got, a_got, _ = run(v, True)
                tag = (M, N, K, v, (save, ca, cb, cc), with_part)
                assert bool(torch.isfinite(z_ref).all()), tag
                assert torch.equal(z_got, z_ref), (tag, float((z_got - z_ref).abs().max()))
                assert torch.equal(zb_got, zb_ref), tag
                assert torch.equal(zb_got, _to_patch(z_start if save else zb_start, NTOK)), tag
                assert torch.equal(a_got, a_ref), tag
                if with_part:      # masked frames read zero in the patch operand, the latent keeps evolving there
                    tok_frames = (torch.arange(NTOK, device="cuda") * 4)[None, :, None] + torch.arange(4, device="cuda")[None, None, :]
                    dead = (tok_frames >= frames[:, None, None]).view(B, NTOK, 1, 4).expand(B, NTOK, Cc, 4).reshape(Mh, N)
                    assert bool((a_got[dead] == 0).all()) and bool(dead.any()), tag
                want = _to_patch(_stage64(xpred, z_start, zb_start, B, s_cfg, t, ca, cb, cc, save), NTOK)
                mag = max(float(z_start.abs().max()), float(z_got.abs().max()), 0.0 if save else float(zb_start.abs().max()))
                bound = (5 if save else 7) * 2.0 ** -24 * mag
                err = float((z_got.double() - want).abs().max())
                print(f"stage kernel {tag}: |z' - fp64| {err:.3e}, bound {bound:.3e}")
                assert err <= bound, tag


def test_kernel_rejects_tiles_without_the_epilogue():
    A = torch.zeros(32, 256, dtype=OP, device="cuda")
    W = torch.zeros(128, 256, dtype=OP, device="cuda")
    z = torch.zeros(16, 128, device="cuda")
    zb = torch.zeros(16, 128, device="cuda")
    a_patch = torch.zeros(16, 128, dtype=torch.int16, device="cuda")
    rc = L.lib().jat_k_gemm_cfg_stage(L.ptr(A), L.ptr(W), None, 32, 128, 256, 16, None, 0, L.ptr(z), L.ptr(zb), L.ptr(a_patch), None,
                                      None, 3.0, 0.5, 1.0, 0.0, 0.04, 0, 26, 1, L.stream_ptr())
    assert rc == L.JAT_E_INVALID
    rc = L.lib().jat_k_gemm_cfg_stage(L.ptr(A), L.ptr(W), None, 32, 128, 256, 16, None, 0, L.ptr(z), None, L.ptr(a_patch), None,
                                      None, 3.0, 0.5, 1.0, 0.0, 0.04, 0, 28, 1, L.stream_ptr())
    assert rc == L.JAT_E_INVALID        # no z_base


# ---- 5. the element-wise kernel -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Cc,T", [(1, 3, 37), (3, 33, 101)], ids=["111", "9999"])
@pytest.mark.parametrize("s_cfg", [3.0, 1.0])
def test_cfg_stage_step_against_fp64(B, Cc, T, s_cfg):
    """`jat_cfg_stage_step` on element counts that are no multiple of 4 (the scalar tail) in one block and in several."""
    nb = 2 * B if s_cfg != 1.0 else B
    xpred = cuda(recipe.gaussian("step_x", (nb, Cc, T), B))
    z_start = cuda(recipe.gaussian("step_z", (B, Cc, T), B))
    zb_start = cuda(recipe.gaussian("step_zb", (B, Cc, T), B))
    for save, ca, cb, cc in MODES:
        z = z_start.clone()
        zb = torch.full_like(z, float("nan")) if save else zb_start.clone()
        L.check(L.lib().jat_cfg_stage_step(L.ptr(xpred), L.ptr(z), L.ptr(zb), s_cfg, 0.5, ca, cb, cc, save, B, Cc, T, L.stream_ptr()))
        torch.cuda.synchronize()
        assert torch.equal(zb, z_start if save else zb_start)
        want = _stage64(xpred, z_start, zb_start, B, s_cfg, 0.5, ca, cb, cc, save)
        mag = max(float(z_start.abs().max()), float(z.abs().max()), 0.0 if save else float(zb_start.abs().max()))
        rounds = (5 if save else 7) - (0 if s_cfg != 1.0 else 2)
        err = float((z.double() - want).abs().max())
        print(f"stage step {(B, Cc, T, s_cfg, save, ca, cb, cc)}: |z' - fp64| {err:.3e}, bound {rounds * 2.0 ** -24 * mag:.3e}")
        assert err <= rounds * 2.0 ** -24 * mag


# ---- 6. the folded-weight table is keyed by the distinct times -------------------------------------------------------------------
def test_fold_table_is_keyed_by_the_times():
    """Euler-4, midpoint-4 and Heun-4 samplers alive together on one model (Heun shares Euler's table, midpoint's has 8 entries):
    each equals a freshly created sampler of its kind on a freshly loaded model."""
    lr, z0 = cuda(recipe.gaussian("fold_lr", (2, 32, 64), 31)), cuda(recipe.gaussian("fold_z0", (2, 32, 64), 32))
    kinds = ["euler", "midpoint", "heun"]
    m = fresh_model("micro")
    m._get_handle().set_switch("fold_norm", 2)
    together = {k: jatsr_amd.Sampler(m, 2, 64, 4, 3.0, solver=k) for k in kinds}
    info = {k: s.info() for k, s in together.items()}
    assert all(i["folded"] for i in info.values()), info
    assert info["heun"]["fold_bytes"] == info["euler"]["fold_bytes"] < info["midpoint"]["fold_bytes"]
    outs = {k: s.run(lr, z0) for k, s in together.items()}
    outs2 = {k: together[k].run(lr, z0) for k in reversed(kinds)}
    for k in kinds:
        f = fresh_model("micro")
        f._get_handle().set_switch("fold_norm", 2)
        s = jatsr_amd.Sampler(f, 2, 64, 4, 3.0, solver=k)
        assert s.info()["folded"]
        want = s.run(lr, z0)
        assert torch.equal(outs[k], want) and torch.equal(outs2[k], want), k
        del s, f
    assert not torch.equal(outs["euler"], outs["heun"]) and not torch.equal(outs["euler"], outs["midpoint"])


# ---- 7. the key mask under midpoint ---------------------------------------------------------------------------------------------
def test_short_row_under_midpoint_equals_its_stand_alone_run():
    """tiny; the figure is that of tests/test_gpu_model.py's Euler case (2e-5)."""
    m = model("tiny")
    Cc, T, short = 1024, 92, 50
    lr = recipe.gaussian("len_lr", (2, Cc, T), short)
    z0 = recipe.gaussian("len_z0", (2, Cc, T), short + 100)
    lr[1, :, short:] = 0
    z0[1, :, short:] = 0
    kw = dict(num_steps=4, cfg_scale=2.5, verbose=False, solver="midpoint")
    both = jatsr_amd.flow_matching_sample(m, cuda(lr), z0=cuda(z0), lengths=[T, short], **kw)
    alone = jatsr_amd.flow_matching_sample(m, cuda(lr[1:2, :, :short]), z0=cuda(z0[1:2, :, :short]), **kw)
    r = rel_l2(both[1:2, :, :short].cpu().numpy(), alone.cpu().numpy().astype(np.float64))
    print(f"short row under midpoint: rel-L2 {r:.3e}")
    assert r < 2e-5
