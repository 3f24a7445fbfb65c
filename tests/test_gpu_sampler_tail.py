"""The CFG sampler's fused step tail: CFG combine + Euler update inside the final Linear (EPI_CFG_EULER, csrc/gemm.hip), the
latent kept in patch layout over the steps.

The fused tail replaces three launches per step (unpatchify store of x_pred, cfg_euler, next step's patchify) and is built to
change no bit, so the yardstick is an equality: the same model with the "fuse_euler" switch at 0 runs the three launches, and
every output must be `torch.equal`.  Two levels:

  * the sampler (`jat_sampler_run`): graph and eager replays, two consecutive runs, shapes that make ragged paired tiles, rows of
    several samples in one half tile, a frame mask, and the shapes / settings that must NOT fuse (`jat_sampler_tail_fused`);
  * the kernel (`jat_k_gemm_cfg_euler`, fused = 1 against fused = 0 on caller buffers): every tile the epilogue is built for,
    with and without the folded norms' row partials, on the Euler branch (t = 0.5) and on the direct branch (t = 0.9995), which
    no short schedule reaches.

Sanity bound of the kernel cases.  z' is also compared with a torch fp64 evaluation of the same formula on the fp32 preds the
un-fused launch stored: x = u + s (c - u); z' = z + (x - z) / denom * dt (or x).  The kernel evaluates it as one chain of at most
four fp32 roundings (c - u; the fused s * . + u; x - z and the correctly rounded quotient; the fused . * dt + z), each at most half
an ulp of a value no larger than a few times the data's magnitude (s = 3, dt / denom < 1), so the bound is 4 ulp of fp32
(4 * 2^-23) at the magnitude of z: max |z| over the old and the new latent of the case.  The data are scaled so that preds and z
are both O(1).  It is a bound on that chain, not a measured figure.
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

OP = torch.float16 if L.OPERAND_DTYPE == "fp16" else torch.bfloat16
_models = {}


def model(name):
    """One model per configuration with recipe weights; at most one resident."""
    if name not in _models:
        L.require_gpu()
        _models.clear()
        cfg = recipe.CONFIGS[name]
        sd = recipe.make_state_dict(cfg)
        m = JaT_AudioSR_V3(**cfg)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
        _models[name] = m.to("cuda").eval()
    return _models[name]


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


# (config, B, T, cfg_scale, lengths, extra switches, fused expected)
SAMPLER_CASES = [
    ("micro", 1, 64, 3.0, None, {}, True),              # Mh = 16: one ragged paired tile
    ("micro", 7, 64, 3.0, None, {}, True),              # Mh = 112
    ("micro", 9, 64, 3.0, None, {}, True),              # Mh = 144: second row tile ragged
    ("micro", 3, 100, 3.0, None, {}, True),             # ntok = 25, Mh = 75: rows of several samples in a half tile
    ("micro", 3, 64, 3.0, [64, 40, 12], {}, True),      # frame mask
    ("micro", 7, 64, 3.0, None, {"fold_norm": 2}, True),   # folded norms: the epilogue scales its rows by the producers' rstd
    ("micro", 2, 62, 3.0, None, {}, False),             # T % 4 != 0
    ("micro", 2, 64, 1.0, None, {}, False),             # no CFG
    ("wide2", 2, 512, 3.0, None, {"fold_norm": 2, "fuse_qkv_attn": 2}, True),   # the flagship's folded + fused-attention arrangement
    ("wide2", 7, 64, 3.0, None, {}, True),              # Mh = 112 at full width
    ("wide2", 28, 512, 3.0, None, {}, True),            # the flagship's bucket: M = 7168 plans the 224 x 256 quadrant ping-pong tile (35)
]
# the final Linear's tile (jat_k_gemm_plan, site 4) the cases above are there for: (config, B, T) -> variant
FINAL_TILE = {("wide2", 2, 512): 28, ("wide2", 28, 512): 35}
DEFAULTS = {"fold_norm": 1, "fuse_qkv_attn": 1, "fuse_euler": 1}


@pytest.mark.parametrize("name,B,T,scale,lengths,switches,fused", SAMPLER_CASES,
                         ids=[f"{c[0]}-B{c[1]}-T{c[2]}-s{c[3]}" + ("-len" if c[4] else "") + ("-sw" if c[5] else "") for c in SAMPLER_CASES])
def test_sampler_fused_tail_equals_separate_launches(name, B, T, scale, lengths, switches, fused):
    """3 steps; "fuse_euler" 1 against 0 (the separate launches) on the same model: graph replay, a second graph replay and an
    eager replay, all `torch.equal`; `jat_sampler_tail_fused` reports what the case expects."""
    m = model(name)
    h = m._get_handle()
    Cin = recipe.CONFIGS[name]["input_channels"]
    if (name, B, T) in FINAL_TILE:
        v, k = C.c_int32(), C.c_int32()
        L.check(L.lib().jat_k_gemm_plan(h.ptr, 4, 2 * B * (T // 4), 4 * Cin, recipe.CONFIGS[name]["hidden_size"], 1, C.byref(v), C.byref(k)))
        assert (v.value, k.value) == (FINAL_TILE[(name, B, T)], 1)
    lr = recipe.gaussian("tail_lr", (B, Cin, T), 500 + B)
    z0 = recipe.gaussian("tail_z0", (B, Cin, T), 600 + B)
    if lengths:
        for b, n in enumerate(lengths):   # the caller zero-pads beyond a row's frames
            lr[b, :, n:] = 0
            z0[b, :, n:] = 0
    lr, z0 = cuda(lr), cuda(z0)
    outs = {}
    try:
        for k, v in switches.items():
            h.set_switch(k, v)
        for fuse in (0, 1):
            h.set_switch("fuse_euler", fuse)
            s = jatsr_amd.Sampler(m, B, T, 3, scale)
            assert s.tail_fused() == (fused and fuse == 1), (fuse, s.info())
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


def _to_patch(z, ntok):
    B, Cc, _ = z.shape
    return z.view(B, Cc, ntok, 4).permute(0, 2, 1, 3).reshape(B * ntok, Cc * 4).contiguous()


KERNEL_SHAPES = [(M, N, K) for M in (32, 224, 288) for N in (128, 4096) for K in (256, 1280)]
NTOK = 16       # divides M / 2 = 16, 112, 144: 1, 7 and 9 samples


@pytest.mark.parametrize("M,N,K", KERNEL_SHAPES)
def test_kernel_fused_tail_equals_composition(M, N, K):
    """`jat_k_gemm_cfg_euler` fused against the three launches it replaces, bit for bit on the latent and on the next step's
    bf16 patch operand, on every tile that has the epilogue (28: 64 x 128, 20: 128 x 128; for N % 256 == 0 also the quadrant
    ping-pong tiles 35: 224 x 256 — the flagship's — and 33: 256 x 256), with and without row partials (then also with a frame
    mask), at t = 0.5 and t = 0.9995; plus the fp64 sanity bound of the module docstring."""
    idx = KERNEL_SHAPES.index((M, N, K))
    Mh, B, Cc, T = M // 2, M // 2 // NTOK, N // 4, NTOK * 4
    A = cuda(recipe.gaussian("tail_a", (M, K), idx)).to(OP)
    W = cuda(recipe.gaussian("tail_w", (N, K), idx) * np.float32(1.0 / np.sqrt(K))).to(OP)
    bias = cuda(recipe.gaussian("tail_b", (N,), idx) * np.float32(0.1))
    z_start = cuda(recipe.gaussian("tail_z", (B, Cc, T), idx))
    np_slots = (4, 8, 16)[idx % 3]
    part = (cuda(recipe.gaussian("tail_p", (M, np_slots), idx)).abs() + 0.5) * (K / np_slots)    # row sums of x^2: rstd = O(1)
    frames = torch.tensor([T - 5 * (b + 1) for b in range(B)], dtype=torch.int32, device="cuda")
    s_cfg, dt = 3.0, 0.02
    variants = [28, 20] + ([35, 33] if N % 256 == 0 else [])
    for t in (0.5, 0.9995):
        for with_part in (False, True):
            p_in, p_np, fr = (part, np_slots, frames) if with_part else (None, 0, None)

            def run(variant, fused):
                z = _to_patch(z_start, NTOK) if fused else z_start.clone()
                a_patch = torch.full((Mh, N), -1, dtype=torch.int16, device="cuda")
                xpred = torch.full((2 * B, Cc, T), float("nan"), device="cuda")
                L.check(L.lib().jat_k_gemm_cfg_euler(L.ptr(A), L.ptr(W), L.ptr(bias), M, N, K, NTOK, L.ptr(p_in), p_np, L.ptr(z),
                                                     L.ptr(a_patch), L.ptr(xpred), L.ptr(fr), s_cfg, t, dt, variant,
                                                     1 if fused else 0, L.stream_ptr()))
                torch.cuda.synchronize()
                return (z if fused else _to_patch(z, NTOK)), a_patch, xpred

            for v in variants:
                z_ref, a_ref, xpred = run(v, False)
                z_got, a_got, _ = run(v, True)
                tag = (M, N, K, v, t, with_part)
                assert bool(torch.isfinite(z_ref).all()), tag
                assert torch.equal(z_got, z_ref), (tag, float((z_got - z_ref).abs().max()))
                assert torch.equal(a_got, a_ref), tag
                if with_part:      # masked frames read zero in the patch operand, the latent keeps evolving there
                    tok_frames = (torch.arange(NTOK, device="cuda") * 4)[None, :, None] + torch.arange(4, device="cuda")[None, None, :]
                    dead = (tok_frames >= frames[:, None, None]).view(B, NTOK, 1, 4).expand(B, NTOK, Cc, 4).reshape(Mh, N)
                    assert bool((a_got[dead] == 0).all()) and bool(dead.any()), tag
                # the same formula in fp64 on the fp32 preds
                c, u = xpred[:B].double(), xpred[B:].double()
                x = u + s_cfg * (c - u)
                z64 = z_start.double()
                denom = float(np.float32(1.0) - np.float32(t) + np.float32(1e-5))
                want = x if not (np.float32(t) < np.float32(0.999)) else z64 + (x - z64) / denom * float(np.float32(dt))
                want = _to_patch(want, NTOK)
                mag = max(float(z_start.abs().max()), float(z_got.abs().max()))
                err = float((z_got.double() - want).abs().max())
                print(f"tail kernel {tag}: |z' - fp64| {err:.3e}, bound {4 * 2.0 ** -23 * mag:.3e}")
                assert err <= 4 * 2.0 ** -23 * mag, tag


def test_kernel_rejects_tiles_without_the_epilogue():
    """A tile the epilogue is not built for is an error in the fused form (the sampler then keeps the separate launches)."""
    A = torch.zeros(32, 256, dtype=OP, device="cuda")
    W = torch.zeros(128, 256, dtype=OP, device="cuda")
    z = torch.zeros(16, 128, device="cuda")
    a_patch = torch.zeros(16, 128, dtype=torch.int16, device="cuda")
    rc = L.lib().jat_k_gemm_cfg_euler(L.ptr(A), L.ptr(W), None, 32, 128, 256, 16, None, 0, L.ptr(z), L.ptr(a_patch), None, None,
                                      3.0, 0.5, 0.02, 26, 1, L.stream_ptr())
    assert rc == L.JAT_E_INVALID
