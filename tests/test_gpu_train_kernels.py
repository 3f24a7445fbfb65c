"""Per-kernel parity of the training step on the GPU, through the C ABI (include/jat_hip.h `jat_k_*` training entries).

Every kernel that jat_trainer_fwd_bwd / jat_trainer_optim launches is compared with a plain fp64 torch evaluation of the
same operation on the SAME operand-rounded inputs (autograd where it is a gradient), at ragged shapes and the edges where
the kernels change form: the 64-bit dropout index of the attention, the one-block dK/dV path, every norm_bwd width, both
gate_bwd thread counts, the 256-row slab of small_dx.  Dropout masks are rebuilt with the numpy mirror of csrc/jat_rng.h
(oracle.jat_oracle_train.drop_mult / drop_mult_range) and must agree exactly.

Tolerances are derived per output from the roundings the kernel is allowed to make; the symbols used:
  U     unit roundoff of the operand dtype (bf16 2^-8, fp16 2^-11): one rounding of a value to OP
  ulp   spacing of OP at the fp64 reference rounded to OP: a rounded output may sit one ulp from it (its own rounding
        plus the fp32 error before it, which moves it across at most one rounding boundary)
  g_n   n * 2^-24: worst-case relative error of an n-term fp32 sum, relative to the sum of the absolute terms
Scratch is poisoned with NaN, outputs are pre-filled with NaN inside NaN guard bands: an element a kernel forgets to
write, or writes out of place, shows up as a NaN or a changed guard.
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import jatsr_amd._lib as L  # noqa: E402
from oracle import jat_oracle_train as OT  # noqa: E402

OP = torch.float16 if L.OPERAND_DTYPE == "fp16" else torch.bfloat16
MANT = 10 if OP == torch.float16 else 7          # stored mantissa bits of OP
U = 2.0 ** -(MANT + 1)                           # unit roundoff of OP
EMIN = -24 if OP == torch.float16 else -133      # exponent of OP's smallest subnormal (its ulp below the normal range)
TINY = 2.0 ** (EMIN - 1)                         # absolute rounding error of a value that lands in OP's subnormal range
F32 = 2.0 ** -24                                 # unit roundoff of fp32
SEED = 0x9E3779B97F4A7C15
GUARD = 256                                      # elements of NaN on each side of every output buffer
NAN = float("nan")


def dev():
    L.require_gpu()
    return torch.device("cuda:0")


def gen(shape, seed, scale=1.0, offset=0.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale + offset).to(dev())


def gen_op(shape, seed, scale=1.0, offset=0.0):
    return gen(shape, seed, scale, offset).to(OP)


def guarded(shape, dtype=torch.float32, fill=NAN):
    """(buffer, view): the view has `shape`, the buffer holds GUARD NaN elements before and after it."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), NAN, dtype=dtype, device=dev())
    view = buf[GUARD:GUARD + n].view(shape)
    if not (isinstance(fill, float) and math.isnan(fill)):
        view.copy_(fill if torch.is_tensor(fill) else torch.full(shape, fill, dtype=dtype, device=dev()))
    return buf, view


def guards_intact(buf):
    return bool(torch.isnan(buf[:GUARD].float()).all()) and bool(torch.isnan(buf[-GUARD:].float()).all())


def work(nbytes):
    return torch.full(((int(nbytes) + 3) // 4 + 4,), NAN, dtype=torch.float32, device=dev())


def C_ptr(t, offset_elems=0):
    """Device pointer to element `offset_elems` of t (a column slot inside a strided row)."""
    return ctypes.c_void_p(t.data_ptr() + offset_elems * t.element_size())


def call(fn, *args):
    L.check(fn(*args))
    torch.cuda.synchronize()


def ulp(r):
    """Spacing of OP at each element of r (values representable in OP, as float64)."""
    _, e = torch.frexp(r.float())
    u = torch.pow(2.0, (e - 1 - MANT).clamp_min(EMIN).double())
    return torch.where(r == 0, torch.full_like(u, 2.0 ** EMIN), u)


def assert_rounded(out, ref, bound, what):
    """out (OP) against the fp64 reference rounded to OP: within one ulp plus `bound` (error the kernel makes before it
    rounds)."""
    r = ref.to(OP).double()
    err = (out.double() - r).abs()
    tol = ulp(r) + bound
    bad = ~(err <= tol)
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} / {bad.numel()} elements out of bound; first at "
                                 f"{np.unravel_index(int(bad.flatten().nonzero()[0]), tuple(bad.shape))}, "
                                 f"err {float(err[bad].flatten()[0]):.3e} tol {float(tol[bad].flatten()[0]):.3e}")


def assert_within(out, ref, bound, what):
    """fp32 output against the unrounded fp64 reference."""
    err = (out.double() - ref).abs()
    bad = ~(err <= bound)
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} / {bad.numel()} elements out of bound; first at "
                                 f"{np.unravel_index(int(bad.flatten().nonzero()[0]), tuple(bad.shape))}, "
                                 f"err {float(err[bad].flatten()[0]):.3e} "
                                 f"bound {float(bound.expand_as(err)[bad].flatten()[0]):.3e}")


@functools.lru_cache(maxsize=4)
def mask(site, p, shape):
    return torch.from_numpy(OT.drop_mult(SEED, site, p, shape)).to(dev())


def assert_mask_exact(out, m, ref, what):
    """Every element the mirror drops is exactly 0, and no other element is where the exact value cannot round to 0
    (|ref| above OP's smallest subnormal; inputs are nonzero by construction)."""
    z = out == 0
    drop = (m == 0).expand_as(z)
    assert bool(z[drop].all()), f"{what}: {int((~z[drop]).sum())} dropped elements are not 0"
    live = ~drop & (ref.abs() > 2.0 ** EMIN)
    assert not bool(z[live].any()), f"{what}: {int(z[live].sum())} kept elements are 0"


# ---------------------------------------------------------------------------------------------------------------------
# GELU forward / backward (MLP hidden activation with nn.Dropout after it: site kind 2)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,p", [(8, 0.0), (8 * 37 * 61, 0.1), (2048 * 5 + 8, 0.5), (262152, 0.0)])
def test_gelu_forward_and_backward(n, p):
    site = 5 * 8 + 2
    x = gen_op((n,), 1, 2.0)
    assert bool((x != 0).all())
    ob, out = guarded((n,), OP)
    call(L.lib().jat_k_gelu, L.ptr(x), L.ptr(out), n, SEED, site, p, L.stream_ptr())
    m = mask(site, p, (n,))
    xd = x.double()
    cdf = 0.5 * (1 + torch.erf(xd / math.sqrt(2)))
    ref = xd * cdf * m
    # fp32 erff: <= 2 fp32 ulp absolute on a value near 1, times 0.5 |x|; the product / dropout factor: 2^-23 relative
    assert_rounded(out, ref, 2 * F32 * xd.abs() * m + 2 * F32 * ref.abs(), "gelu")
    # fp32 1 + erff(x / sqrt 2) is exactly 0 below x ~ -5.9: the kept side is checked where it is not (x > -4)
    assert_mask_exact(out, m, ref * (xd > -4), "gelu mask")
    assert guards_intact(ob)
    out2 = torch.empty_like(out)
    call(L.lib().jat_k_gelu, L.ptr(x), L.ptr(out2), n, SEED, site, p, L.stream_ptr())
    assert torch.equal(out.view(torch.int16), out2.view(torch.int16))

    dpost = gen_op((n,), 2)
    assert bool((dpost != 0).all())
    db, d = guarded((n,), OP, dpost)
    call(L.lib().jat_k_gelu_bwd, L.ptr(x), L.ptr(d), n, SEED, site, p, L.stream_ptr())
    dg = cdf + xd * torch.exp(-0.5 * xd * xd) / math.sqrt(2 * math.pi)
    ref = dpost.double() * dg * m
    # gelu' in fp32: erff (2 fp32 ulp absolute near 1) + x phi(x) with __expf (relative error <= (|x^2/2| + 2) 2^-24 on
    # |x phi| <= 0.25): < 2^-20 absolute for |x| < 8; then two fp32 products (2^-23 relative)
    assert_rounded(d, ref, (2.0 ** -20 + 2 * F32 * dg.abs()) * dpost.double().abs() * m, "gelu_bwd")
    assert_mask_exact(d, m, ref * (xd > -4), "gelu_bwd mask")
    assert guards_intact(db)
    d2 = dpost.clone()
    call(L.lib().jat_k_gelu_bwd, L.ptr(x), L.ptr(d2), n, SEED, site, p, L.stream_ptr())
    assert torch.equal(d.view(torch.int16), d2.view(torch.int16))


# ---------------------------------------------------------------------------------------------------------------------
# gated residual forward and its backward (DropPath: site kind 1 / 4 over [B]; MLP-output dropout: kind 3 over [B,N,D])
# ---------------------------------------------------------------------------------------------------------------------
GATE_CASES = [  # D, B, ntok, DropPath p, element dropout p
    (256, 3, 1, 0.0, 0.0), (384, 1, 15, 0.5, 0.0), (1280, 3, 16, 0.0, 0.1), (2048, 3, 17, 0.3, 0.1),
    (2304, 1, 345, 0.1, 0.5), (256, 3, 345, 0.5, 0.1), (384, 3, 17, 0.0, 0.5), (1280, 1, 1, 0.5, 0.5),
    (2048, 1, 15, 0.0, 0.0), (2304, 3, 16, 0.3, 0.0)]
# DropPath sites (layer * 8 + 4, element dropout at layer * 8 + 3) whose draws under SEED drop some but not all of 3 samples at
# p = 0.3 and 0.5 and keep a single sample at p = 0.1 and 0.5: every case with element dropout has a live branch to check it on
PATH_R, PATH_G = 1 * 8 + 4, 18 * 8 + 4


def _gate_inputs(D, B, ntok, seed):
    M = B * ntok
    gate_all = gen((B, 6 * D), seed, 0.5)            # the adaLN modulation rows: gate at slot 5, stride 6 D
    y = gen_op((M, D), seed + 1)
    dx = gen((M, D), seed + 2)
    return gate_all, y, dx


@pytest.mark.parametrize("D,B,ntok,pp,pe", GATE_CASES)
def test_resid_gate(D, B, ntok, pp, pe):
    M = B * ntok
    gate_all, y, _ = _gate_inputs(D, B, ntok, 10)
    x_in = gen((M, D), 13)
    gate = gate_all[:, 5 * D:]
    xb, x_out = guarded((M, D))
    call(L.lib().jat_k_resid_gate, L.ptr(x_in), L.ptr(y), L.ptr(gate), 6 * D, L.ptr(x_out), M, D, ntok, SEED, PATH_R, pp,
         PATH_R - 1, pe, L.stream_ptr())
    pm = mask(PATH_R, pp, (B,)).repeat_interleave(ntok).view(M, 1)
    em = mask(PATH_R - 1, pe, (B, ntok, D)).view(M, D)
    g = gate.double().repeat_interleave(ntok, 0)
    br = g * y.double() * pm * em
    ref = x_in.double() + br
    # fp32: pm * em, * y, * gate, + x_in: four roundings, 2^-22 of the two terms' magnitudes covers them
    assert_within(x_out, ref, 4 * F32 * (x_in.double().abs() + br.abs()), "resid_gate")
    dropped = (pm * em).expand(M, D) == 0
    assert torch.equal(x_out[dropped], x_in[dropped]), "a dropped branch element must leave x_in bit-unchanged"
    assert guards_intact(xb)


@pytest.mark.parametrize("D,B,ntok,pp,pe", GATE_CASES)
def test_gate_bwd(D, B, ntok, pp, pe):
    M = B * ntok
    gate_all, y, dx = _gate_inputs(D, B, ntok, 20)
    gate = gate_all[:, 5 * D:]
    dyb, dy = guarded((M, D), OP)
    dmb, dmod = guarded((B, 6 * D))                   # dgate lands in slot 5 of each row; the other slots stay NaN
    nchunk = (ntok + 15) // 16
    wk = work(B * nchunk * D * 4)

    def args(dyv, dmv):
        return (L.ptr(dx), L.ptr(y), L.ptr(gate), 6 * D, L.ptr(dyv), C_ptr(dmv, 5 * D), 6 * D, B, D, ntok, SEED,
                PATH_G, pp, PATH_G - 1, pe, L.ptr(wk), wk.numel() * 4, L.stream_ptr())
    call(L.lib().jat_k_gate_bwd, *args(dy, dmod))
    pm = mask(PATH_G, pp, (B,)).repeat_interleave(ntok).view(M, 1)
    em = mask(PATH_G - 1, pe, (B, ntok, D)).view(M, D)
    g = gate.double().repeat_interleave(ntok, 0)
    ref_dy = dx.double() * g * pm * em
    # gate * pm, * dx, * m in fp32: three roundings before the one to OP
    assert_rounded(dy, ref_dy, 3 * F32 * ref_dy.abs(), "gate_bwd dy")
    assert_mask_exact(dy, pm * em, ref_dy, "gate_bwd dy mask")
    terms = (dx.double() * y.double() * pm * em).view(B, ntok, D)
    ref_dg = terms.sum(1)
    # each term: 3 fp32 products; the sum: a <= 16-term chunk in fp32 then nchunk chunk partials in order: g_(16 + nchunk)
    bound = (16 + nchunk + 3) * F32 * terms.abs().sum(1)
    dgate = dmod[:, 5 * D:]
    assert_within(dgate, ref_dg, bound, "gate_bwd dgate")
    assert bool(torch.isnan(dmod[:, :5 * D]).all()), "dgate wrote outside its slot"
    assert guards_intact(dyb) and guards_intact(dmb) and bool(torch.isfinite(dy).all())
    dy2, dm2 = torch.empty_like(dy), torch.full_like(dmod, NAN)
    call(L.lib().jat_k_gate_bwd, *args(dy2, dm2))
    assert torch.equal(dy.view(torch.int16), dy2.view(torch.int16)) and torch.equal(dgate, dm2[:, 5 * D:])
    if B > 1:   # another sample's inputs do not reach this sample's outputs
        dx[:ntok] = gen((ntok, D), 99)
        call(L.lib().jat_k_gate_bwd, *args(dy2, dm2))
        assert torch.equal(dy[ntok:].view(torch.int16), dy2[ntok:].view(torch.int16))
        assert torch.equal(dgate[1:], dm2[1:, 5 * D:])


# ---------------------------------------------------------------------------------------------------------------------
# norm backward: y = norm(x) (* w) * (1 + scale[b]) + shift[b]  (mode 0 RMSNorm with weight, mode 1 LayerNorm no affine)
# ---------------------------------------------------------------------------------------------------------------------
NORM_CASES = [  # D, mode, B, ntok, w, scale, accumulate, outputs (s dshift, c dscale, w dw)
    (256, 0, 3, 1, True, True, False, "scw"), (512, 0, 1, 15, False, True, True, "sc"),
    (768, 1, 3, 16, False, True, False, "sc"), (1280, 0, 3, 17, True, False, True, "w"),
    (2048, 1, 1, 345, False, False, True, ""), (2048, 0, 3, 345, True, True, True, "scw"),
    (1280, 1, 3, 345, False, True, True, "s"), (768, 0, 1, 17, True, True, False, "c"),
    (256, 1, 3, 15, False, True, False, "c"), (512, 0, 3, 16, True, True, False, "sw"),
    (1024, 0, 3, 17, True, True, True, "scw"), (1536, 1, 1, 16, False, True, False, "sc"),
    (1792, 0, 1, 15, True, False, False, "w")]


@pytest.mark.parametrize("D,mode,B,ntok,use_w,use_scale,acc,outs", NORM_CASES)
def test_norm_bwd(D, mode, B, ntok, use_w, use_scale, acc, outs):
    M = B * ntok
    x = gen((M, D), 30, 2.0, 0.3)
    dy = gen_op((M, D), 31, 1.0, 0.3)                    # a nonzero mean: the LayerNorm's mean(g) term is not small
    w = (1 + 0.2 * gen((D,), 32)) if use_w else None
    modb, mod = guarded((B, 6 * D))                      # scale at slot 4 (stride 6 D); every other slot stays NaN
    mod[:, 4 * D:5 * D] = gen((B, D), 33, 0.3)
    scale = mod[:, 4 * D:5 * D] if use_scale else None
    dxb, dx = guarded((M, D), fill=gen((M, D), 34) if acc else NAN)
    old = dx.clone()
    dmb, dmod = guarded((B, 6 * D))                      # dshift at slot 3, dscale at slot 4
    dwb, dw = guarded((D,))
    nchunk = (ntok + 15) // 16
    wk = work((B * nchunk * 3 * D + B * D) * 4)

    def run(dxv, dmv, dwv):
        call(L.lib().jat_k_norm_bwd, L.ptr(x), L.ptr(dy), L.ptr(w), C_ptr(mod, 4 * D) if use_scale else None, 6 * D, L.ptr(dxv),
             int(acc), C_ptr(dmv, 3 * D) if "s" in outs else None, C_ptr(dmv, 4 * D) if "c" in outs else None, 6 * D,
             L.ptr(dwv) if "w" in outs else None, B, D, ntok, mode, L.ptr(wk), wk.numel() * 4, L.stream_ptr())
    run(dx, dmod, dw)

    xd = x.double().requires_grad_()
    wd = (w.double() if use_w else torch.ones(D, dtype=torch.float64, device=x.device)).requires_grad_()
    sd = (scale.double() if use_scale else torch.zeros(B, D, dtype=torch.float64, device=x.device)).requires_grad_()
    shd = torch.zeros(B, D, dtype=torch.float64, device=x.device, requires_grad=True)
    if mode == 0:
        xh = xd / torch.sqrt((xd * xd).mean(-1, keepdim=True) + 1e-6)
        nw = xh * wd
    else:
        mu = xd.mean(-1, keepdim=True)
        xh = (xd - mu) / torch.sqrt(((xd - mu) ** 2).mean(-1, keepdim=True) + 1e-6)
        nw = xh
    bi = torch.arange(M, device=x.device) // ntok
    yv = nw * (1 + sd[bi]) + shd[bi]
    (yv * dy.double()).sum().backward()
    with torch.no_grad():
        xh = xh.detach()
        rstd = 1 / torch.sqrt(((xd - (xd.mean(-1, keepdim=True) if mode else 0)) ** 2).mean(-1, keepdim=True) + 1e-6)
        gv = dy.double() * wd * (1 + sd[bi])
        # dx = rstd (g - [mean g] - xh mean(g xh)): fp32 wave sums over D (<= 32 serial + 6 butterfly levels: g_38), rsqrt and
        # the statistics (a few 2^-24), LayerNorm's mean (g_38 of |x|, times rstd): < 4e-6 of the terms' scale; gate 1e-5
        scale_dx = rstd * (gv.abs() + gv.abs().mean(-1, keepdim=True) + xh.abs() * (gv * xh).abs().mean(-1, keepdim=True)
                           + (xd.abs().mean(-1, keepdim=True) * rstd * (gv * xh).abs().mean(-1, keepdim=True) if mode else 0))
        ref_dx = xd.grad + (old.double() if acc else 0)
        assert_within(dx, ref_dx, 1e-5 * scale_dx + (2 * F32 * old.double().abs() if acc else 0), "norm_bwd dx")
        # column sums over a sample's tokens (4 rows per wave, 4 waves, nchunk chunks) and, for dw, over samples: g_(8 + nchunk
        # + B) < 2e-6 plus xh's own 2^-21: gate 1e-5 of the sum of |terms|
        if "s" in outs:
            t = dy.double().view(B, ntok, D)
            assert_within(dmod[:, 3 * D:4 * D], shd.grad, 1e-5 * t.abs().sum(1), "norm_bwd dshift")
        if "c" in outs:
            t = (dy.double() * xh * wd).view(B, ntok, D)
            assert_within(dmod[:, 4 * D:5 * D], sd.grad, 1e-5 * t.abs().sum(1), "norm_bwd dscale")
        if "w" in outs:
            t = dy.double() * (1 + sd[bi]) * xh
            assert_within(dw, wd.grad, 1e-5 * t.abs().sum(0), "norm_bwd dw")
        else:
            assert bool(torch.isnan(dw).all())
        written = torch.zeros(6 * D, dtype=torch.bool, device=x.device)
        written[3 * D:4 * D] = "s" in outs
        written[4 * D:5 * D] = "c" in outs
        assert bool(torch.isnan(dmod[:, ~written]).all()), "dshift / dscale wrote outside their slots"
        assert bool(torch.isfinite(dmod[:, written]).all()) and bool(torch.isfinite(dx).all())
    assert guards_intact(dxb) and guards_intact(dmb) and guards_intact(dwb) and guards_intact(modb)
    # bit-reproducible, and per-sample: another sample's x does not reach this sample's dx / dshift / dscale
    dx2, dm2, dw2 = old.clone(), torch.full_like(dmod, NAN), torch.full_like(dw, NAN)
    run(dx2, dm2, dw2)
    assert torch.equal(dx, dx2) and torch.equal(dmod.nan_to_num(7.0), dm2.nan_to_num(7.0))
    assert torch.equal(dw.nan_to_num(7.0), dw2.nan_to_num(7.0))
    if B > 1:
        x[:ntok] = gen((ntok, D), 98)
        dx2.copy_(old)
        run(dx2, dm2, dw2)
        assert torch.equal(dx[ntok:], dx2[ntok:]) and torch.equal(dmod[1:].nan_to_num(7.0), dm2[1:].nan_to_num(7.0))


# ---------------------------------------------------------------------------------------------------------------------
# attention: training forward (o, lse, dropout on the probabilities: site kind 0) and backward
# ---------------------------------------------------------------------------------------------------------------------
def rope_tables():
    inv = 1.0 / torch.pow(10000.0, torch.arange(32, dtype=torch.float32) * 2 / 64)
    a = torch.arange(2048, dtype=torch.float32)[:, None] * inv[None, :]
    return torch.cos(a).to(dev()).contiguous(), torch.sin(a).to(dev()).contiguous()


def attn_inputs(B, N, Hq, Hkv, seed, spiky=False):
    qx = gen((B * N, Hq * 64), seed, 1.0)
    kx = gen((B * N, Hkv * 64), seed + 1, 1.0)
    if spiky:   # one key in the LAST 64-key block dominates every row: the running max jumps there and earlier blocks vanish
        u = torch.where(gen((64,), seed + 3) > 0, 1.75, -1.75)
        kx.view(B, N, Hkv, 64)[:, N - 3] = u
        qx.view(B, N, Hq, 64)[:] += u
    q, k = qx.to(OP), kx.to(OP)
    v = gen_op((B, Hkv, N, 64), seed + 2)
    npad = (N + 63) // 64 * 64
    vt = torch.zeros(B, Hkv, 64, npad, dtype=OP, device=q.device)
    vt[..., :N] = v.transpose(-1, -2)
    return q, k, v, vt, npad


def heads(t, B, N, H):   # [B*N, H*64] -> [B, H, N, 64] fp64
    return t.double().view(B, N, H, 64).transpose(1, 2)


def attn_ref(qh, kh, vh, M):
    G = qh.shape[1] // kh.shape[1]
    S = qh @ kh.repeat_interleave(G, 1).transpose(-1, -2)
    P = torch.softmax(S / 8, -1)
    O = (P * M) @ vh.repeat_interleave(G, 1)
    return S, P, O, torch.logsumexp(S / 8, -1) / math.log(2)


def check_attn_fwd(o_k, lse_k, qh, kh, vh, M, what):
    S, P, O, lse = attn_ref(qh, kh, vh, M)
    G = qh.shape[1] // kh.shape[1]
    # P o m is rounded to OP once (U relative, TINY absolute in OP's subnormal range) before the PV product; its fp32
    # score / exp2 / row-sum error stays below 2^-12 relative at these magnitudes (score: 64 exact products summed in fp32,
    # sum |q k| < 200 -> < 2e-4 absolute in log2 units).  Bound: (U + 2^-12) sum_j P m |v| + TINY sum_j |v| per element.
    va = vh.abs().repeat_interleave(G, 1)
    bound = (U + 2.0 ** -12) * ((P * M) @ va) + TINY * va.sum(-2, keepdim=True)
    assert_rounded(o_k, O, bound, what + " o")
    # lse: max score (error < 2^-12 as above) + log2 of an fp32 row sum (relative g_(N/64 + 18))
    assert_within(lse_k, lse, 2.0 ** -12 + 2.0 ** -20 * lse.abs(), what + " lse")
    return P, O


def unrope(x, cos, sin):   # gradient w.r.t. post-RoPE rows -> pre-RoPE: x0' = c x0 + s x1, x1' = c x1 - s x0 (pairs 2d', 2d'+1)
    N = x.shape[-2]
    c, s = cos[:N].double(), sin[:N].double()
    out = torch.empty_like(x)
    out[..., 0::2] = c * x[..., 0::2] + s * x[..., 1::2]
    out[..., 1::2] = c * x[..., 1::2] - s * x[..., 0::2]
    return out


def pair_sum(b):   # an error bound through the rotation: |c e0 + s e1| <= |e0| + |e1|
    s = b[..., 0::2] + b[..., 1::2]
    return torch.stack([s, s], -1).flatten(-2)


def check_attn_bwd(dq_k, dk_k, dv_k, qh, kh, vh, doh, o_kh, M, cos, sin, what):
    """dq_k [B,Hq,N,64], dk_k / dv_k [B,Hkv,N,64] from the kernel; o_kh = the kernel's own forward output."""
    G = qh.shape[1] // kh.shape[1]
    B, Hkv = kh.shape[0], kh.shape[1]
    q_, k_, v_ = (t.clone().requires_grad_() for t in (qh, kh, vh))
    _, P, O, _ = attn_ref(q_, k_, v_, M)
    (O * doh).sum().backward()
    with torch.no_grad():
        P, O = P.detach(), O.detach()
        ke, ve = kh.repeat_interleave(G, 1), vh.repeat_interleave(G, 1)
        dP = doh @ ve.transpose(-1, -2)
        delta = (doh * O).sum(-1, keepdim=True)
        dS = P * (dP * M - delta)
        # the kernel's delta is rowsum(dO o O_kernel): off by |dO . (O_kernel - O)| plus its 64-term fp32 sum (2^-18)
        ddelta = (doh * (o_kh - O)).sum(-1, keepdim=True).abs() + 2.0 ** -18 * (doh * o_kh).abs().sum(-1, keepdim=True)
        # dS = P (dP m - delta) / 8 carries P's fp32 error and its own rounding to OP (each <= U + 2^-12 relative: E), dP's
        # fp32 error (E of |dP| m, generous), the delta offset, and TINY absolute after the 1/8 scale
        E = U + 2.0 ** -12
        err_dS = 2 * E * dS.abs() + P * ddelta + E * P * M * dP.abs() + 8 * TINY
        b_dq = err_dS @ ke.abs() / 8
        b_dk = (err_dS.transpose(-1, -2) @ qh.abs() / 8).view(B, Hkv, G, *qh.shape[2:]).sum(2)
        b_dv = ((E * P * M + TINY).transpose(-1, -2) @ doh.abs()).view(B, Hkv, G, *qh.shape[2:]).sum(2)
        # fp32 MFMA accumulation over <= 2048 keys / queries: g_2048 = 2^-13 of the same absolute sums, inside E
        assert_rounded(dq_k, unrope(q_.grad, cos, sin), pair_sum(b_dq), what + " dq")
        assert_rounded(dk_k, unrope(k_.grad, cos, sin), pair_sum(b_dk), what + " dk")
        assert_rounded(dv_k, v_.grad, b_dv, what + " dv")


ATTN_CASES = [  # B, N, Hq, Hkv, p
    (2, 1, 4, 2, 0.1), (3, 3, 4, 4, 0.5), (1, 63, 8, 4, 0.0), (2, 64, 20, 4, 0.1), (1, 65, 4, 2, 0.5),
    (2, 130, 4, 4, 0.1), (1, 345, 20, 4, 0.1), (2, 345, 8, 4, 0.0), (1, 2048, 4, 2, 0.1), (1, 2048, 4, 4, 0.0)]


def run_fwd(q, k, vt, B, N, Hq, Hkv, npad, site, p):
    ob, o = guarded((B * N, Hq * 64), OP)
    lb, lse = guarded((B, Hq, N))
    call(L.lib().jat_k_attention_train, L.ptr(q), L.ptr(k), L.ptr(vt), L.ptr(o), L.ptr(lse), B, N, Hq, Hkv, npad, SEED, site,
         p, L.stream_ptr())
    assert guards_intact(ob) and guards_intact(lb) and bool(torch.isfinite(o).all()) and bool(torch.isfinite(lse).all())
    return o, lse


def run_bwd(q, k, vt, o, dout, lse, cos, sin, B, N, Hq, Hkv, npad, site, p, split):
    W = (Hq + 2 * Hkv) * 64
    gb, dqkv = guarded((B * N, W), OP)
    rows = B * Hq * N
    wk = work((rows * 4 + 255) // 256 * 256 + (rows * 128 * 4 if split else 0))
    call(L.lib().jat_k_attention_bwd, L.ptr(q), L.ptr(k), L.ptr(vt), L.ptr(o), L.ptr(dout), L.ptr(lse), L.ptr(dqkv), L.ptr(cos),
         L.ptr(sin), B, N, Hq, Hkv, npad, SEED, site, p, int(split), L.ptr(wk), wk.numel() * 4, L.stream_ptr())
    assert guards_intact(gb) and bool(torch.isfinite(dqkv).all())
    return dqkv


def split_dqkv(dqkv, B, N, Hq, Hkv):
    D, kvD = Hq * 64, Hkv * 64
    return heads(dqkv[:, :D], B, N, Hq), heads(dqkv[:, D:D + kvD], B, N, Hkv), heads(dqkv[:, D + kvD:], B, N, Hkv)


@pytest.mark.parametrize("B,N,Hq,Hkv,p", ATTN_CASES)
def test_attention_train_forward(B, N, Hq, Hkv, p):
    q, k, v, vt, npad = attn_inputs(B, N, Hq, Hkv, 40)
    o, lse = run_fwd(q, k, vt, B, N, Hq, Hkv, npad, 0, p)
    M = mask(0, p, (B, Hq, N, N))
    check_attn_fwd(heads(o, B, N, Hq), lse, heads(q, B, N, Hq), heads(k, B, N, Hkv), v.double(), M, "attention fwd")


def test_attention_train_forward_spiky_last_block():
    B, N, Hq, Hkv, p = 2, 200, 4, 2, 0.1
    q, k, v, vt, npad = attn_inputs(B, N, Hq, Hkv, 45, spiky=True)
    o, lse = run_fwd(q, k, vt, B, N, Hq, Hkv, npad, 0, p)
    M = mask(0, p, (B, Hq, N, N))
    qh, kh = heads(q, B, N, Hq), heads(k, B, N, Hkv)
    S = qh @ kh.repeat_interleave(Hq // Hkv, 1).transpose(-1, -2)
    assert bool((torch.softmax(S / 8, -1)[..., N - 3] > 0.9).all())   # the case is what it says
    check_attn_fwd(heads(o, B, N, Hq), lse, qh, kh, v.double(), M, "attention fwd spiky")


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("B,N,Hq,Hkv,p", ATTN_CASES)
def test_attention_train_backward(B, N, Hq, Hkv, p, split):
    q, k, v, vt, npad = attn_inputs(B, N, Hq, Hkv, 50)
    o, lse = run_fwd(q, k, vt, B, N, Hq, Hkv, npad, 0, p)
    dout = gen_op((B * N, Hq * 64), 53)
    cos, sin = rope_tables()
    dqkv = run_bwd(q, k, vt, o, dout, lse, cos, sin, B, N, Hq, Hkv, npad, 0, p, split)
    dq, dk, dv = split_dqkv(dqkv, B, N, Hq, Hkv)
    M = mask(0, p, (B, Hq, N, N))
    check_attn_bwd(dq, dk, dv, heads(q, B, N, Hq), heads(k, B, N, Hkv), v.double(), heads(dout, B, N, Hq), heads(o, B, N, Hq),
                   M, cos, sin, f"attention bwd split={split}")


def test_attention_train_per_sample_and_deterministic():
    B, N, Hq, Hkv, p = 3, 130, 4, 2, 0.1
    q, k, v, vt, npad = attn_inputs(B, N, Hq, Hkv, 60)
    dout = gen_op((B * N, Hq * 64), 63)
    cos, sin = rope_tables()
    o, lse = run_fwd(q, k, vt, B, N, Hq, Hkv, npad, 0, p)
    g = {s: run_bwd(q, k, vt, o, dout, lse, cos, sin, B, N, Hq, Hkv, npad, 0, p, s) for s in (True, False)}
    o2, lse2 = run_fwd(q, k, vt, B, N, Hq, Hkv, npad, 0, p)
    assert torch.equal(o.view(torch.int16), o2.view(torch.int16)) and torch.equal(lse, lse2)
    for s in (True, False):
        assert torch.equal(g[s].view(torch.int16), run_bwd(q, k, vt, o, dout, lse, cos, sin, B, N, Hq, Hkv, npad, 0, p,
                                                           s).view(torch.int16))
    # sample 1's inputs change: samples 0 and 2 keep every bit of o, lse, dq, dk, dv
    q[N:2 * N] = gen_op((N, Hq * 64), 64)
    vt[1] = gen_op((Hkv, 64, npad), 65)
    vt[1, ..., N:] = 0
    dout[N:2 * N] = gen_op((N, Hq * 64), 66)
    o3, lse3 = run_fwd(q, k, vt, B, N, Hq, Hkv, npad, 0, p)
    keep = torch.ones(B * N, dtype=torch.bool, device=q.device)
    keep[N:2 * N] = False
    assert torch.equal(o3[keep].view(torch.int16), o[keep].view(torch.int16)) and torch.equal(lse3[[0, 2]], lse[[0, 2]])
    for s in (True, False):
        g3 = run_bwd(q, k, vt, o3, dout, lse3, cos, sin, B, N, Hq, Hkv, npad, 0, p, s)
        assert torch.equal(g3[keep].view(torch.int16), g[s][keep].view(torch.int16))


@pytest.fixture(scope="module")
def crossing():
    """B * Hq * N^2 just above 2^32 (B = 52, Hq = 20, N = 2048): the 64-bit-index forms of the forward and of both backward
    kernels run.  Element index ((b*Hq + h)*N + i)*N + j reaches 2^32 at b = 51, h = 4 (KV group 0 of sample 51 spans the
    crossing).  Returns the kernel outputs of two (b, g) slices with their masks; inputs are drawn on the GPU."""
    B, N, Hq, Hkv, p, site = 52, 2048, 20, 4, 0.1, 7 * 8
    assert B * Hq * N * N > 2 ** 32 and (51 * Hq + 4) * N * N == 2 ** 32
    gg = torch.Generator(device=dev()).manual_seed(7)
    q = torch.randn((B * N, Hq * 64), generator=gg, device=dev()).to(OP)
    k = torch.randn((B * N, Hkv * 64), generator=gg, device=dev()).to(OP)
    vt = torch.randn((B, Hkv, 64, N), generator=gg, device=dev()).to(OP)
    dout = torch.randn((B * N, Hq * 64), generator=gg, device=dev()).to(OP)
    cos, sin = rope_tables()
    o, lse = run_fwd(q, k, vt, B, N, Hq, Hkv, N, site, p)
    out = {"fwd": {}, "bwd": {}}
    G = Hq // Hkv
    slices = [(51, 0), (0, 1)]
    for split in (True, False):
        dqkv = run_bwd(q, k, vt, o, dout, lse, cos, sin, B, N, Hq, Hkv, N, site, p, split)
        for b, g in slices:
            rows = slice(b * N, (b + 1) * N)
            hs = slice(g * G * 64, (g + 1) * G * 64)
            out["bwd"][(b, g, split)] = (heads(dqkv[rows, :Hq * 64][:, hs], 1, N, G),
                                         heads(dqkv[rows, Hq * 64 + g * 64:Hq * 64 + (g + 1) * 64], 1, N, 1),
                                         heads(dqkv[rows, (Hq + Hkv) * 64 + g * 64:(Hq + Hkv) * 64 + (g + 1) * 64], 1, N, 1))
        del dqkv
    for b, g in slices:
        rows = slice(b * N, (b + 1) * N)
        hs = slice(g * G * 64, (g + 1) * G * 64)
        start = (b * Hq + g * G) * N * N
        M = torch.from_numpy(OT.drop_mult_range(SEED, site, p, start, G * N * N)).to(dev()).view(1, G, N, N)
        ins = (heads(q[rows][:, hs], 1, N, G), heads(k[rows][:, g * 64:(g + 1) * 64], 1, N, 1),
               vt[b, g].double().transpose(0, 1)[None, None], heads(dout[rows][:, hs], 1, N, G))
        out["fwd"][(b, g)] = (heads(o[rows][:, hs], 1, N, G), lse[b, g * G:(g + 1) * G][None], M, ins)
    return out, cos, sin


@pytest.mark.parametrize("b,g", [(51, 0), (0, 1)])
def test_attention_train_forward_64bit_dropout_index(crossing, b, g):
    out, _, _ = crossing
    o, lse, M, (qh, kh, vh, _) = out["fwd"][(b, g)]
    check_attn_fwd(o, lse, qh, kh, vh, M, f"attention fwd b={b} g={g}")


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("b,g", [(51, 0), (0, 1)])
def test_attention_train_backward_64bit_dropout_index(crossing, b, g, split):
    out, cos, sin = crossing
    o, _, M, (qh, kh, vh, doh) = out["fwd"][(b, g)]
    dq, dk, dv = out["bwd"][(b, g, split)]
    check_attn_bwd(dq, dk, dv, qh, kh, vh, doh, o, M, cos, sin, f"attention bwd b={b} g={g} split={split}")


# ---------------------------------------------------------------------------------------------------------------------
# gradient norm + clip_grad_norm_ + AdamW
# ---------------------------------------------------------------------------------------------------------------------
def _f(x):
    return float(np.float32(x))


@pytest.mark.parametrize("n,step,clip", [(4, 1, True), (1028, 7, False), (1028, 1, True), (1_000_004, 1, False),
                                         (1_000_004, 7, True)])
def test_adamw(n, step, clip):
    ls = 1024.0   # loss scale: inv_scale = 2^-10 exactly
    lr, b1, b2, eps, wd = 1e-3, 0.9, 0.999, 1e-8, 0.01
    p0 = gen((n,), 70)
    g = gen((n,), 71, 0.01 * ls)
    m0 = gen((n,), 72, 1e-3)
    v0 = gen((n,), 73, 1e-3).abs() * 1e-2
    gs = g.double() / ls
    norm = float(gs.norm())
    max_norm = 0.5 * norm if clip else 2.0 * norm
    pb, p = guarded((n,), fill=p0)
    mb, m = guarded((n,), fill=m0)
    vb, v = guarded((n,), fill=v0)
    nb, nrm = guarded((1,))
    wk = work((1024 + 2) * 4)
    call(L.lib().jat_k_adamw, L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), n, lr, b1, b2, eps, wd, max_norm, ls, step, L.ptr(nrm),
         L.ptr(wk), wk.numel() * 4, L.stream_ptr())
    lr, b1, b2, eps, wd, max_norm = map(_f, (lr, b1, b2, eps, wd, max_norm))
    coef = min(1.0, max_norm / (norm + 1e-6))
    assert (coef < 1.0) == clip
    gr = gs * coef
    mr = b1 * m0.double() + (1 - b1) * gr
    vr = b2 * v0.double() + (1 - b2) * gr * gr
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    denom = vr.sqrt() / math.sqrt(bc2) + eps
    pr = p0.double() * (1 - lr * wd) - lr / bc1 * mr / denom
    # fp32 state updates: a handful of roundings (coef from the fp32 norm: 2^-22; products, sums, sqrt, division: <= 8
    # 2^-24) on terms that do not cancel beyond their own magnitudes; gate 1e-5 of those magnitudes
    am = b1 * m0.double().abs() + (1 - b1) * gr.abs()
    assert_within(m, mr, 1e-5 * am, "adamw m")
    assert_within(v, vr, 1e-5 * (b2 * v0.double() + (1 - b2) * gr * gr), "adamw v")
    assert_within(p, pr, 1e-5 * (p0.double().abs() + lr / bc1 * am / denom), "adamw p")
    # the norm of the scaled gradients: fp32 partial sums of squares (g_16), finished in double: 1e-5 relative
    assert abs(float(nrm[0]) - norm * ls) <= 1e-5 * norm * ls
    assert all(guards_intact(x) for x in (pb, mb, vb, nb))


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_adamw_skips_a_non_finite_step(bad):
    n = 1028
    p0, m0, v0 = gen((n,), 80), gen((n,), 81, 1e-3), gen((n,), 82, 1e-3).abs()
    g = gen((n,), 83)
    g[517] = bad
    p, m, v = p0.clone(), m0.clone(), v0.clone()
    nrm = torch.zeros(1, device=p.device)
    wk = work((1024 + 2) * 4)
    call(L.lib().jat_k_adamw, L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), n, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1.0, 1.0, 3, L.ptr(nrm),
         L.ptr(wk), wk.numel() * 4, L.stream_ptr())
    assert torch.equal(p.view(torch.int32), p0.view(torch.int32)) and torch.equal(m.view(torch.int32), m0.view(torch.int32))
    assert torch.equal(v.view(torch.int32), v0.view(torch.int32))
    assert not math.isfinite(float(nrm[0]))


# ---------------------------------------------------------------------------------------------------------------------
# reconstruction loss (MSE / Charbonnier) and its gradient: recon_grad_kernel<CHARB> through jat_k_recon_loss
# ---------------------------------------------------------------------------------------------------------------------
RECON_SWEEP = 1024 * 256 * 4                     # elements one sweep of the grid covers: 1024 blocks x 256 threads x 4
RECON_SIZES = (1, 7, 4099, RECON_SWEEP + 5)      # the scalar tail alone; one vector + tail; many vectors + a tail of 3; a second
#                                                  sweep with one vector and a one-element tail


@functools.lru_cache(maxsize=1)
def recon_inputs():
    """(pred, target) fp32 of the largest size, every size uses a prefix: every third target sits at pred + 2e-3 * noise
    (|d| ~ sqrt(eps)), every ninth element from index 4 on has pred == target (index 0 keeps a non-zero difference)."""
    import jatsr_amd.recipe as recipe
    n = max(RECON_SIZES)
    pred, target, near = (recipe.gaussian("recon_" + k, (n,), 900 + i) for i, k in enumerate(("pred", "target", "near")))
    target[::3] = pred[::3] + np.float32(2e-3) * near[::3]
    target[4::9] = pred[4::9]
    return pred, target


@pytest.mark.parametrize("eps", [0.0, 1e-6])
@pytest.mark.parametrize("n", RECON_SIZES)
def test_recon_loss_vector_body_tail_and_second_sweep(n, eps):
    """jat_k_recon_loss against fp64 numpy where the merged kernel changes form, at loss_scale 1 and 1024 (it scales the gradient
    only).  Gates of test_charbonnier_kernel_vs_reference_function: loss 2e-6 relative, dpred rel-L2 2e-6, exact 0 where
    pred == target."""
    pred, target = (x[:n] for x in recon_inputs())
    d = pred.astype(np.float64) - target.astype(np.float64)
    if eps > 0:
        r = np.sqrt(d * d + eps)
        loss_ref, g_ref = float(r.mean()), d / r / n
    else:
        loss_ref, g_ref = float((d * d).mean()), 2 * d / n
    assert loss_ref > 0
    p_d, t_d = torch.from_numpy(pred.copy()).to(dev()), torch.from_numpy(target.copy()).to(dev())
    for scale in (1.0, 1024.0):
        gb, g = guarded((n,))
        ob, out = guarded((1,))
        wk = work((1024 + 2) * 4)
        call(L.lib().jat_k_recon_loss, L.ptr(p_d), L.ptr(t_d), L.ptr(g), L.ptr(out), n, eps, scale, L.ptr(wk), wk.numel() * 4,
             L.stream_ptr())
        got = g.cpu().numpy().astype(np.float64) / scale
        loss_err = abs(float(out[0]) - loss_ref) / loss_ref
        g_err = float(np.linalg.norm(got - g_ref) / np.linalg.norm(g_ref))
        print(f"n {n} eps {eps} scale {scale}: loss rel err {loss_err:.3e}, dpred rel-L2 {g_err:.3e}")
        assert loss_err <= 2e-6
        assert g_err <= 2e-6
        assert np.all(got[4::9] == 0.0) and np.isfinite(got).all()
        assert guards_intact(gb) and guards_intact(ob)


# ---------------------------------------------------------------------------------------------------------------------
# small-batch Linear backward (adaLN modulation and t_embedder)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,K,silu,ldy_pad,with_db", [
    (1, 7, 4, False, 0, True), (64, 16, 100, True, 3, True), (64, 7680, 1280, True, 0, True), (17, 16389, 100, False, 5, False),
    (3, 16389, 1280, True, 0, True)])
def test_small_dw(B, N, K, silu, ldy_pad, with_db):
    ldy, ldx = N + ldy_pad, K + (4 if K == 100 else 0)
    dy = gen((B, ldy), 90)
    x = gen((B, ldx), 91, 2.0)
    dwb, dW = guarded((N, K))
    dbb, db = guarded((N,))
    call(L.lib().jat_k_small_dw, L.ptr(dy), ldy, L.ptr(x), ldx, L.ptr(dW), L.ptr(db) if with_db else None, B, N, K, int(silu),
         L.stream_ptr())
    xd = x.double()[:, :K]
    xs = xd * torch.sigmoid(xd) if silu else xd
    dyd = dy.double()[:, :N]
    # B serial fp32 FMAs per output (g_B) on exact-operand products; silu in fp32 with __expf: (|x| + 4) 2^-24 relative
    # (|x| < 12 here); gate (B + 16) 2^-23 of sum_b |dy x'|
    assert_within(dW, dyd.T @ xs, (B + 16) * 2 * F32 * (dyd.abs().T @ xs.abs()), "small_dw dW")
    if with_db:
        assert_within(db, dyd.sum(0), B * F32 * dyd.abs().sum(0), "small_dw db")
    else:
        assert bool(torch.isnan(db).all())
    assert guards_intact(dwb) and guards_intact(dbb)
    dW2 = torch.empty_like(dW)
    call(L.lib().jat_k_small_dw, L.ptr(dy), ldy, L.ptr(x), ldx, L.ptr(dW2), None, B, N, K, int(silu), L.stream_ptr())
    assert torch.equal(dW, dW2)


@pytest.mark.parametrize("B,N,K,w_bf16,acc,silu", [
    (1, 7, 4, True, False, False), (32, 16, 100, False, True, False), (32, 7680, 1280, True, False, True),
    (7, 16389, 100, False, False, True), (32, 16389, 1280, True, True, False), (5, 16384, 4, False, False, False)])
def test_small_dx(B, N, K, w_bf16, acc, silu):
    ldy = N + 3
    dy = gen((B, ldy), 100)
    W32 = gen((N, K), 101, 0.05)
    W = W32.to(OP) if w_bf16 else W32
    Wd = W.double()
    pre = gen((B, K), 102, 2.0) if silu else None
    xb, dx = guarded((B, K), fill=gen((B, K), 103) if acc else NAN)
    old = dx.clone()
    slab = 256 if N >= 16384 else 32
    nsplit = (N + slab - 1) // slab
    wk = work(nsplit * B * K * 4)

    def run(dxv):
        call(L.lib().jat_k_small_dx, L.ptr(dy), ldy, L.ptr(W), int(w_bf16), L.ptr(dxv), B, N, K, int(acc), L.ptr(pre),
             L.ptr(wk), wk.numel() * 4, L.stream_ptr())
    run(dx)
    dyd = dy.double()[:, :N]
    s = dyd @ Wd
    A = dyd.abs() @ Wd.abs()
    # a slab of <= slab rows summed serially, then nsplit slab partials in order: g_(slab + nsplit) of sum_n |dy W|
    bound = (slab + nsplit + 2) * F32 * A
    ref = s + (old.double() if acc else 0)
    if acc:
        bound = bound + 2 * F32 * (old.double().abs() + s.abs())
    if silu:
        u = pre.double()
        sg = torch.sigmoid(u)
        ds = sg * (1 + u * (1 - sg))
        # silu' in fp32 with __expf: < (|u| + 4) 2^-24 absolute for |u| < 12
        bound = bound * ds.abs() + (u.abs() + 4) * F32 * ref.abs()
        ref = ref * ds
    assert_within(dx, ref, bound, "small_dx")
    assert guards_intact(xb)
    dx2 = old.clone()
    run(dx2)
    assert torch.equal(dx, dx2)
    if B > 1:   # another sample's dy does not reach this sample's dx
        dy[0] = gen((ldy,), 104)
        dx2.copy_(old)
        run(dx2)
        assert torch.equal(dx[1:], dx2[1:])


# ---------------------------------------------------------------------------------------------------------------------
# validation: shapes the launchers do not take come back as ValueError (JAT_E_INVALID) without a launch
# ---------------------------------------------------------------------------------------------------------------------
def test_training_entries_reject_unsupported_shapes():
    lib, s = L.lib(), L.stream_ptr()
    f = torch.zeros(1 << 16, device=dev())
    h = torch.zeros(1 << 16, dtype=OP, device=dev())
    wk = work(1 << 16)
    P, WB = L.ptr(f), wk.numel() * 4

    def rejected(rc):
        with pytest.raises(ValueError):
            L.check(rc)
    for D in (384, 2304, 0):      # norm_bwd takes D = 256 .. 2048 in steps of 256
        rejected(lib.jat_k_norm_bwd(P, L.ptr(h), None, None, 0, P, 0, None, None, 0, None, 1, D, 2, 0, L.ptr(wk), WB, s))
    rejected(lib.jat_k_norm_bwd(P, L.ptr(h), P, None, 0, P, 0, None, None, 0, None, 1, 256, 2, 1, L.ptr(wk), WB, s))
    rejected(lib.jat_k_norm_bwd(P, L.ptr(h), None, None, 0, P, 0, None, None, 0, None, 1, 256, 2, 0, L.ptr(wk), 16, s))
    rejected(lib.jat_k_small_dw(P, 8, P, 8, P, P, 65, 8, 8, 0, s))
    rejected(lib.jat_k_small_dw(P, 8, P, 8, P, P, 2, 8, 6, 0, s))
    rejected(lib.jat_k_small_dx(P, 8, P, 0, P, 33, 8, 8, 0, None, L.ptr(wk), WB, s))
    rejected(lib.jat_k_small_dx(P, 8, P, 0, P, 2, 8, 8, 0, None, L.ptr(wk), 32, s))
    rejected(lib.jat_k_attention_train(L.ptr(h), L.ptr(h), L.ptr(h), L.ptr(h), P, 1, 2049, 4, 2, 2112, SEED, 0, 0.1, s))
    rejected(lib.jat_k_attention_train(L.ptr(h), L.ptr(h), L.ptr(h), L.ptr(h), P, 1, 64, 5, 2, 64, SEED, 0, 0.1, s))
    rejected(lib.jat_k_attention_train(L.ptr(h), L.ptr(h), L.ptr(h), L.ptr(h), P, 1, 64, 4, 2, 64, SEED, 0, 1.0, s))
    rejected(lib.jat_k_attention_bwd(*[L.ptr(h)] * 5, P, L.ptr(h), P, P, 1, 64, 4, 2, 32, SEED, 0, 0.1, 1, L.ptr(wk), WB, s))
    rejected(lib.jat_k_attention_bwd(*[L.ptr(h)] * 5, P, L.ptr(h), P, P, 1, 64, 4, 2, 64, SEED, 0, 0.1, 1, L.ptr(wk), 1024, s))
    rejected(lib.jat_k_gate_bwd(P, L.ptr(h), P, 8, L.ptr(h), P, 8, 1, 6, 2, SEED, 1, 0.0, 3, 0.0, L.ptr(wk), WB, s))
    rejected(lib.jat_k_gate_bwd(P, L.ptr(h), P, 8, L.ptr(h), P, 8, 1, 8, 2, SEED, 1, 0.0, 3, 0.0, L.ptr(wk), 16, s))
    rejected(lib.jat_k_resid_gate(P, L.ptr(h), P, 12, P, 2, 12, 2, SEED, 1, 0.0, 3, 0.0, s))
    rejected(lib.jat_k_gelu(L.ptr(h), L.ptr(h), 12, SEED, 2, 0.1, s))
    rejected(lib.jat_k_gelu_bwd(L.ptr(h), L.ptr(h), 16, SEED, 2, -0.1, s))
    rejected(lib.jat_k_adamw(P, P, P, P, 6, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 1.0, 1, None, L.ptr(wk), WB, s))
    rejected(lib.jat_k_adamw(P, P, P, P, 8, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 1.0, 0, None, L.ptr(wk), WB, s))
    rejected(lib.jat_k_adamw(P, P, P, P, 8, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 1.0, 1, None, L.ptr(wk), 64, s))
    torch.cuda.synchronize()
    assert bool((f == 0).all()) and bool((h == 0).all())
