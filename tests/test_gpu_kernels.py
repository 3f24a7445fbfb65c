"""Per-kernel parity on the GPU, through the C ABI (include/jat_hip.h `jat_k_*`).

Each HIP kernel is compared with a plain PyTorch evaluation of the same op on the SAME bf16-rounded
operands (fp64 accumulate), so the only admissible differences are fp32 accumulation order and the final
bf16 rounding: tolerances are stated per test.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import jatsr_amd._lib as L  # noqa: E402

import forward_ref as R  # noqa: E402

# operand dtype of the loaded library: bf16, or fp16 when the process runs with JAT_OPERAND_DTYPE=fp16 (the v3mod2 trainer's
# autocast dtype; tests/test_gpu_fp16.py re-runs this module that way).  fp16 has 3 more mantissa bits: same gates hold.
OP = torch.float16 if L.OPERAND_DTYPE == "fp16" else torch.bfloat16


def dev():
    L.require_gpu()
    return torch.device("cuda:0")


def bf16_bits(t):  # fp32 tensor -> (uint16-bits tensor as int16 view, rounded fp32 values)
    b = t.to(OP)
    return b, b.float()


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def gen(shape, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dev())


def test_cast_bf16():
    x = gen((3, 1001), 1)
    out = torch.empty(x.shape, dtype=OP, device=x.device)
    L.check(L.lib().jat_k_cast_bf16(L.ptr(x), L.ptr(out), x.numel(), L.stream_ptr()))
    assert torch.equal(out, x.to(OP))


MANT = 10 if OP == torch.float16 else 7          # stored mantissa bits of OP
EMIN = -24 if OP == torch.float16 else -133      # exponent of OP's smallest subnormal
F32 = 2.0 ** -24                                 # unit roundoff of fp32
GUARD = 256                                      # elements of NaN on each side of the norm tests' output


def op_ulp(r):
    """Spacing of OP at each element of r (values representable in OP, as float64); `ulp` of tests/test_gpu_train_kernels.py."""
    _, e = torch.frexp(r.float())
    u = torch.pow(2.0, (e - 1 - MANT).clamp_min(EMIN).double())
    return torch.where(r == 0, torch.full_like(u, 2.0 ** EMIN), u)


def norm_modulate_case(x, w, shift, scale, mod_bstride, ntok, mode, what):
    """jat_k_norm_modulate on x [M, D] into a NaN-filled output between NaN guard bands, against fp64:
      - every element within one OP ulp of the fp64 result rounded to OP (its own rounding, plus the fp32 error before it, which
        moves it across at most one rounding boundary), plus that fp32 error: the statistics are D-term fp32 sums (sum of squares,
        and the mean for LayerNorm), g_D = D * 2^-24 relative to the sum of their absolute terms as tests/test_gpu_train_kernels.py
        derives it — the sum of squares has no cancellation, so rstd carries at most g_D / 2, the mean g_D * mean|x| — and the
        element-wise chain (x - mu) * rstd * w * (1 + scale) + shift adds <= 8 roundings of 2^-24 on |n (1 + scale)| + |shift|;
      - the guard bands untouched, no NaN left inside;
      - the rel-L2 gate the norm tests always had (3e-3: one OP rounding of the result).
    shift / scale: [B or 1, D] views (row stride mod_bstride, 0 = one row for every sample) or None; w: [D] or None."""
    M, D = x.shape
    buf = torch.full((M * D + 2 * GUARD,), float("nan"), device=x.device).to(OP)
    y = buf[GUARD:GUARD + M * D].view(M, D)
    L.check(L.lib().jat_k_norm_modulate(L.ptr(x), L.ptr(w), C.c_void_p(shift.data_ptr()) if shift is not None else None,
                                        C.c_void_p(scale.data_ptr()) if scale is not None else None, mod_bstride, L.ptr(y), M, D,
                                        ntok, mode, L.stream_ptr()))
    torch.cuda.synchronize()
    xd = x.double()
    ax = xd.abs().mean(-1, keepdim=True)
    if mode == 0:
        rstd = 1 / torch.sqrt((xd * xd).mean(-1, keepdim=True) + 1e-6)
        n = xd * rstd * (w.double() if w is not None else 1.0)
    elif mode == 1:
        mu = xd.mean(-1, keepdim=True)
        rstd = 1 / torch.sqrt(((xd - mu) ** 2).mean(-1, keepdim=True) + 1e-6)
        n = (xd - mu) * rstd
    else:
        rstd = torch.zeros_like(ax)
        n = xd
    bidx = torch.arange(M, device=x.device) // ntok if mod_bstride else torch.zeros(M, dtype=torch.long, device=x.device)
    one_plus = 1 + scale.double()[bidx] if scale is not None else torch.ones_like(n)
    sh = shift.double()[bidx] if shift is not None else torch.zeros_like(n)
    ref = n * one_plus + sh
    g_d = D * F32
    bound = (g_d / 2 + 8 * F32) * ((n * one_plus).abs() + sh.abs())
    if mode == 1:
        bound = bound + g_d * ax * rstd * one_plus.abs()
    assert bool(torch.isnan(buf[:GUARD].float()).all()) and bool(torch.isnan(buf[-GUARD:].float()).all()), what
    assert bool(torch.isfinite(y).all()), what
    r = ref.to(OP).double()
    err = (y.double() - r).abs()
    tol = op_ulp(r) + bound
    bad = ~(err <= tol)
    print(f"{what}: worst element at {float((err / tol).max()):.3f} of its bound, rel-L2 {rel(y, ref):.3e}")
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} / {bad.numel()} elements out of bound; first at "
                                 f"{np.unravel_index(int(bad.flatten().nonzero()[0]), tuple(bad.shape))}, "
                                 f"err {float(err[bad].flatten()[0]):.3e} tol {float(tol[bad].flatten()[0]):.3e}")
    # fp32 statistics, one bf16 rounding of the result (2^-9 relative)
    assert (y.double() - ref).abs().max() <= 2 ** -8 * ref.abs().max() + 1e-6
    assert rel(y, ref) < 3e-3


# 256 / 512 / 1280 run norm_modulate_rows_kernel<1, 2, 5>, every other width norm_modulate_kernel (launch_norm_modulate); the first
# three cases are the original ones, the other widths take the same (M, ntok) pairs and one more with M % 4 == 3 (the last block's
# fourth wave has no row) and a ragged last sample
NORM_WIDTHS = [768, 1024, 1536, 1792, 2048]
NORM_SHAPES = [(1280, 257, 64, False), (512, 64, 32, True), (256, 9, 3, False)] + \
              [(D, M, ntok, sh) for D in NORM_WIDTHS for M, ntok, sh in ((257, 64, False), (64, 32, True), (9, 3, False), (131, 50, False))] + \
              [(D, 131, 50, False) for D in (256, 512, 1280)]


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("D,M,ntok,shared", NORM_SHAPES)
def test_norm_modulate(mode, D, M, ntok, shared):
    B = (M + ntok - 1) // ntok
    x = gen((M, D), 2, 3.0) + 0.5
    w = 1 + 0.2 * gen((D,), 3)
    mod = gen((1 if shared else B, 2 * D), 4, 0.3)
    norm_modulate_case(x, w, mod[:, :D], mod[:, D:], 0 if shared else 2 * D, ntok, mode, f"norm_modulate D={D} M={M} mode {mode}")


def test_norm_no_modulation():
    """The final norm's form (weight, no shift / scale) at every width: 1280 on the rows kernel, the others on norm_modulate_kernel."""
    for D, M in [(1280, 37)] + [(D, 37) for D in NORM_WIDTHS]:
        x = gen((M, D), 5)
        w = 1 + 0.2 * gen((D,), 6)
        norm_modulate_case(x, w, None, None, 0, M, 0, f"norm without modulation D={D}")


GEMM_SHAPES = [(128, 128, 64), (256, 512, 128), (1000, 1792, 1280), (56, 1536, 256), (1035, 1280, 5120),
               (384, 256, 8192),
               # N divisible by 160 / 320 / 448 (the wide tiles), K-tile counts 1, 2, 3 (pipeline prologue / tail paths)
               (300, 2240, 64), (300, 2240, 128), (500, 4480, 192),
               # more tiles than CUs: the one-block-per-CU variants walk several tiles per block (persistent launch)
               (4500, 4480, 128)]


# every live tile / pipeline variant of gemm.hip (ids are stable; the structures measured and retired in rounds 1-2 are
# rejected by launch_gemm: test_retired_gemm_variants_are_rejected); JAT_TEST_VARIANTS="31,32" narrows the sweep
LIVE_VARIANTS = [10, 18, 20, 21, 25, 26, 27, 28, 31, 32, 33, 34, 35, 36, 38, 39]
GEMM_VARIANTS = [int(v) for v in os.environ.get("JAT_TEST_VARIANTS", "").split(",") if v] or LIVE_VARIANTS


@pytest.mark.parametrize("variant", GEMM_VARIANTS)
@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
@pytest.mark.parametrize("epi", [0, 1, 2, 3])
def test_gemm(variant, M, N, K, epi):
    """C = A W^T (+bias) with epilogues fp32 / bf16 / bf16-GELU / gated residual; ragged M, asymmetric data."""
    A, Af = bf16_bits(gen((M, K), 10 + epi))
    W, Wf = bf16_bits(gen((N, K), 20 + epi, 1.0 / np.sqrt(K)))
    bias = gen((N,), 30, 0.1)
    ntok = 7 if M % 7 == 0 else (M if M < 64 else 23)
    B = (M + ntok - 1) // ntok
    gate = gen((B, N), 31, 0.5)
    ref = Af.double() @ Wf.double().T + bias.double()
    if epi == 0:
        out = torch.full((M, N), float("nan"), device=A.device)
    elif epi in (1, 2):
        out = torch.zeros((M, N), dtype=OP, device=A.device)
    else:
        out = gen((M, N), 32)
        x0 = out.clone()
    L.check(L.lib().jat_k_gemm(L.ptr(A), L.ptr(W), L.ptr(bias), L.ptr(out), M, N, K, epi, L.ptr(gate), N, ntok,
                               variant, L.stream_ptr()))
    torch.cuda.synchronize()
    if epi == 0:
        assert rel(out, ref) < 2e-6
        assert (out.double() - ref).abs().max() < 1e-4 * max(1.0, float(ref.abs().max()))
    elif epi == 1:
        assert rel(out, ref) < 3e-3
        assert torch.equal(out, ref.float().to(OP)) or (out.float() - ref.float()).abs().max() <= \
            2 ** -8 * float(ref.abs().max())
    elif epi == 2:
        g = torch.nn.functional.gelu(ref)  # erf form, fp64
        assert (out.double() - g).abs().max() <= 2 ** -8 * float(g.abs().max()) + 1e-6
        assert rel(out, g) < 3e-3
    else:
        bidx = torch.arange(M, device=A.device) // ntok
        r = x0.double() + gate.double()[bidx] * ref
        assert rel(out, r) < 2e-6


def _fold_case(M, N, K, ntok, seed):
    A, Af = bf16_bits(gen((M, K), seed))
    W, Wf = bf16_bits(gen((N, K), seed + 1, 1.0 / np.sqrt(K)))
    bias = gen((N,), seed + 2, 0.1)
    B = (M + ntok - 1) // ntok
    gate = gen((B, N), seed + 3, 0.5)
    x0 = gen((M, N), seed + 4, 2.0)
    hi0 = x0.to(OP)
    lo0 = (x0 - hi0.float()).to(OP)
    return A, Af, W, Wf, bias, gate, hi0, lo0


@pytest.mark.parametrize("variant", [20, 25, 32])
@pytest.mark.parametrize("M,N,K,ntok", [(300, 1280, 256, 128), (512, 1280, 128, 128), (300, 1280, 192, 23), (700, 1280, 64, 345)])
@pytest.mark.parametrize("epi", [0, 3])
def test_gemm_fold_producer(variant, M, N, K, ntok, epi):
    """Split-residual epilogue of the sampler's folded norms (jat_k_gemm_fold): x_new = acc + bias (epilogue 0) or
    (hi + lo) + gate (acc + bias) (epilogue 3, jat_audiosr_v3.py:300,306) kept as two 16-bit planes, plus the row partial
    sums of x_new^2 the consumer's rstd is built from; ragged M, wave tiles inside one sample / across two / across many."""
    A, Af, W, Wf, bias, gate, hi0, lo0 = _fold_case(M, N, K, ntok, 200 + epi)
    if N % (L.lib().jat_k_gemm_wave_n(variant) or 1) != 0:
        pytest.skip("tile does not divide N")
    wn = L.lib().jat_k_gemm_wave_n(variant)
    hi, lo = hi0.clone(), lo0.clone()
    part = torch.full((M, N // wn), float("nan"), device=A.device)
    L.check(L.lib().jat_k_gemm_fold(L.ptr(A), L.ptr(W), L.ptr(bias), None, M, N, K, epi, L.ptr(gate), N, ntok, L.ptr(hi),
                                    L.ptr(lo), L.ptr(part), None, 0, variant, L.stream_ptr()))
    torch.cuda.synchronize()
    y = Af.double() @ Wf.double().T + bias.double()
    if epi == 3:
        bidx = torch.arange(M, device=A.device) // ntok
        ref = (hi0.double() + lo0.double()) + gate.double()[bidx] * y
    else:
        ref = y
    got = hi.double() + lo.double()
    # hi = round(x), lo = round(x - hi): 16 significant bits (bf16) / 22 (fp16)
    assert (got - ref).abs().max() <= 2 ** -15 * float(ref.abs().max()) + 1e-6
    # hi alone is x rounded to the operand dtype: it is the next GEMM's A operand as it stands
    assert ((hi.double() - ref).abs() <= 2 ** -8 * ref.abs() + 1e-6).all()
    assert rel(part.double().sum(1), (ref * ref).sum(1)) < 1e-5


@pytest.mark.parametrize("M,N,K,ntok", [(224, 160, 64, 128), (448, 1280, 128, 128), (448, 1280, 192, 23), (672, 320, 256, 345),
                                        (7168, 1280, 1280, 128), (7168, 1280, 5120, 128)])
@pytest.mark.parametrize("epi", [0, 3])
def test_gemm_kpair_kernel(M, N, K, ntok, epi):
    """Variant 39 (gemm_kpair_kernel: 224 x 160 tile, two wave groups on the two k-steps of every K-tile, three LDS stages,
    partial accumulators exchanged through LDS) on the split-residual producer epilogues: against fp64, 1 / 2 / 3 / 4 / 20 / 80
    K-tiles (every prologue and tail path), wave tiles inside one sample and across several; and deterministic."""
    A, Af, W, Wf, bias, gate, hi0, lo0 = _fold_case(M, N, K, ntok, 240 + epi)
    res = []
    for _ in range(2):
        hi, lo = hi0.clone(), lo0.clone()
        part = torch.full((M, N // 80), float("nan"), device=A.device)
        L.check(L.lib().jat_k_gemm_fold(L.ptr(A), L.ptr(W), L.ptr(bias), None, M, N, K, epi, L.ptr(gate), N, ntok, L.ptr(hi),
                                        L.ptr(lo), L.ptr(part), None, 0, 39, L.stream_ptr()))
        torch.cuda.synchronize()
        res.append((hi, lo, part))
    assert all(torch.equal(a, b) for a, b in zip(*res))
    hi, lo, part = res[0]
    y = Af.double() @ Wf.double().T + bias.double()
    if epi == 3:
        bidx = torch.arange(M, device=A.device) // ntok
        ref = (hi0.double() + lo0.double()) + gate.double()[bidx] * y
    else:
        ref = y
    assert ((hi.double() + lo.double()) - ref).abs().max() <= 2 ** -15 * float(ref.abs().max()) + 1e-5
    assert ((hi.double() - ref).abs() <= 2 ** -8 * ref.abs() + 1e-5).all()
    assert rel(part.double().sum(1), (ref * ref).sum(1)) < 1e-5


@pytest.mark.parametrize("variant,M,N,K,ksplit", [(39, 224, 160, 384, 2), (39, 448, 320, 1280, 2), (39, 3584, 1280, 5120, 2),
                                                  (39, 224, 1280, 2560, 4), (20, 200, 256, 512, 2), (20, 3584, 1280, 5120, 2)])
def test_gemm_splitk_slices(variant, M, N, K, ksplit):
    """Split-K slices (jat_k_gemm_splitk): slice z = the product over its K columns alone, for the plain 128 x 128 tile and for
    the 224 x 160 k-step-pair tile the half-size forward (BASELINE configs[1], M = 3584) cuts fc2 with; every slice against
    fp64, the rest of the workspace untouched, deterministic."""
    A, Af = bf16_bits(gen((M, K), 260))
    W, Wf = bf16_bits(gen((N, K), 261, 1.0 / np.sqrt(K)))
    res = []
    for _ in range(2):
        parts = torch.full((ksplit + 1, M, N), float("nan"), device=A.device)
        L.check(L.lib().jat_k_gemm_splitk(L.ptr(A), L.ptr(W), L.ptr(parts), M, N, K, ksplit, variant, L.stream_ptr()))
        torch.cuda.synchronize()
        res.append(parts)
    assert torch.equal(res[0][:ksplit], res[1][:ksplit]) and torch.isnan(res[0][ksplit]).all()
    ks = K // ksplit
    for z in range(ksplit):
        ref = Af[:, z * ks:(z + 1) * ks].double() @ Wf[:, z * ks:(z + 1) * ks].double().T
        assert (res[0][z].double() - ref).abs().max() < 2e-5 * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("variant", [31, 36])
@pytest.mark.parametrize("np_", [4, 8, 16])
@pytest.mark.parametrize("epi", [1, 2])
def test_gemm_fold_consumer(variant, np_, epi):
    """Consumer side: accumulator rows scaled by rsqrt(sum_j part[m][j] / K + 1e-6) before the bias (the RMSNorm statistic
    of jat_audiosr_v3.py:297,303 applied after the matmul), bf16 / GELU outputs; 36 = 31 + pipelined epilogue, bit-identical."""
    M, N, K, ntok = 500, 2240, 192, 128
    A, Af = bf16_bits(gen((M, K), 220))
    W, Wf = bf16_bits(gen((N, K), 221, 1.0 / np.sqrt(K)))
    bias = gen((N,), 222, 0.1)
    part = gen((M, np_), 223).abs() * K / np_ + 0.1
    out = torch.zeros((M, N), dtype=OP, device=A.device)
    L.check(L.lib().jat_k_gemm_fold(L.ptr(A), L.ptr(W), L.ptr(bias), L.ptr(out), M, N, K, epi, None, 0, ntok, None, None, None,
                                    L.ptr(part), np_, variant, L.stream_ptr()))
    torch.cuda.synchronize()
    rstd = torch.rsqrt(part.double().sum(1, keepdim=True) / K + 1e-6)
    ref = rstd * (Af.double() @ Wf.double().T) + bias.double()
    if epi == 2:
        ref = torch.nn.functional.gelu(ref)
    assert rel(out, ref) < 3e-3
    if variant == 36:
        out31 = torch.zeros_like(out)
        L.check(L.lib().jat_k_gemm_fold(L.ptr(A), L.ptr(W), L.ptr(bias), L.ptr(out31), M, N, K, epi, None, 0, ntok, None, None,
                                        None, L.ptr(part), np_, 31, L.stream_ptr()))
        torch.cuda.synchronize()
        assert torch.equal(out, out31)


@pytest.mark.parametrize("M,N,K", [(448, 640, 128), (3808, 5120, 64), (3808, 5120, 128), (3808, 5120, 192), (7168, 5120, 1280),
                                   (57568, 320, 256)])
@pytest.mark.parametrize("epi,use_part,use_bias", [(2, True, True), (1, True, False), (2, False, True), (1, False, False)])
def test_gemm_persistent_two_tile_kernel(M, N, K, epi, use_part, use_bias):
    """Variant 38 (gemm_persist_kernel: one block per CU walks two 224 x 320 tiles, the second tile's first K-tile, bias slice
    and row statistics prefetched under the first tile's epilogue) is bit-identical to the one-tile kernel (variant 36) and
    right against fp64: one tile per block, 16 / all blocks with two tiles, 1 / 2 / 3 / 20 K-tiles (every prologue / tail path),
    with and without the consumer's row statistics and bias."""
    A, Af = bf16_bits(gen((M, K), 230))
    W, Wf = bf16_bits(gen((N, K), 231, 1.0 / np.sqrt(K)))
    bias = gen((N,), 232, 0.1) if use_bias else None
    part = (gen((M, 16), 233).abs() * K / 16 + 0.1) if use_part else None
    outs = []
    for variant in (36, 38):
        out = torch.full((M, N), float("nan"), device=A.device).to(OP)
        L.check(L.lib().jat_k_gemm_fold(L.ptr(A), L.ptr(W), L.ptr(bias), L.ptr(out), M, N, K, epi, None, 0, 128, None, None, None,
                                        L.ptr(part), 16 if use_part else 0, variant, L.stream_ptr()))
        torch.cuda.synchronize()
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    if M * N <= 3808 * 5120:
        ref = Af.double() @ Wf.double().T
        if use_part:
            ref = ref * torch.rsqrt(part.double().sum(1, keepdim=True) / K + 1e-6)
        if use_bias:
            ref = ref + bias.double()
        if epi == 2:
            ref = torch.nn.functional.gelu(ref)
        assert rel(outs[1], ref) < 3e-3


@pytest.mark.parametrize("tokens,out,inn,ksplit", [
    (64, 128, 128, 1), (1, 128, 128, 1), (100, 128, 256, 1), (1000, 384, 256, 1), (1000, 384, 256, 4),
    (2583, 256, 640, 3), (9660, 1280, 1280, 4), (9660, 5120, 1280, 1), (6182, 1280, 5120, 2),
    # 256 x 256 tiles (out * in >= 2^20): automatic split, ragged and < 64-token batches, one K-tile per slice
    (9660, 1280, 1280, 0), (9660, 3840, 1280, 0), (2583, 1024, 1024, 0), (37, 1024, 1024, 1), (4096, 1024, 1280, 7),
    (130, 1024, 1024, 3), (9660, 5120, 1280, 0)])
def test_weight_grad(tokens, out, inn, ksplit):
    """dW = dY^T X and db = column sums of dY straight from the token-major operands (gemm_tn.hip): ragged token counts
    (last K-tile zero-filled in LDS), split-K summed in order, no transposed copies.  The buffers are allocated exactly
    `tokens` rows long inside a poisoned arena: whatever follows them must not leak into the sums."""
    arena_y = torch.full(((tokens + 64) * out,), float("nan"), device=dev()).to(OP)
    arena_x = torch.full(((tokens + 64) * inn,), float("nan"), device=dev()).to(OP)
    dY = arena_y[:tokens * out].view(tokens, out)
    X = arena_x[:tokens * inn].view(tokens, inn)
    dY.copy_(gen((tokens, out), 40, 0.05).to(OP))
    X.copy_((gen((tokens, inn), 41) + 0.25).to(OP))
    dW = torch.full((out, inn), float("nan"), device=dev())
    db = torch.full((out,), float("nan"), device=dev())
    work = torch.full((64 + 16 * out * inn + 32 * out,), float("nan"), device=dev())
    L.check(L.lib().jat_k_weight_grad(L.ptr(dY), L.ptr(X), L.ptr(dW), L.ptr(db), tokens, out, inn, ksplit, L.ptr(work),
                                      work.numel() * 4, L.stream_ptr()))
    torch.cuda.synchronize()
    ref = dY.double().T @ X.double()
    assert rel(dW, ref) < 3e-6
    assert (dW.double() - ref).abs().max() < 2e-5 * max(1.0, float(ref.abs().max()))
    rb = dY.double().sum(0)
    assert (db.double() - rb).abs().max() < 2e-5 * max(1.0, float(rb.abs().max()))
    # bit-reproducible: fixed-order partial sums, no atomics
    dW2 = torch.empty_like(dW)
    L.check(L.lib().jat_k_weight_grad(L.ptr(dY), L.ptr(X), L.ptr(dW2), None, tokens, out, inn, ksplit, L.ptr(work),
                                      work.numel() * 4, L.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(dW, dW2)


def test_weight_grad_rejects_unsupported_shapes():
    z = torch.zeros((64, 192), device=dev()).to(OP)
    o = torch.zeros((192, 192), device=dev())
    assert L.lib().jat_k_weight_grad(L.ptr(z), L.ptr(z), L.ptr(o), None, 64, 192, 192, 1, None, 0, L.stream_ptr()) != 0


def test_retired_gemm_variants_are_rejected():
    A = torch.zeros(128, 64, dtype=OP, device=dev())
    out = torch.zeros(128, 128, device=dev())
    for v in [v for v in range(-1, 40) if v not in LIVE_VARIANTS]:
        rc = L.lib().jat_k_gemm(L.ptr(A), L.ptr(A), None, L.ptr(out), 128, 128, 64, 0, None, 0, 128, v, L.stream_ptr())
        assert rc != 0, v


def _attention_ref(q, k, v, B, N, Hq, Hkv, lens=None):
    """tests/forward_ref.py `attention_heads` (fp64; with lens: the keys >= lens[b] at -inf for every query row of sample b)"""
    return R.attention_heads(q, k, v, B, N, Hq, Hkv, lens)


@pytest.mark.parametrize("B,N,Hq,Hkv", [(2, 128, 20, 4), (1, 345, 20, 4), (3, 6, 4, 2), (1, 1024, 8, 4), (2, 70, 4, 4)])
def test_attention(B, N, Hq, Hkv):
    """softmax(q k^T/8) v with GQA head sharing; N ragged w.r.t. the 64-key block and the 128-query block."""
    npad = (N + 63) // 64 * 64
    q, qf = bf16_bits(gen((B * N, Hq * 64), 40, 1.5))
    k, kf = bf16_bits(gen((B * N, Hkv * 64), 41, 1.5))
    v, vf = bf16_bits(gen((B * N, Hkv * 64), 42))
    vt = torch.zeros(B, Hkv, 64, npad, dtype=OP, device=q.device)
    vt[:, :, :, :N] = v.view(B, N, Hkv, 64).permute(0, 2, 3, 1)
    o = torch.zeros(B * N, Hq * 64, dtype=OP, device=q.device)
    L.check(L.lib().jat_k_attention(L.ptr(q), L.ptr(k), L.ptr(vt), L.ptr(o), B, N, Hq, Hkv, npad, L.stream_ptr()))
    ref = _attention_ref(qf, kf, vf, B, N, Hq, Hkv)
    # P is rounded to bf16 before PV and the output once more: ~2^-8 relative to the value scale
    assert rel(o, ref) < 6e-3
    assert (o.double() - ref).abs().max() < 2e-2 * float(ref.abs().max())


def test_attention_spiky_rows():
    """Online-softmax rescale across key blocks: one key in the LAST block dominates a query row."""
    B, N, Hq, Hkv = 1, 256, 4, 2
    npad = 256
    qx = gen((B * N, Hq * 64), 50)
    kx = gen((B * N, Hkv * 64), 51)
    kx[200, :64] = qx[5, :64] * 4.0  # query 5 of head 0 / kv-head 0 spikes at key 200 (4th block)
    kx[3, 64:] = qx[77, 128:192] * 4.0  # head 2 -> kv head 1 spikes in the first block
    q, qf = bf16_bits(qx)
    k, kf = bf16_bits(kx)
    v, vf = bf16_bits(gen((B * N, Hkv * 64), 52))
    vt = v.view(B, N, Hkv, 64).permute(0, 2, 3, 1).contiguous()
    o = torch.zeros(B * N, Hq * 64, dtype=OP, device=q.device)
    L.check(L.lib().jat_k_attention(L.ptr(q), L.ptr(k), L.ptr(vt), L.ptr(o), B, N, Hq, Hkv, npad, L.stream_ptr()))
    ref = _attention_ref(qf, kf, vf, B, N, Hq, Hkv)
    assert rel(o, ref) < 6e-3
    assert (o.double() - ref).abs().max() < 2e-2 * float(ref.abs().max())


# ---- per-sample key counts (AttnArgs::lens through jat_k_attention_lens) -----------------------------------------------------
# How Sampler.run(lengths=...) and sample_long run a short chunk in a bucket of longer ones.  attn_fwd_kernel: Nb = min(lens[b], N),
# the key-block count from Nb, the mask only where key0 + KVB > Nb; attn_group_kernel: Nk = min(lens[b], N), the mask only where
# Nk < 128.  name -> (N, Npad, Hq, Hkv, lens, (group, qt, kvb) under the default switches, the lens < N whose stand-alone run takes
# the same route under the default switches).  Heads as few as the head loops allow: the streaming kernel has none (one block per
# q head; (4, 2) keeps the GQA sharing), the group kernel walks the G = Hq / Hkv heads of a KV head in pairs: G = 3 (odd), 1, 2.
# In "stream345" 344 / 321 / 320 / 192 / 65 / 64 / 63 sit on either side of a 64-key block edge; "block23" is the one shape the
# sampler-level lengths tests reach.
_GROUP_LENS = [100, 99, 65, 64, 33, 17, 1]
LENS_BUCKETS = {
    "stream345": (345, 384, 4, 2, [345, 344, 321, 320, 192, 130, 65, 64, 63, 1], (0, 1, 64), [344, 321, 320, 192, 130]),
    "group100_g3": (100, 128, 6, 2, _GROUP_LENS, (1, 1, 64), _GROUP_LENS[1:]),
    "group100_g1": (100, 128, 2, 2, _GROUP_LENS, (1, 1, 64), _GROUP_LENS[1:]),
    "group100_g2": (100, 128, 4, 2, _GROUP_LENS, (1, 1, 64), _GROUP_LENS[1:]),
    "group128": (128, 128, 4, 2, [128, 127, 96], (1, 1, 64), [127, 96]),
    "block23": (23, 64, 4, 2, [23, 13, 1], (0, 1, 64), [13, 1]),
}
DEFAULT_SWITCHES = not any(os.environ.get(k) for k in ("JAT_ATTN_GROUP", "JAT_ATTN_QT", "JAT_ATTN_KVB"))
_lens_cache = {}


def _attn_route(N, npad):
    g, qt, kvb = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    L.check(L.lib().jat_k_attention_route(N, npad, 0, 0, C.byref(g), C.byref(qt), C.byref(kvb)))
    return (g.value, qt.value, kvb.value)


def _to_vt(v, B, N, Hkv, npad):
    """v [B*N, Hkv*64] -> V^T [B, Hkv, 64, npad], zero from N to npad"""
    vt = torch.zeros(B, Hkv, 64, npad, dtype=OP, device=v.device)
    vt[:, :, :, :N] = v.view(B, N, Hkv, 64).permute(0, 2, 3, 1)
    return vt


def _run_attention(q, k, vt, B, N, Hq, Hkv, npad, lens=None):
    """jat_k_attention (lens None) or jat_k_attention_lens into a NaN-filled output"""
    o = torch.full((B * N, Hq * 64), float("nan"), device=q.device).to(OP)
    if lens is None:
        L.check(L.lib().jat_k_attention(L.ptr(q), L.ptr(k), L.ptr(vt), L.ptr(o), B, N, Hq, Hkv, npad, L.stream_ptr()))
    else:
        assert lens.dtype == torch.int32 and lens.numel() == B and int(lens.min()) >= 1
        L.check(L.lib().jat_k_attention_lens(L.ptr(q), L.ptr(k), L.ptr(vt), L.ptr(o), L.ptr(lens), B, N, Hq, Hkv, npad,
                                             L.stream_ptr()))
    torch.cuda.synchronize()
    return o


def _past_lens(k, v, B, N, lens, fill):
    """copies of k and v [B*N, Hkv*64] with the rows at keys >= lens[b] replaced: fill None -> K times 8 (exact in OP) and V = 100,
    so that ONE leaked key takes most of the softmax weight of about half of the query rows (its logit has eight times the
    spread of a real one) and moves them by tens of units; fill = a seed -> other finite values"""
    kp, vp = k.clone().view(B, N, -1), v.clone().view(B, N, -1)
    for b, n in enumerate(lens):
        if n < N:
            if fill is None:
                kp[b, n:] = kp[b, n:] * 8
                vp[b, n:] = 100.0
            else:
                kp[b, n:] = gen(tuple(kp[b, n:].shape), fill + b, 6.0).to(OP)
                vp[b, n:] = (gen(tuple(vp[b, n:].shape), fill + 50 + b, 20.0) - 37.0).to(OP)
    return kp.view(B * N, -1), vp.view(B * N, -1)


def _lens_case(name):
    """Inputs as test_attention draws them (q, k at scale 1.5, v at 1), poisoned past lens[b]; the kernel's output; the fp64 reference.
    Built once per bucket and left unchanged."""
    if name not in _lens_cache:
        N, npad, Hq, Hkv, lens, _, _ = LENS_BUCKETS[name]
        B = len(lens)
        q, k, v = (gen((B * N, h * 64), s, sc).to(OP) for h, s, sc in ((Hq, 40, 1.5), (Hkv, 41, 1.5), (Hkv, 42, 1.0)))
        kp, vp = _past_lens(k, v, B, N, lens, None)
        vt = _to_vt(vp, B, N, Hkv, npad)
        lens_t = torch.tensor(lens, dtype=torch.int32, device=q.device)
        o = _run_attention(q, kp, vt, B, N, Hq, Hkv, npad, lens_t)
        ref = _attention_ref(q, kp, vp, B, N, Hq, Hkv, lens_t)
        assert bool(torch.isfinite(kp).all()) and bool(torch.isfinite(vt).all()) and float(vt[..., N:].abs().max() if npad > N else 0) == 0
        _lens_cache[name] = dict(q=q, k=k, v=v, kp=kp, vp=vp, vt=vt, lens_t=lens_t, o=o, ref=ref)
    return _lens_cache[name]


@pytest.mark.parametrize("name", list(LENS_BUCKETS))
def test_attention_lens_vs_fp64(name):
    """jat_k_attention_lens against the masked fp64 reference, with test_attention's gates (P and the output are rounded to OP:
    rel < 6e-3, max-abs < 2e-2 max|ref|) applied to every sample on its own, over all N query rows (the rows past lens[b] too: the
    next layer reads them), every element finite; a sample with lens[b] = 1 is V's row 0 in every query row, bit for bit (P = 1,
    l = 1).  The leak the poison makes: with the mask of one sample off by a key, that sample's rel is of order 1."""
    N, npad, Hq, Hkv, lens, route, _ = LENS_BUCKETS[name]
    if DEFAULT_SWITCHES:
        assert _attn_route(N, npad) == route
    c = _lens_case(name)
    o, ref = c["o"], c["ref"]
    assert bool(torch.isfinite(o).all())
    for b, n in enumerate(lens):
        ob, rb = o[b * N:(b + 1) * N], ref[b * N:(b + 1) * N]
        r, ma, top = rel(ob, rb), float((ob.double() - rb).abs().max()), float(rb.abs().max())
        print(f"{name} route {_attn_route(N, npad)} lens {n}: rel {r:.3e}, max-abs {ma:.3e} of max|ref| {top:.3e}")
        assert r < 6e-3 and ma < 2e-2 * top, (name, n)
        if n == 1:
            row0 = c["v"].view(len(lens), N, Hkv, 64)[b, 0].repeat_interleave(Hq // Hkv, 0).reshape(1, Hq * 64)
            assert torch.equal(ob, row0.expand(N, -1)), (name, b)


@pytest.mark.parametrize("name", list(LENS_BUCKETS))
def test_attention_lens_full_lengths_are_the_plain_call(name):
    """lens[b] = N everywhere, and lens[b] = N + 7 (values above N act as N): the bits of jat_k_attention on the same buffers."""
    N, npad, Hq, Hkv, lens, _, _ = LENS_BUCKETS[name]
    B = len(lens)
    c = _lens_case(name)
    vt = _to_vt(c["v"], B, N, Hkv, npad)
    plain = _run_attention(c["q"], c["k"], vt, B, N, Hq, Hkv, npad)
    assert bool(torch.isfinite(plain).all())
    for full in (N, N + 7):
        lens_t = torch.full((B,), full, dtype=torch.int32, device=plain.device)
        assert torch.equal(_run_attention(c["q"], c["k"], vt, B, N, Hq, Hkv, npad, lens_t), plain), (name, full)


@pytest.mark.parametrize("name", list(LENS_BUCKETS))
def test_attention_lens_rows_equal_the_stand_alone_run(name):
    """"Same key blocks as a stand-alone run of Nb tokens" (attn_fwd_kernel): the rows < lens[b] of sample b are the bits of
    jat_k_attention on that sample's first lens[b] tokens alone (same Npad, V^T zero beyond lens[b]) — wherever
    jat_k_attention_route gives (N, Npad) and (lens[b], Npad) the same kernel; elsewhere only the fp64 gate applies.  Under the
    default switches the lengths of LENS_BUCKETS' last column must take this branch, so that the condition cannot skip them."""
    N, npad, Hq, Hkv, lens, _, must = LENS_BUCKETS[name]
    c = _lens_case(name)
    here, taken = _attn_route(N, npad), []
    for b, n in enumerate(lens):
        if n >= N or _attn_route(n, npad) != here:
            continue
        rows = slice(b * N, b * N + n)
        vt = _to_vt(c["v"][rows], 1, n, Hkv, npad)
        alone = _run_attention(c["q"][rows], c["k"][rows], vt, 1, n, Hq, Hkv, npad)
        assert torch.equal(c["o"][rows], alone), (name, n)
        taken.append(n)
    print(f"{name} route {here}: bitwise against the stand-alone run at lens {taken}")
    if DEFAULT_SWITCHES:
        assert taken == must, (taken, must)
    assert taken, name           # under every switch setting of tests/test_gpu_widths.py some length keeps the route


@pytest.mark.parametrize("name", ["stream345", "group100_g3"])
def test_attention_lens_ignores_what_lies_past_lens(name):
    """The K rows and V columns at keys >= lens[b] refilled with other finite values: every row of every sample keeps its bits."""
    N, npad, Hq, Hkv, lens, _, _ = LENS_BUCKETS[name]
    B = len(lens)
    c = _lens_case(name)
    kp, vp = _past_lens(c["k"], c["v"], B, N, lens, 900)
    assert not torch.equal(kp, c["kp"]) and not torch.equal(vp, c["vp"])
    again = _run_attention(c["q"], kp, _to_vt(vp, B, N, Hkv, npad), B, N, Hq, Hkv, npad, c["lens_t"])
    assert torch.equal(again, c["o"])


def test_attention_lens_refuses_a_null_lens():
    z = torch.zeros(64, 128, dtype=OP, device=dev())
    assert L.lib().jat_k_attention_lens(L.ptr(z), L.ptr(z), L.ptr(z), L.ptr(z), None, 1, 64, 2, 2, 64, L.stream_ptr()) == L.JAT_E_INVALID


def _rope_pair_rows(w):
    """rows (or bias entries) of q / k heads in the rotate-half pair order of cast_bf16_rope_rows_kernel: inside every head, packed
    row 2i holds source row i and packed row 2i + 1 holds source row i + 32"""
    H = w.shape[0] // 64
    return w.reshape(H, 2, 32, -1).permute(0, 2, 1, 3).reshape(w.shape)


def _pack_group_major(q, k, v, Hkv):
    """[Hkv][5 q heads, the k head, the v head] = 448 rows per KV group, q / k heads pair-interleaved"""
    return torch.cat([torch.cat([_rope_pair_rows(q[g * 320:(g + 1) * 320]), _rope_pair_rows(k[g * 64:(g + 1) * 64]),
                                 v[g * 64:(g + 1) * 64]]) for g in range(Hkv)]).contiguous()


def _qkv_attn_case(M, K, Hkv, np_, a_scale=1.0):
    """Runs jat_k_qkv_attn on weights packed here from plain Wq / Wk / Wv, into a poisoned arena; returns what the checks need."""
    B = M // 128
    A, Af = bf16_bits(gen((M, K), 300 + K, a_scale))
    (Wq, Wqf), (Wk, Wkf), (Wv, Wvf) = (bf16_bits(gen((Hkv * r, K), 301 + i, 1.0 / np.sqrt(K))) for i, r in enumerate((320, 64, 64)))
    Wg = _pack_group_major(Wq, Wk, Wv, Hkv)
    invf = torch.from_numpy(R.rope_inv_freq()).to(A.device)
    assert torch.allclose(invf.double(), 10000.0 ** (-2.0 * torch.arange(32, device=A.device).double() / 64), rtol=1e-6)
    bias = part = rs = None
    bq = bk = bv = None
    if np_:
        bq, bk, bv = gen((Hkv * 320,), 310, 0.3), gen((Hkv * 64,), 311, 0.3), gen((Hkv * 64,), 312, 0.3)
        bias = _pack_group_major(bq, bk, bv, Hkv)
        part = gen((M, np_), 313).abs() * K / np_ + 0.1
        rs = torch.rsqrt(part.double().sum(1) / K + 1e-6).view(B, 128, 1)
    ld = Hkv * 320
    arena = torch.full(((M + 128) * ld,), float("nan"), device=A.device).to(OP)
    out = arena[:M * ld].view(M, ld)

    def launch(a, o, m, p):
        L.check(L.lib().jat_k_qkv_attn(L.ptr(a), L.ptr(Wg), L.ptr(bias), L.ptr(o), m, Hkv, K, L.ptr(invf), L.ptr(p), np_,
                                       L.stream_ptr()))
    launch(A, out, M, part)
    torch.cuda.synchronize()
    assert torch.isnan(arena[M * ld:]).all() and torch.isfinite(out).all()     # the 128 guard rows stay poisoned
    # every sample of the batch equals the same sample run alone, bit for bit
    for b in range(B):
        alone = torch.full((128, ld), float("nan"), device=A.device).to(OP)
        launch(A[b * 128:(b + 1) * 128], alone, 128, part[b * 128:(b + 1) * 128] if np_ else None)
        assert torch.equal(alone, out[b * 128:(b + 1) * 128]), b
    refs = []
    for rnd in (R.identity, R.make_rnd(OP)):
        refs.append(torch.cat([R.qkv_attention_group(
            Af.double().view(B, 128, K), Wqf[g * 320:(g + 1) * 320].double(), Wkf[g * 64:(g + 1) * 64].double(),
            Wvf[g * 64:(g + 1) * 64].double(), rnd, invf.cpu().numpy(),
            *((bq[g * 320:(g + 1) * 320].double(), bk[g * 64:(g + 1) * 64].double(), bv[g * 64:(g + 1) * 64].double(), rs)
              if np_ else ())) for g in range(Hkv)], -1).view(M, ld))
    exact, rounded = refs
    err, e0 = rel(out, exact), rel(rounded, exact)
    ma, ma0 = float((out.double() - exact).abs().max()), float((rounded - exact).abs().max())
    print(f"qkv_attn M={M} K={K} Hkv={Hkv} np={np_}: error {err:.3e} / E0 {e0:.3e} = {err / e0:.3f}, max-abs {ma:.3e} / {ma0:.3e} = "
          f"{ma / ma0:.3f}")
    return err, e0, ma, ma0


@pytest.mark.parametrize("np_", [0, 4, 8, 16])
@pytest.mark.parametrize("Hkv", [4, 1])
@pytest.mark.parametrize("K", [64, 128, 192, 1280])
@pytest.mark.parametrize("M", [128, 256, 7168])
def test_qkv_attn_fused_kernel(M, K, Hkv, np_):
    """jat_k_qkv_attn (q/k/v projection + RoPE + GQA attention of one (sample, KV group) per block) on its own: the group-major,
    pair-interleaved weight is packed HERE from plain Wq / Wk / Wv; 1, 2, 3 and 20 K-tiles; 1, 2 and 56 samples; 4 KV groups and 1;
    without row statistics, and with the folded norms' consumer side (np_ = 4 / 8 / 16 partial sums per row: accumulator rows
    scaled by rsqrt(sum part / K + 1e-6) before the bias, bias in the packed order).
    Reference: tests/forward_ref.py `qkv_attention_group` in fp64 on the same rounded A and W, with rope_inv_freq[i] =
    10000^(-2i/64).  Gate: error against the exact twin (rnd = identity) <= 1.5 E0, E0 = the error of the twin that rounds q, k,
    v, P and the output — relative L2 and max-abs.  Measured (MI355X, bf16): error / E0 0.998 ... 1.005 over the 96 cases and
    the spiky one (E0 3.2e-3 ... 3.4e-3), max-abs ratio 1.000.  The output lies in a
    poisoned arena (128 guard rows stay NaN) and every sample equals its stand-alone run bit for bit."""
    err, e0, ma, ma0 = _qkv_attn_case(M, K, Hkv, np_)
    assert err <= 1.5 * e0 and ma <= 1.5 * ma0


def test_qkv_attn_fused_kernel_spiky_rows():
    """Logits of standard deviation ~9 (A scaled by 3): most query rows are dominated by one or two keys, as in
    test_attention_spiky_rows; same gate."""
    err, e0, ma, ma0 = _qkv_attn_case(256, 128, 4, 16, a_scale=3.0)
    assert err <= 1.5 * e0 and ma <= 1.5 * ma0


def test_qkv_attn_fused_kernel_rejects_unsupported_shapes():
    z = torch.zeros(256, 128, dtype=OP, device=dev())
    w = torch.zeros(448, 128, dtype=OP, device=dev())
    o = torch.zeros(256, 320, dtype=OP, device=dev())
    invf = torch.ones(32, device=dev())
    for M, K in ((100, 128), (128, 96)):     # M must be whole 128-token samples, K whole 64-deep K-tiles
        assert L.lib().jat_k_qkv_attn(L.ptr(z), L.ptr(w), None, L.ptr(o), M, 1, K, L.ptr(invf), None, 0, L.stream_ptr()) != 0


@pytest.mark.parametrize("use_cfg,t", [(True, 0.3), (False, 0.5), (True, 0.9995)])
def test_cfg_euler_step(use_cfg, t):
    """Bit-exact against the reference expression order (infer_test_v3m2.py:161-179) in fp32."""
    B, Cc, T = 2, 8, 37
    scale = 3.0 if use_cfg else 1.0
    xp = gen((2 * B if use_cfg else B, Cc, T), 60)
    z = gen((B, Cc, T), 61)
    z0 = z.clone()
    dt = 0.02
    L.check(L.lib().jat_cfg_euler_step(L.ptr(xp), L.ptr(z), scale, t, dt, B, Cc, T, L.stream_ptr()))
    x = xp[B:] + scale * (xp[:B] - xp[B:]) if use_cfg else xp
    tt = torch.tensor(t, dtype=torch.float32)
    if t < 0.999:
        ref = z0 + (x - z0) / (1 - tt + 1e-5).to(x.device) * torch.tensor(dt, dtype=torch.float32, device=x.device)
    else:
        ref = x
    assert torch.allclose(z, ref, rtol=0, atol=2e-6)
    assert rel(z, ref) < 1e-6


def test_channel_affine_roundtrip():
    B, Cc, T = 2, 32, 50
    x = gen((B, Cc, T), 70)
    mean, std = gen((Cc,), 71), gen((Cc,), 72).abs() + 0.5
    y = torch.empty_like(x)
    L.check(L.lib().jat_channel_affine(L.ptr(x), L.ptr(mean), L.ptr(std), L.ptr(y), B, Cc, T, 0, L.stream_ptr()))
    assert torch.allclose(y, (x - mean.view(1, -1, 1)) / std.view(1, -1, 1), atol=1e-6)
    x2 = torch.empty_like(x)
    L.check(L.lib().jat_channel_affine(L.ptr(y), L.ptr(mean), L.ptr(std), L.ptr(x2), B, Cc, T, 1, L.stream_ptr()))
    assert torch.allclose(x2, x, atol=1e-5)
