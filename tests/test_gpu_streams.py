"""Every stream-taking entry of include/jat_hip.h on a delayed side stream (tests/stream_check.py): the bits of the plain call, and
no synchronisation outside the SYNCHRONISES table.  One case per entry family, at the smallest shapes of the family's own tests
at which it still takes its multi-launch path.  tests/test_streams_table_cpu.py keeps the table complete against the header.

The cases call the entries as users do: through the Python wrappers where one exists and does not itself read a result back,
through ctypes with `L.stream_ptr()` otherwise.  At most two streams exist at a time (the default stream and the case's), no
environment variable is set, no graph is captured here (the sampler's own is the only one) and no process is started."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import jatsr_amd  # noqa: E402
import jatsr_amd._lib as L  # noqa: E402
import jatsr_amd.sampler  # noqa: E402,F401
import jatsr_amd.recipe as recipe  # noqa: E402
from jatsr_amd.model import JaT_AudioSR_V2, JaT_AudioSR_V3  # noqa: E402
from stream_check import Case, check_case, run_on_side_stream  # noqa: E402

OP = torch.float16 if L.OPERAND_DTYPE == "fp16" else torch.bfloat16

# Entries that wait for the caller's stream (or the device) before they return, from csrc/: name -> where and why.
SYNCHRONISES = {
    "jat_model_load_weights": "hipStreamSynchronize after the pack: the caller's fp32 tensors are only borrowed for the call",
    "jat_sampler_create": "takes no stream: builds its tables on a private one, waits for the device, then captures the graph",
    "jat_sampler_create_ex": "as jat_sampler_create",
    "jat_sampler_set_lengths": "hipStreamSynchronize: the two tables are copied from host memory of the caller",
    "jat_trainer_create": "hipStreamSynchronize after the first pack and the upload of the copy-job and twiddle tables",
    "jat_k_latent_loss": "unit-test entry: uploads its twiddle table from a host vector and waits before that vector goes",
    "jat_k_latent_loss_ex": "as jat_k_latent_loss (the trainer keeps its table from creation and does not wait)",
    "jat_dac_decoder_create": "synchronous hipMemcpy of every re-laid-out weight, after a hipStreamSynchronize of the caller's stream",
    "jat_dac_encoder_create": "as jat_dac_decoder_create",
    "jat_resampler_create": "hipStreamSynchronize after the tap table's upload from a host vector",
    "jat_audio_metrics_create": "hipStreamSynchronize after the upload of window, twiddles and filterbank from a host vector",
}

# Stream-taking entries without a case of their own, each with the reason: none today.
EXEMPT = {}

CASES = {}


def case(name, covers):
    def deco(fn):
        assert name not in CASES
        CASES[name] = (tuple(covers), fn)
        return fn
    return deco


def covered_entries():
    return sorted({e for covers, _ in CASES.values() for e in covers})


# ---- shared pieces ---------------------------------------------------------------------------------------------------------
def gen(shape, seed, scale=1.0, offset=0.0, dtype=torch.float32):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale + offset).to("cuda").to(dtype)


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def fresh_model(norm="rms", salt=0, **kw):
    cfg = recipe.CONFIGS["micro"]
    m = (JaT_AudioSR_V3 if norm == "rms" else JaT_AudioSR_V2)(**cfg, **kw)
    sd = {k: torch.from_numpy(v) for k, v in recipe.make_state_dict(cfg, norm, salt).items()}
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all(".rope." in k for k in missing)
    return m.to("cuda").eval()


_shared = {}


def micro():
    """the micro model every model, sampler and chunk case shares (its handle's cached workspace is scrubbed by the harness)"""
    if "micro" not in _shared:
        L.require_gpu()
        _shared["micro"] = fresh_model()
    return _shared["micro"]


def ck(rc):
    L.check(rc)


def vp(t, offset_elems=0):
    return C.c_void_p(t.data_ptr() + offset_elems * t.element_size()) if t is not None else None


def work_bytes(n):
    return torch.empty(int(n) + 16, dtype=torch.uint8, device="cuda")


# ---- the detector must detect ----------------------------------------------------------------------------------------------
def _stand_in(wrong_stream):
    """a two-op "entry" in torch: y = (2 x + 1) * w.  wrong_stream: the second op is issued on the default stream."""
    def call(_, i, o):
        tmp = i["x"] * 2 + 1
        if wrong_stream:
            with torch.cuda.stream(torch.cuda.default_stream()):
                o["y"].copy_(tmp * i["w"])
        else:
            o["y"].copy_(tmp * i["w"])
    x, w = gen((257, 129), 1), gen((257, 129), 2)
    return Case({"x": x, "w": w}, call, outputs={"y": x})


def test_a_second_op_on_the_default_stream_is_detected():
    r = run_on_side_stream(_stand_in(True))
    print(r)
    assert r.pending, "the delay had ended before the stand-in returned: the detector proves nothing at this delay"
    assert r.mismatched == ["out:y"], r


def test_both_ops_on_the_current_stream_pass():
    check_case(_stand_in(False), "stand-in")


# ---- model -----------------------------------------------------------------------------------------------------------------
@case("load_state_dict", ["jat_model_load_weights", "jat_forward"])
def _load_state_dict():
    cfg = recipe.CONFIGS["micro"]
    sd = {k: cuda(v) for k, v in recipe.make_state_dict(cfg, "rms", 7).items()}
    x_t, x_c = recipe.make_latents(2, 32, 24, salt=100)
    inputs = dict(sd, x_t=cuda(x_t), t=cuda(np.array([0.02, 0.98], np.float32)), x_cond=cuda(x_c))

    def state(live, outs):
        return fresh_model(salt=3)              # packed once from OTHER weights

    def call(m, i, o):
        m.load_state_dict({k: i[k] for k in sd}, strict=False)       # copies on the current stream; the next forward re-packs
        return {"y": m(i["x_t"], i["t"], i["x_cond"])}
    return Case(inputs, call, state=state)


def _forward(T):
    x_t, x_c = recipe.make_latents(2, 32, T, salt=100)
    m = micro()
    return Case({"x_t": cuda(x_t), "t": cuda(np.array([0.02, 0.98], np.float32)), "x_cond": cuda(x_c)},
                lambda _, i, o: {"y": m(i["x_t"], i["t"], i["x_cond"])})


@case("forward_T24", ["jat_forward"])
def _forward_24():
    return _forward(24)


@case("forward_T22_pad", ["jat_forward"])
def _forward_22():
    return _forward(22)


@case("block_forward", ["jat_block_forward"])
def _block_forward():
    m = micro()
    return Case({"x": cuda(recipe.gaussian("blk_x", (2, 10, 256), 1)), "t_emb": cuda(recipe.gaussian("blk_t", (2, 256), 2))},
                lambda _, i, o: {"y": m.blocks[1](i["x"], i["t_emb"])})


@case("attn_forward", ["jat_attn_forward"])
def _attn_forward():
    m = micro()
    return Case({"x": cuda(recipe.gaussian("attn_x", (2, 37, 256), 3))}, lambda _, i, o: {"y": m.blocks[1].attn(i["x"])})


@case("time_embed", ["jat_time_embed"])
def _time_embed():
    m = micro()
    return Case({"t": cuda(np.array([0.0, 0.02, 0.5, 0.98, 1.0], np.float32))}, lambda _, i, o: {"y": m.time_embed(i["t"])})


# ---- sampler ---------------------------------------------------------------------------------------------------------------
def _sampler_inputs(lengths=None):
    lr, z0 = recipe.gaussian("len_lr", (3, 32, 92), 50), recipe.gaussian("len_z0", (3, 32, 92), 150)
    for b, n in enumerate(lengths or []):
        lr[b, :, n:] = 0
        z0[b, :, n:] = 0
    return {"lr": cuda(lr), "z0": cuda(z0)}


def _sampler(use_graph, lengths=None, solver="euler", steps=3):
    m = micro()
    return Case(_sampler_inputs(lengths),
                lambda s, i, o: {"z": s.run(i["lr"], i["z0"], use_graph=use_graph, lengths=lengths)},
                state=lambda live, outs: jatsr_amd.sampler.Sampler(m, 3, 92, steps, 2.5, solver=solver))


@case("sampler_graph", ["jat_sampler_run"])
def _sampler_graph():
    return _sampler(True)


@case("sampler_eager", ["jat_sampler_run"])
def _sampler_eager():
    return _sampler(False)


@case("sampler_graph_lengths", ["jat_sampler_set_lengths", "jat_sampler_run"])
def _sampler_graph_lengths():
    return _sampler(True, [92, 37, 92])


@case("sampler_eager_lengths", ["jat_sampler_set_lengths", "jat_sampler_run"])
def _sampler_eager_lengths():
    return _sampler(False, [92, 37, 92])


@case("sampler_heun_graph", ["jat_sampler_run"])
def _sampler_heun_graph():
    return _sampler(True, solver="heun", steps=2)


@case("sampler_heun_eager", ["jat_sampler_run"])
def _sampler_heun_eager():
    return _sampler(False, solver="heun", steps=2)


@case("sampler_created_on_the_stream", ["jat_sampler_create_ex", "jat_sampler_run"])
def _sampler_created():
    m = micro()
    keep = []           # destroyed after the comparison, not while its run is queued

    def call(_, i, o):
        keep.append(jatsr_amd.sampler.Sampler(m, 3, 92, 3, 2.5))
        return {"z": keep[-1].run(i["lr"], i["z0"])}
    return Case(_sampler_inputs(), call)


# ---- chunk pieces ----------------------------------------------------------------------------------------------------------
@case("cfg_euler_step", ["jat_cfg_euler_step"])
def _cfg_euler_step():
    B, Cc, T = 2, 32, 37
    return Case({"xp": gen((2 * B, Cc, T), 10), "z": gen((B, Cc, T), 11)},
                lambda _, i, o: ck(L.lib().jat_cfg_euler_step(vp(i["xp"]), vp(i["z"]), 2.5, 0.3, 0.1, B, Cc, T, L.stream_ptr())))


@case("cfg_stage_step", ["jat_cfg_stage_step"])
def _cfg_stage_step():
    B, Cc, T = 2, 32, 37

    def call(_, i, o):
        fn = L.lib().jat_cfg_stage_step
        ck(fn(vp(i["xp"]), vp(i["z"]), vp(i["zb"]), 2.5, 0.3, 0.0, 0.0, 0.1, 1, B, Cc, T, L.stream_ptr()))     # save: z_base = z
        ck(fn(vp(i["xp2"]), vp(i["z"]), vp(i["zb"]), 2.5, 0.4, 0.5, 0.5, 0.05, 0, B, Cc, T, L.stream_ptr()))
    return Case({"xp": gen((2 * B, Cc, T), 12), "xp2": gen((2 * B, Cc, T), 13), "z": gen((B, Cc, T), 14), "zb": gen((B, Cc, T), 15)},
                call)


@case("channel_affine", ["jat_channel_affine"])
def _channel_affine():
    def call(_, i, o):
        y = jatsr_amd.sampler.channel_affine(i["x"], i["mean"], i["std"])
        return {"y": y, "back": jatsr_amd.sampler.channel_affine(y, i["mean"], i["std"], inverse=True)}
    return Case({"x": gen((2, 32, 37), 16), "mean": gen((32,), 17, 0.1), "std": gen((32,), 18).abs() + 0.5}, call)


@case("crossfade_pair", ["jat_crossfade_pair"])
def _crossfade_pair():
    return Case({"a": gen((1, 32, 40), 19), "b": gen((1, 32, 40), 20), "c": gen((1, 32, 36), 21)},
                lambda _, i, o: {"y": jatsr_amd.sampler.crossfade_chunks([i["a"], i["b"], i["c"]], 8)})


@case("sample_long", ["jat_channel_affine", "jat_sampler_run", "jat_crossfade_pair"])
def _sample_long():
    m = micro()
    Cc, total, chunk, ov = 32, 100, 40, 8
    plan = jatsr_amd.chunk_plan(total, chunk, ov)
    inputs = {"lr": cuda(recipe.gaussian("long_lr", (Cc, total), 1) * 2 + 0.3), "mean": cuda(recipe.gaussian("mean", (Cc,), 2) * 0.1),
              "std": cuda(np.abs(recipe.gaussian("std", (Cc,), 3)) + 0.5)}
    for n, (a, b) in enumerate(plan):
        inputs[f"noise{n}"] = cuda(recipe.gaussian("noise", (1, Cc, b - a), n))

    def call(_, i, o):
        return {"y": jatsr_amd.sample_long(m, i["lr"], i["mean"], i["std"], i["mean"], i["std"], num_steps=4, cfg_scale=2.0,
                                           chunk_frames=chunk, overlap_frames=ov, noise=[i[f"noise{n}"] for n in range(len(plan))])}
    return Case(inputs, call)


# ---- trainer ---------------------------------------------------------------------------------------------------------------
def _optim(tr, step, k=1):
    """jat_trainer_optim as Trainer.optimizer_step calls it, without that method's read-back of loss and norm"""
    ck(L.lib().jat_trainer_optim(tr.ptr, 1e-3, 0.9, 0.999, 1e-8, 0.1, 1.0, float(tr.scaler.scale * k), step,
                                 C.c_void_p(tr._scal.data_ptr() + 4), L.stream_ptr()))
    tr._micro = 0


def _trainer_inputs(B=2, T=24):
    i = {k: cuda(recipe.gaussian("stream_" + k, (B, 32, T), 300 + n)) for n, k in enumerate(("hr", "lr", "noise", "cn", "hr2", "lr2"))}
    i["t"] = cuda(np.array([0.3, 0.8], np.float32))
    i["mask"] = torch.tensor([False, True], device="cuda")
    return i, {"mask": torch.tensor([True, False], device="cuda")}


def _make_trainer(**kw):
    from jatsr_amd.train import Trainer
    rich = bool(kw.get("latent_loss_weight"))
    m = fresh_model(dropout=0.1 if rich else 0.0, drop_path_rate=0.05 if rich else 0.0).train()
    tr = Trainer(m, batch_size=2, frames=24, lr=1e-3, use_grad_scaler=False, **kw)
    if L.OPERAND_DTYPE == "fp16":
        tr.scaler.scale = 4096.0
    return tr


def _trainer_step(**kw):
    """prepare, fwd_bwd, optim, loss_terms, swap_ema (twice), repack and a second fwd_bwd on the re-packed weights; gradients,
    parameters, moments and the average are copied (on the case's stream) after each call"""
    inputs, decoys = _trainer_inputs()

    def call(tr, i, o):
        r = {}
        z_t, t, cond = tr.prepare(i["hr"], i["lr"], noise=i["noise"], cond_noise=i["cn"], cfg_mask=i["mask"], t=i["t"])
        r["z_t"], r["cond"] = z_t, cond
        t0 = time.perf_counter()
        r["pred"] = tr.forward_backward(z_t, t, cond, i["hr"], want_pred=True, mask_seed=1234, cond_clean=i["lr"])
        print(f"forward_backward alone: host {(time.perf_counter() - t0) * 1e3:.3f} ms")
        r["grads"], r["loss"] = tr.grads.clone(), tr._scal.clone()
        if tr.loss_config.has_latent:
            r["terms"] = torch.empty(6, device="cuda")
            ck(L.lib().jat_trainer_loss_terms(tr.ptr, vp(r["terms"]), L.stream_ptr()))
        _optim(tr, 1)
        r["params"], r["m"], r["v"], r["norm"] = tr.params.clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone(), tr._scal.clone()
        if tr.ema is not None:
            r["ema"] = tr.ema.clone()
            ck(L.lib().jat_trainer_swap_ema(tr.ptr, L.stream_ptr()))
            r["params_swapped"], r["ema_swapped"] = tr.params.clone(), tr.ema.clone()
            r["pred_on_ema"] = tr.model(i["hr"], i["t"], i["lr"])
            ck(L.lib().jat_trainer_swap_ema(tr.ptr, L.stream_ptr()))
        tr.params.mul_(0.5)                                               # the caller overwrites parameters, then re-packs
        ck(L.lib().jat_trainer_repack(tr.ptr, L.stream_ptr()))
        r["pred2"] = tr.forward_backward(z_t, t, cond, i["hr"], want_pred=True, mask_seed=99, cond_clean=i["lr"])
        r["grads2"], r["params2"] = tr.grads.clone(), tr.params.clone()
        return r
    return Case(inputs, call, decoys=decoys, state=lambda live, outs: _make_trainer(**kw))


TRAINER_ENTRIES = ["jat_trainer_prepare", "jat_trainer_fwd_bwd", "jat_trainer_optim", "jat_trainer_repack"]


@case("trainer_step", TRAINER_ENTRIES)
def _trainer_plain():
    return _trainer_step()


@case("trainer_step_latent_ema_dropout", TRAINER_ENTRIES + ["jat_trainer_loss_terms", "jat_trainer_swap_ema", "jat_forward"])
def _trainer_rich():
    return _trainer_step(latent_loss_weight=0.3, ema_decay=0.9)


@case("trainer_grad_accum", ["jat_trainer_prepare", "jat_trainer_fwd_bwd_ex", "jat_trainer_optim"])
def _trainer_accum():
    """two micro-batches: the accumulating call reads the gradients the first call's second stream wrote"""
    inputs, decoys = _trainer_inputs()

    def call(tr, i, o):
        r = {}
        for j, (hr, lr) in enumerate((("hr", "lr"), ("hr2", "lr2"))):
            z_t, t, cond = tr.prepare(i[hr], i[lr], noise=i["noise"], cond_noise=i["cn"], cfg_mask=i["mask"], t=i["t"])
            tr.forward_backward(z_t, t, cond, i[hr], mask_seed=5 + j, cond_clean=i[lr])
            r[f"grads{j}"], r[f"loss{j}"] = tr.grads.clone(), tr._scal.clone()
        _optim(tr, 1, k=2)
        r["params"], r["m"], r["v"] = tr.params.clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone()
        return r
    return Case(inputs, call, decoys=decoys, state=lambda live, outs: _make_trainer(grad_accum_steps=2))


@case("trainer_created_on_the_stream", ["jat_trainer_create", "jat_trainer_prepare", "jat_trainer_fwd_bwd"])
def _trainer_created():
    inputs, decoys = _trainer_inputs()
    keep = []

    def call(_, i, o):
        tr = _make_trainer()
        keep.append(tr)
        z_t, t, cond = tr.prepare(i["hr"], i["lr"], noise=i["noise"], cond_noise=i["cn"], cfg_mask=i["mask"], t=i["t"])
        tr.forward_backward(z_t, t, cond, i["hr"], mask_seed=1234, cond_clean=i["lr"])
        return {"grads": tr.grads.clone(), "loss": tr._scal.clone()}
    return Case(inputs, call, decoys=decoys)


# ---- jat_k_* ---------------------------------------------------------------------------------------------------------------
@case("k_cast_bf16", ["jat_k_cast_bf16"])
def _k_cast():
    x = gen((3, 1001), 1)
    return Case({"x": x}, lambda _, i, o: ck(L.lib().jat_k_cast_bf16(vp(i["x"]), vp(o["y"]), x.numel(), L.stream_ptr())),
                outputs={"y": x.to(OP)})


@case("k_norm_modulate", ["jat_k_norm_modulate"])
def _k_norm_modulate():
    M, D, ntok = 131, 256, 50
    B = (M + ntok - 1) // ntok
    inputs = {"x": gen((M, D), 2, 3.0, 0.5), "w": 1 + 0.2 * gen((D,), 3), "mod": gen((B, 2 * D), 4, 0.3)}

    def call(_, i, o):
        ck(L.lib().jat_k_norm_modulate(vp(i["x"]), vp(i["w"]), vp(i["mod"]), vp(i["mod"], D), 2 * D, vp(o["y"]), M, D, ntok, 0,
                                       L.stream_ptr()))
    return Case(inputs, call, outputs={"y": torch.empty(M, D, dtype=OP, device="cuda")})


@case("k_gemm", ["jat_k_gemm"])
def _k_gemm():
    M, N, K, ntok = 300, 256, 128, 23
    B = (M + ntok - 1) // ntok
    inputs = {"A": gen((M, K), 10, dtype=OP), "W": gen((N, K), 20, K ** -0.5, dtype=OP), "bias": gen((N,), 30, 0.1),
              "gate": gen((B, N), 31, 0.5), "out": gen((M, N), 32)}        # epilogue 3 adds into `out`

    def call(_, i, o):
        ck(L.lib().jat_k_gemm(vp(i["A"]), vp(i["W"]), vp(i["bias"]), vp(i["out"]), M, N, K, 3, vp(i["gate"]), N, ntok, 20,
                              L.stream_ptr()))
    return Case(inputs, call)


@case("k_gemm_fold", ["jat_k_gemm_fold"])
def _k_gemm_fold():
    M, N, K, ntok, variant = 300, 1280, 256, 128, 20
    B = (M + ntok - 1) // ntok
    wn = L.lib().jat_k_gemm_wave_n(variant)
    x0 = gen((M, N), 204, 2.0)
    hi = x0.to(OP)
    inputs = {"A": gen((M, K), 200, dtype=OP), "W": gen((N, K), 201, K ** -0.5, dtype=OP), "bias": gen((N,), 202, 0.1),
              "gate": gen((B, N), 203, 0.5), "hi": hi, "lo": (x0 - hi.float()).to(OP)}

    def call(_, i, o):
        ck(L.lib().jat_k_gemm_fold(vp(i["A"]), vp(i["W"]), vp(i["bias"]), None, M, N, K, 3, vp(i["gate"]), N, ntok, vp(i["hi"]),
                                   vp(i["lo"]), vp(o["part"]), None, 0, variant, L.stream_ptr()))
    return Case(inputs, call, outputs={"part": torch.empty(M, N // wn, device="cuda")})


@case("k_gemm_splitk", ["jat_k_gemm_splitk"])
def _k_gemm_splitk():
    M, N, K, ks = 200, 256, 512, 2
    return Case({"A": gen((M, K), 260, dtype=OP), "W": gen((N, K), 261, K ** -0.5, dtype=OP)},
                lambda _, i, o: ck(L.lib().jat_k_gemm_splitk(vp(i["A"]), vp(i["W"]), vp(o["parts"]), M, N, K, ks, 20, L.stream_ptr())),
                outputs={"parts": torch.empty(ks, M, N, device="cuda")})


@case("k_weight_grad_ex", ["jat_k_weight_grad_ex", "jat_k_weight_grad"])
def _k_weight_grad():
    tokens, out, in_, ks = 300, 128, 256, 3
    need = 256 + ks * out * in_ * 4 + 32 * out * 4
    inputs = {"dY": gen((tokens, out), 70, dtype=OP), "X": gen((tokens, in_), 71, dtype=OP), "dW": gen((out, in_), 72),
              "db": gen((out,), 73)}

    def call(_, i, o):
        w = work_bytes(need)
        ck(L.lib().jat_k_weight_grad(vp(i["dY"]), vp(i["X"]), vp(o["dW0"]), vp(o["db0"]), tokens, out, in_, ks, vp(w), need,
                                     L.stream_ptr()))
        ck(L.lib().jat_k_weight_grad_ex(vp(i["dY"]), vp(i["X"]), vp(i["dW"]), vp(i["db"]), tokens, out, in_, ks, vp(w), need, 1,
                                        L.stream_ptr()))
    return Case(inputs, call, outputs={"dW0": inputs["dW"], "db0": inputs["db"]})


def _to_patch(z, ntok):
    B, Cc, _ = z.shape
    return z.view(B, Cc, ntok, 4).permute(0, 2, 1, 3).reshape(B * ntok, Cc * 4).contiguous()


def _k_gemm_cfg(stage):
    """the sampler's step tail on caller buffers, un-fused (three launches) and fused (one), each on buffers of its own"""
    M, N, K, ntok, variant = 224, 128, 256, 16, 20
    Mh, B, Cc, T = M // 2, M // 2 // ntok, N // 4, ntok * 4
    z, zb = gen((B, Cc, T), 273), gen((B, Cc, T), 274)
    inputs = {"A": gen((M, K), 270, dtype=OP), "W": gen((N, K), 271, K ** -0.5, dtype=OP), "bias": gen((N,), 272, 0.1),
              "z": z, "zp": _to_patch(z, ntok), "zb": zb, "zbp": _to_patch(zb, ntok)}

    def call(_, i, o):
        for fused, zk, zbk, ap in ((0, "z", "zb", "a_patch"), (1, "zp", "zbp", "a_patch_fused")):
            if stage:
                ck(L.lib().jat_k_gemm_cfg_stage(vp(i["A"]), vp(i["W"]), vp(i["bias"]), M, N, K, ntok, None, 0, vp(i[zk]), vp(i[zbk]),
                                                vp(o[ap]), vp(o["xpred"]), None, 3.0, 0.5, 0.5, 0.5, 0.01, 0, variant, fused,
                                                L.stream_ptr()))
            else:
                ck(L.lib().jat_k_gemm_cfg_euler(vp(i["A"]), vp(i["W"]), vp(i["bias"]), M, N, K, ntok, None, 0, vp(i[zk]), vp(o[ap]),
                                                vp(o["xpred"]), None, 3.0, 0.5, 0.02, variant, fused, L.stream_ptr()))
    patch = torch.empty(Mh, N, dtype=torch.int16, device="cuda")
    return Case(inputs, call, outputs={"a_patch": patch, "a_patch_fused": patch, "xpred": torch.empty(2 * B, Cc, T, device="cuda")})


@case("k_gemm_cfg_euler", ["jat_k_gemm_cfg_euler"])
def _k_gemm_cfg_euler():
    return _k_gemm_cfg(False)


@case("k_gemm_cfg_stage", ["jat_k_gemm_cfg_stage"])
def _k_gemm_cfg_stage():
    return _k_gemm_cfg(True)


@case("k_qkv_attn", ["jat_k_qkv_attn"])
def _k_qkv_attn():
    """any weight values do: the case compares bits, the packing is test_gpu_kernels.py's business"""
    M, K, Hkv, np_ = 256, 128, 2, 8
    inputs = {"A": gen((M, K), 300, dtype=OP), "Wg": gen((Hkv * 448, K), 301, K ** -0.5, dtype=OP), "bias": gen((Hkv * 448,), 302, 0.3),
              "invf": (10000.0 ** (-2.0 * torch.arange(32, dtype=torch.float64) / 64)).float().cuda(),
              "part": gen((M, np_), 303).abs() * K / np_ + 0.1}

    def call(_, i, o):
        ck(L.lib().jat_k_qkv_attn(vp(i["A"]), vp(i["Wg"]), vp(i["bias"]), vp(o["out"]), M, Hkv, K, vp(i["invf"]), vp(i["part"]), np_,
                                  L.stream_ptr()))
    return Case(inputs, call, outputs={"out": torch.empty(M, Hkv * 320, dtype=OP, device="cuda")})


def _attn_inputs(B, N, Hq, Hkv, seed):
    npad = (N + 63) // 64 * 64
    v = gen((B, Hkv, N, 64), seed + 2, dtype=OP)
    vt = torch.zeros(B, Hkv, 64, npad, dtype=OP, device="cuda")
    vt[..., :N] = v.transpose(-1, -2)
    return {"q": gen((B * N, Hq * 64), seed, dtype=OP), "k": gen((B * N, Hkv * 64), seed + 1, dtype=OP), "vt": vt}, npad


@case("k_attention", ["jat_k_attention"])
def _k_attention():
    B, N, Hq, Hkv = 2, 130, 4, 2          # more than one key block
    inputs, npad = _attn_inputs(B, N, Hq, Hkv, 40)

    def call(_, i, o):
        ck(L.lib().jat_k_attention(vp(i["q"]), vp(i["k"]), vp(i["vt"]), vp(o["o"]), B, N, Hq, Hkv, npad, L.stream_ptr()))
    return Case(inputs, call, outputs={"o": inputs["q"]})


@case("k_attention_lens", ["jat_k_attention_lens"])
def _k_attention_lens():
    """a short second sample; the decoy lengths are in range (1 ... N) and differ from the true ones in both samples"""
    B, N, Hq, Hkv = 2, 130, 4, 2          # three key blocks, the short sample ends in the second
    inputs, npad = _attn_inputs(B, N, Hq, Hkv, 45)
    inputs["lens"] = torch.tensor([N, 70], dtype=torch.int32, device="cuda")
    decoys = {"lens": torch.tensor([3, N - 1], dtype=torch.int32, device="cuda")}

    def call(_, i, o):
        ck(L.lib().jat_k_attention_lens(vp(i["q"]), vp(i["k"]), vp(i["vt"]), vp(o["o"]), vp(i["lens"]), B, N, Hq, Hkv, npad,
                                        L.stream_ptr()))
    return Case(inputs, call, outputs={"o": inputs["q"]}, decoys=decoys)


def _k_attention_train(split):
    B, N, Hq, Hkv, p, seed, site = 2, 130, 4, 2, 0.1, 0x1234567, 3
    inputs, npad = _attn_inputs(B, N, Hq, Hkv, 50)
    inv = 1.0 / torch.pow(10000.0, torch.arange(32, dtype=torch.float32) * 2 / 64)
    a = torch.arange(2048, dtype=torch.float32)[:, None] * inv[None, :]
    inputs.update(dout=gen((B * N, Hq * 64), 53, dtype=OP), cos=torch.cos(a).cuda().contiguous(), sin=torch.sin(a).cuda().contiguous())
    rows = B * Hq * N
    need = (rows * 4 + 255) // 256 * 256 + (rows * 128 * 4 if split else 0)

    def call(_, i, o):
        ck(L.lib().jat_k_attention_train(vp(i["q"]), vp(i["k"]), vp(i["vt"]), vp(o["o"]), vp(o["lse"]), B, N, Hq, Hkv, npad, seed,
                                         site, p, L.stream_ptr()))
        w = work_bytes(need)
        ck(L.lib().jat_k_attention_bwd(vp(i["q"]), vp(i["k"]), vp(i["vt"]), vp(o["o"]), vp(i["dout"]), vp(o["lse"]), vp(o["dqkv"]),
                                       vp(i["cos"]), vp(i["sin"]), B, N, Hq, Hkv, npad, seed, site, p, int(split), vp(w), need,
                                       L.stream_ptr()))
    return Case(inputs, call, outputs={"o": inputs["q"], "lse": torch.empty(B, Hq, N, device="cuda"),
                                       "dqkv": torch.empty(B * N, (Hq + 2 * Hkv) * 64, dtype=OP, device="cuda")})


@case("k_attention_train_bwd", ["jat_k_attention_train", "jat_k_attention_bwd"])
def _k_attention_train_one():
    return _k_attention_train(False)


@case("k_attention_train_bwd_split_heads", ["jat_k_attention_train", "jat_k_attention_bwd"])
def _k_attention_train_split():
    return _k_attention_train(True)


def _k_latent_loss(T, kind):
    import loss_path_cases as P
    k, a, b, lds = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
    ck(L.lib().jat_k_latent_loss_plan(T, C.byref(k), C.byref(a), C.byref(b), C.byref(lds)))
    assert k.value == kind, (T, k.value)
    pred, target, lr = (cuda(x[0]) for x in P.make_inputs(T, P.SALT[T]))
    rows = pred.shape[0]
    need = (T * 8 + 255) // 256 * 256 + rows * 32
    args = [P.WEIGHTS[n] for n in ("latent_weight", "freq_weight", "ms_weight", "consistency_weight")] + \
           [P.CUTS[n] for n in ("low_freq_phase_ratio", "strict_cutoff", "soft_cutoff")]

    def call(_, i, o):
        w = work_bytes(need)
        ck(L.lib().jat_k_latent_loss_ex(vp(i["pred"]), vp(i["target"]), vp(i["lr"]), vp(o["dpred"]), vp(o["out6"]), rows, T,
                                        1e-6, 1.0, *args, 1.0, vp(w), need, L.stream_ptr()))
        ck(L.lib().jat_k_latent_loss(vp(i["pred"]), vp(i["target"]), vp(i["lr"]), vp(o["dpred0"]), vp(o["out60"]), rows, T,
                                     *args, 1.0, vp(w), need, L.stream_ptr()))
    return Case({"pred": pred, "target": target, "lr": lr}, call,
                outputs={"dpred": pred, "out6": torch.empty(6, device="cuda"), "dpred0": pred, "out60": torch.empty(6, device="cuda")})


@case("k_latent_loss_direct", ["jat_k_latent_loss_ex", "jat_k_latent_loss"])
def _k_latent_loss_direct():
    return _k_latent_loss(23, 1)


@case("k_latent_loss_fft", ["jat_k_latent_loss_ex", "jat_k_latent_loss"])
def _k_latent_loss_fft():
    return _k_latent_loss(35, 2)


@case("k_recon_loss", ["jat_k_recon_loss"])
def _k_recon_loss():
    n = 2 * 32 * 1001

    def call(_, i, o):
        w = work_bytes(4104)
        ck(L.lib().jat_k_recon_loss(vp(i["pred"]), vp(i["target"]), vp(o["dpred"]), vp(o["loss"]), n, 1e-6, 2.0, vp(w), 4104,
                                    L.stream_ptr()))
    return Case({"pred": gen((n,), 80), "target": gen((n,), 81)}, call,
                outputs={"dpred": torch.empty(n, device="cuda"), "loss": torch.empty(1, device="cuda")})


@case("k_norm_bwd", ["jat_k_norm_bwd"])
def _k_norm_bwd():
    B, D, ntok = 2, 256, 37
    M = B * ntok
    need = (B * ((ntok + 15) // 16) * 3 * D + B * D) * 4
    inputs = {"x": gen((M, D), 30, 2.0, 0.3), "dy": gen((M, D), 31, 1.0, 0.3, dtype=OP), "w": 1 + 0.2 * gen((D,), 32),
              "mod": gen((B, 6 * D), 33, 0.3), "dx": gen((M, D), 34)}            # accumulate: dx += dL/dx

    def call(_, i, o):
        w = work_bytes(need)
        ck(L.lib().jat_k_norm_bwd(vp(i["x"]), vp(i["dy"]), vp(i["w"]), vp(i["mod"], 4 * D), 6 * D, vp(i["dx"]), 1, vp(o["dmod"], 3 * D),
                                  vp(o["dmod"], 4 * D), 6 * D, vp(o["dw"]), B, D, ntok, 0, vp(w), need, L.stream_ptr()))
    return Case(inputs, call, outputs={"dmod": torch.empty(B, 6 * D, device="cuda"), "dw": torch.empty(D, device="cuda")})


@case("k_gate_bwd_and_resid_gate", ["jat_k_gate_bwd", "jat_k_resid_gate"])
def _k_gate():
    B, D, ntok, seed = 2, 256, 37, 0x1234567
    M = B * ntok
    need = B * ((ntok + 15) // 16) * D * 4
    inputs = {"gate": gen((B, 6 * D), 20, 0.5), "y": gen((M, D), 21, dtype=OP), "dx": gen((M, D), 22), "x_in": gen((M, D), 23)}

    def call(_, i, o):
        w = work_bytes(need)
        ck(L.lib().jat_k_resid_gate(vp(i["x_in"]), vp(i["y"]), vp(i["gate"], 5 * D), 6 * D, vp(o["x_out"]), M, D, ntok, seed, 14, 0.2,
                                    13, 0.1, L.stream_ptr()))
        ck(L.lib().jat_k_gate_bwd(vp(i["dx"]), vp(i["y"]), vp(i["gate"], 5 * D), 6 * D, vp(o["dy"]), vp(o["dgate"], 5 * D), 6 * D, B, D,
                                  ntok, seed, 14, 0.2, 13, 0.1, vp(w), need, L.stream_ptr()))
    return Case(inputs, call, outputs={"x_out": inputs["x_in"], "dy": inputs["y"], "dgate": torch.empty(B, 6 * D, device="cuda")})


@case("k_gelu_and_gelu_bwd", ["jat_k_gelu", "jat_k_gelu_bwd"])
def _k_gelu():
    n, seed, site, p = 8 * 1001, 0x1234567, 42, 0.1

    def call(_, i, o):
        ck(L.lib().jat_k_gelu(vp(i["x"]), vp(o["y"]), n, seed, site, p, L.stream_ptr()))
        ck(L.lib().jat_k_gelu_bwd(vp(i["x"]), vp(i["d"]), n, seed, site, p, L.stream_ptr()))
    x = gen((n,), 1, 2.0, dtype=OP)
    return Case({"x": x, "d": gen((n,), 2, dtype=OP)}, call, outputs={"y": x})


def _adamw_inputs(n):
    return {"p": gen((n,), 90), "g": gen((n,), 91, 0.01), "m": gen((n,), 92, 0.01), "v": gen((n,), 93, 0.01).abs()}


@case("k_adamw", ["jat_k_adamw"])
def _k_adamw():
    n = 4 * 2503

    def call(_, i, o):
        w = work_bytes(4104)
        ck(L.lib().jat_k_adamw(vp(i["p"]), vp(i["g"]), vp(i["m"]), vp(i["v"]), n, 1e-3, 0.9, 0.999, 1e-8, 0.1, 1.0, 2.0, 3,
                               vp(o["norm"]), vp(w), 4104, L.stream_ptr()))
    return Case(_adamw_inputs(n), call, outputs={"norm": torch.empty(1, device="cuda")})


@case("k_adamw_ema", ["jat_k_adamw_ema"])
def _k_adamw_ema():
    n = 4 * 2503

    def call(_, i, o):
        w = work_bytes(4104)
        ck(L.lib().jat_k_adamw_ema(vp(i["p"]), vp(i["g"]), vp(i["m"]), vp(i["v"]), vp(i["ema"]), n, 1e-3, 0.9, 0.999, 1e-8, 0.1,
                                   1.0, 2.0, 0.75, 3, vp(o["norm"]), vp(w), 4104, L.stream_ptr()))
    return Case(dict(_adamw_inputs(n), ema=gen((n,), 94)), call, outputs={"norm": torch.empty(1, device="cuda")})


@case("k_small_dw_and_dx", ["jat_k_small_dw", "jat_k_small_dx"])
def _k_small():
    B, N, K = 3, 6 * 256, 256
    need = ((N + 31) // 32) * B * K * 4          # slab 32 below N = 16384
    inputs = {"dy": gen((B, N), 60), "x": gen((B, K), 61), "W": gen((N, K), 62, K ** -0.5), "pre": gen((B, K), 63), "dx": gen((B, K), 64)}

    def call(_, i, o):
        w = work_bytes(need)
        ck(L.lib().jat_k_small_dw(vp(i["dy"]), N, vp(i["x"]), K, vp(o["dW"]), vp(o["db"]), B, N, K, 1, L.stream_ptr()))
        ck(L.lib().jat_k_small_dx(vp(i["dy"]), N, vp(i["W"]), 0, vp(i["dx"]), B, N, K, 1, vp(i["pre"]), vp(w), need, L.stream_ptr()))
    return Case(inputs, call, outputs={"dW": inputs["W"], "db": torch.empty(N, device="cuda")})


# ---- audio chain -----------------------------------------------------------------------------------------------------------
def _audio(B, n, seed):
    t = torch.arange(n, dtype=torch.float64)[None] / 44100.0
    f = torch.tensor([[220.0], [330.0], [147.0]][:B], dtype=torch.float64)
    return (0.5 * torch.sin(2 * np.pi * f * t)).float().cuda() + gen((B, n), seed, 0.05)


@case("resample", ["jat_resample"])
def _resample():
    from jatsr_amd.resample import resample
    return Case({"x": _audio(3, 4001, 1)}, lambda _, i, o: {"y": resample(i["x"], 44100, 16000)})


@case("resampler_created_on_the_stream", ["jat_resampler_create", "jat_resample"])
def _resampler_created():
    from jatsr_amd.resample import _Resampler
    keep = []

    def call(_, i, o):
        h = _Resampler(44100, 16000, 6, 0.99, i["x"].device)
        keep.append(h)
        y = torch.empty(3, h.out_length(4001), device="cuda")
        ck(L.lib().jat_resample(h.ptr, vp(i["x"]), vp(y), 3, 4001, L.stream_ptr()))
        return {"y": y}
    return Case({"x": _audio(3, 4001, 1)}, call)


@case("audio_metrics_created_on_the_stream", ["jat_audio_metrics_create", "jat_stft"])
def _metrics_created():
    from jatsr_amd.metrics import _Metrics
    keep = []
    n, n_fft, hop = 1301, 512, 128

    def call(_, i, o):
        h = _Metrics(44100, n_fft, hop, 0, i["x"].device)
        keep.append(h)
        X = torch.empty(2, h.bins, 1 + n // hop, dtype=torch.complex64, device="cuda")
        ck(L.lib().jat_stft(h.ptr, vp(i["x"]), None, 2, n, vp(X), None, L.stream_ptr()))
        return {"X": X}
    return Case({"x": _audio(2, n, 7)}, call)


@case("channel_stats", ["jat_channel_stats"])
def _channel_stats():
    from jatsr_amd.resample import channel_stats
    inputs = {"z": gen((2, 32, 37), 2), "sum": gen((32,), 3, dtype=torch.float64), "sq": gen((32,), 4, dtype=torch.float64).abs()}
    return Case(inputs, lambda _, i, o: channel_stats(i["z"], i["sum"], i["sq"]) and None)


@case("audio_metrics_run", ["jat_audio_metrics_run"])
def _audio_metrics():
    from jatsr_amd.metrics import _run

    def call(_, i, o):
        out, lsd, pdb, gdb = _run(i["pred"], i["gt"], 44100, 512, 128, 40, True, want_db=True)
        return {"out": out, "lsd_frames": lsd, "pred_db": pdb, "gt_db": gdb}
    return Case({"pred": _audio(2, 1301, 5), "gt": _audio(2, 1301, 6)}, call)


@case("stft", ["jat_stft"])
def _stft():
    from jatsr_amd.metrics import stft

    def call(_, i, o):
        X, Y = stft(i["x"], 512, 128, y=i["y"])
        return {"X": X, "Y": Y}
    return Case({"x": _audio(2, 1301, 7), "y": _audio(2, 1301, 8)}, call)


@case("istft", ["jat_istft"])
def _istft():
    from jatsr_amd.splice import istft
    n, n_fft, hop = 1301, 512, 128
    X = torch.view_as_complex(gen((2, 1 + n_fft // 2, 1 + n // hop, 2), 9))
    return Case({"X": X}, lambda _, i, o: {"y": istft(i["X"], n, n_fft, hop)})


@case("ltas", ["jat_ltas"])
def _ltas():
    from jatsr_amd.splice import ltas
    return Case({"x": _audio(2, 1301, 10)}, lambda _, i, o: {"P": ltas(i["x"], 512, 128)})


def _band_splice(n_fft, hop, n):
    from jatsr_amd.splice import band_gain, splice_gain
    gain = band_gain(44100, n_fft, 8000.0, 2000.0).cuda()
    return Case({"g": _audio(2, n, 11), "s": _audio(2, n + 7, 12), "gain": gain},
                lambda _, i, o: {"y": splice_gain(i["g"], i["s"], i["gain"], n_fft, hop)})


@case("band_splice_one_sample", ["jat_band_splice"])
def _band_splice_smallest():
    import splice_ref
    n_fft, hop, n = min(splice_ref.GPU_SHAPES, key=lambda s: s[2])
    return _band_splice(n_fft, hop, n)


@case("band_splice", ["jat_band_splice"])
def _band_splice_frames():
    return _band_splice(512, 128, 1301)


@case("yin_and_f0_compare", ["jat_yin", "jat_f0_compare"])
def _yin():
    from jatsr_amd.pitch import _counts, yin_full

    def call(_, i, o):
        a = yin_full(i["x"], frame_length=1024, hop_length=256, want=("index", "d", "cmndf"))
        b = yin_full(i["y"], frame_length=1024, hop_length=256)
        r = {"a_" + k: v for k, v in a.items()}
        r["counts"] = _counts(a["f0"], a["voiced"], b["f0"], b["voiced"], 50.0)
        return r
    x = _audio(2, 6000, 13)
    return Case({"x": x, "y": x * 0.9 + gen((2, 6000), 14, 0.2)}, call)


@case("pyin_track_and_decode", ["jat_pyin_track", "jat_pyin_decode"])
def _pyin():
    from jatsr_amd.pitch import pyin_decode, pyin_full
    kw = dict(frame_length=1024, hop_length=256)

    def call(_, i, o):
        r = pyin_full(i["x"], want=("cmndf", "prob", "bin", "obs", "log_obs", "state"), **kw)
        d = pyin_decode(r["log_obs"], **kw)
        return dict(r, **{"dec_" + k: v for k, v in d.items()})
    return Case({"x": _audio(2, 6000, 15)}, call)


def _dac(kind):
    if kind not in _shared:
        import jatsr_amd.dac as D
        m = D.DacDecoder() if kind == "dec" else D.DacEncoder()
        sd = recipe.make_dac_state_dict() if kind == "dec" else recipe.make_dac_encoder_state_dict()
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        _shared[kind] = m.cuda()
    return _shared[kind]


@case("dac_decode", ["jat_dac_decode"])
def _dac_decode():
    dec = _dac("dec")       # one handle: the harness's decoy run leaves decoy activations in it
    return Case({"z": cuda(recipe.gaussian("dac_stream", (2, 1024, 24), 4))}, lambda _, i, o: {"audio": dec(i["z"], precision="bf16x3")})


@case("dac_encode", ["jat_dac_encode"])
def _dac_encode():
    enc = _dac("enc")

    def call(_, i, o):
        z, codes, lat, hid = enc(i["audio"], precision="bf16x3", return_hidden=True)
        return {"z": z, "codes": codes, "latents": lat, "hidden": hid}
    return Case({"audio": _audio(2, 24 * 512, 16)[:, None].contiguous()}, call)


@case("dac_handles_created_on_the_stream", ["jat_dac_decoder_create", "jat_dac_encoder_create", "jat_dac_decode", "jat_dac_encode"])
def _dac_created():
    """small codecs (two blocks, 128 / 32 channels), their weights delayed inputs: creation reads them on the caller's stream"""
    import jatsr_amd.dac as D

    def modules():
        dec = D.DacDecoder(latent_channels=64, channels=128, strides=(4, 2))
        enc = D.DacEncoder(channels=32, hidden_size=1024, strides=(2, 4), n_codebooks=2)
        return dec.cuda(), enc.cuda()
    dec0, enc0 = modules()
    inputs = {"z": gen((2, 64, 24), 180), "audio": _audio(2, 24 * 8, 181)[:, None].contiguous()}
    names = {}
    for tag, mod in (("dec.", dec0), ("enc.", enc0)):
        for n, (k, v) in enumerate(mod.state_dict().items()):
            inputs[tag + k] = gen(tuple(v.shape), 182 + n, 0.2, 1.0 if "alpha" in k else 0.0)
            names[tag + k] = k

    def call(mods, i, o):
        dec, enc = mods
        for tag, mod in (("dec.", dec), ("enc.", enc)):
            mod.load_state_dict({names[k]: i[k] for k in names if k.startswith(tag)})     # device copies on the current stream
        z, codes, lat = enc(i["audio"])
        return {"audio": dec(i["z"]), "z": z, "codes": codes, "latents": lat}
    return Case(inputs, call, state=lambda live, outs: modules())


@case("k_dac_split_conv", ["jat_k_dac_split", "jat_k_dac_conv"])
def _k_dac_conv():
    import jatsr_amd.dac as D
    B, T, Cc, dil = 2, 37, 96, 3
    wp = D.pack_weight(0, recipe.uniform("k7w", (Cc, Cc, 7), dil) * np.float32((7 * Cc) ** -0.5), Cc, Cc, 7)
    inputs = {"a": gen((B * T, Cc), 100), "w": cuda(wp), "bias": gen((Cc,), 101, 0.1), "alpha": 1.75 + gen((Cc,), 102, 0.3).abs()}

    def call(_, i, o):
        (a_hi, a_lo), (w_hi, w_lo) = D.split_planes(i["a"]), D.split_planes(i["w"])
        ck(L.lib().jat_k_dac_conv(vp(a_hi), vp(a_lo), vp(w_hi), vp(w_lo), vp(i["bias"]), None, vp(o["o32"]), vp(i["alpha"]),
                                  vp(o["hi"]), vp(o["lo"]), B, T, Cc, Cc, Cc, 7, dil, 0, L.stream_ptr()))
        return {"a_hi": a_hi, "a_lo": a_lo}
    planes = torch.empty(B * T, Cc, dtype=torch.int16, device="cuda")
    return Case(inputs, call, outputs={"o32": inputs["a"], "hi": planes, "lo": planes})


@case("k_dac_head_tail", ["jat_k_dac_head", "jat_k_dac_tail"])
def _k_dac_head_tail():
    import jatsr_amd.dac as D
    B, n, Cc = 2, 1003, 64
    inputs = {"audio": _audio(2, n, 17), "w": gen((Cc, 1, 7), 110, 0.5), "bias": gen((Cc,), 111, 0.1),
              "alpha": 1.75 + gen((Cc,), 112, 0.3).abs(), "tw": gen((7, Cc), 113, 0.1), "tb": gen((1,), 114, 0.1)}

    def call(_, i, o):
        o32, (hi, lo) = D.head(i["audio"], i["w"], i["bias"], i["alpha"])
        ck(L.lib().jat_k_dac_tail(vp(o32), vp(i["alpha"]), vp(i["tw"]), vp(i["tb"]), vp(o["y"]), B, n, Cc, L.stream_ptr()))
        return {"o32": o32, "hi": hi, "lo": lo}
    return Case(inputs, call, outputs={"y": torch.empty(B, 1, n, device="cuda")})


@case("k_dac_rvq", ["jat_k_dac_rvq"])
def _k_dac_rvq():
    B, T, nq = 3, 45, 9
    shapes = {"in_proj.weight": (8, 1024), "in_proj.bias": (8,), "codebook.weight": (1024, 8), "out_proj.weight": (1024, 8),
              "out_proj.bias": (1024,)}
    inputs = {"hidden": gen((B * T, 1024), 120, 1.5)}
    for n, (k, shp) in enumerate(shapes.items()):
        inputs[k] = gen((nq,) + shp, 121 + n, 0.3)

    def call(_, i, o):
        ck(L.lib().jat_k_dac_rvq(vp(i["hidden"]), vp(i["in_proj.weight"]), vp(i["in_proj.bias"]), vp(i["codebook.weight"]),
                                 vp(i["out_proj.weight"]), vp(i["out_proj.bias"]), vp(o["z"]), vp(o["codes"]), vp(o["lat"]),
                                 vp(o["hid"]), B, T, 1024, nq, L.stream_ptr()))
    f = torch.empty(B, 1024, T, device="cuda")
    return Case(inputs, call, outputs={"z": f, "codes": torch.empty(B, nq, T, dtype=torch.int32, device="cuda"),
                                       "lat": torch.empty(B, 8 * nq, T, device="cuda"), "hid": f})


# ---- data ------------------------------------------------------------------------------------------------------------------
@case("latent_gather", ["jat_latent_gather"])
def _latent_gather():
    B, Cc, T, n = 1, 32, 37, 61
    inputs = {"hr": gen((Cc, n), 130, dtype=torch.float16), "lr": gen((Cc, n), 131, dtype=torch.float16),
              "len_start": torch.tensor([[n], [13]], dtype=torch.int64, device="cuda")}
    for j, k in enumerate(("hr_mean", "hr_std", "lr_mean", "lr_std")):
        inputs[k] = gen((Cc,), 132 + j).abs() + 0.3
    decoys = {"len_start": torch.tensor([[n], [3]], dtype=torch.int64, device="cuda")}      # another crop, inside the clip

    def state(live, outs):       # the address table points at this run's live source buffers; it is not a delayed input
        return torch.tensor([[live["hr"].data_ptr()], [live["lr"].data_ptr()]], dtype=torch.int64).cuda()

    def call(ptrs, i, o):
        ck(L.lib().jat_latent_gather(vp(ptrs[0]), vp(ptrs[1]), vp(i["len_start"][0]), vp(i["len_start"][1]), vp(i["hr_mean"]),
                                     vp(i["hr_std"]), vp(i["lr_mean"]), vp(i["lr_std"]), vp(o["hr_out"]), vp(o["lr_out"]), B, Cc, T,
                                     L.stream_ptr()))
    f = torch.empty(B, Cc, T, device="cuda")
    return Case(inputs, call, outputs={"hr_out": f, "lr_out": f}, decoys=decoys, state=state)


@case("train_monitor", ["jat_train_monitor"])
def _train_monitor():
    from jatsr_amd.train import train_monitor
    return Case({"pred": gen((3, 5, 7), 140), "target": gen((3, 5, 7), 141), "clean": gen((3, 5, 7), 142)},
                lambda _, i, o: {"sums": train_monitor(i["pred"], i["target"], i["clean"])})


# ---- retrieval -------------------------------------------------------------------------------------------------------------
@case("bank", ["jat_bank_add", "jat_bank_load_rows", "jat_bank_search", "jat_bank_blend", "jat_bank_search_topk", "jat_bank_blend_topk"])
def _bank():
    """a paired bank filled on the case's stream (300 frames added, 100 ready rows loaded), then searched and blended: the bank's
    contents are delayed inputs too"""
    from jatsr_amd.retrieval import LatentBank
    Cc, n, rows = 32, 300, 100
    inputs = {"lr_src": gen((Cc, n), 150), "hr_src": gen((Cc, n), 151), "keys": gen((rows, Cc), 152, dtype=torch.float16),
              "values": gen((rows, Cc), 153, dtype=torch.float16), "x": gen((2, Cc, 37), 154)}
    for j, k in enumerate(("k_mean", "k_std", "v_mean", "v_std")):
        inputs[k] = gen((Cc,), 155 + j).abs() * 0.5 + 0.5

    def call(bank, i, o):
        ck(L.lib().jat_bank_add(bank._h, vp(i["lr_src"]), vp(i["hr_src"]), 0, n, 0, 1, n, vp(i["k_mean"]), vp(i["k_std"]),
                                vp(i["v_mean"]), vp(i["v_std"]), L.stream_ptr()))
        bank.load_rows(i["keys"], i["values"])
        assert len(bank) == n + rows
        idx, d2 = bank.search(i["x"], i["k_mean"], i["k_std"])
        y = bank.blend(i["x"], idx, 0.6, i["v_mean"], i["v_std"])
        idx3, d3 = bank.search_topk(i["x"], 3, i["k_mean"], i["k_std"])
        y3 = bank.blend_topk(i["x"], idx3, d3, 0.6, i["v_mean"], i["v_std"])
        return {"idx": idx, "dist2": d2, "y": y, "idx3": idx3, "dist23": d3, "y3": y3, "rows": bank.rows("keys")[0].clone(),
                "norms": bank.rows("keys")[1].clone(), "vrows": bank.rows("values")[0].clone()}
    return Case(inputs, call, state=lambda live, outs: LatentBank(Cc, 512, key="lr"))


# ---- the test --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_side_stream(name):
    covers, build = CASES[name]
    check_case(build(), name, synchronises=any(e in SYNCHRONISES for e in covers))


def test_the_never_synchronise_entries_are_not_in_the_table():
    """after creation every bank call "only enqueues on the caller's stream, never synchronises"; and the per-step
    entries enter the table only through the pull request's description, never silently."""
    per_step = ["jat_forward", "jat_sampler_run", "jat_trainer_prepare", "jat_trainer_fwd_bwd", "jat_trainer_fwd_bwd_ex",
                "jat_trainer_optim", "jat_latent_gather", "jat_resample"]
    banks = ["jat_bank_add", "jat_bank_load_rows", "jat_bank_search", "jat_bank_blend", "jat_bank_search_topk", "jat_bank_blend_topk"]
    assert not set(per_step + banks) & set(SYNCHRONISES)
