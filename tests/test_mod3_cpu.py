"""CPU side of the V3-MOD3 trainer's loss (train_ddp_v3mod3.py: Charbonnier + latent perceptual loss with configurable weights):
the fp64 twin tests/mod3_loss_ref.py is PINNED to the reference's own functions under autograd (tests/golden/train_loss_mod3_*.npz
and the fw = 0 step fixtures, tools/gen_golden_mod3.py), and the host side — `fit` flags, `Trainer` argument errors, the public
symbols — is checked without a GPU.  Gates are those tests/test_train_cpu.py applies to the v3mod2 loss and the mod2fw0 steps."""
import math
import os
import re

import numpy as np
import pytest

import jatsr_amd._lib as L
import jatsr_amd.recipe as recipe
import mod3_loss_ref as M3
from helpers import load_golden, rel_l2
from jatsr_amd import fit as F
from jatsr_amd.train import Trainer
from oracle import jat_oracle_train as OT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOTAL_TOL, DPRED_TOL = 2e-6, 1e-4          # test_latent_loss_oracle_matches_reference_classes


def gsub(a, meta):
    s = meta["strides"]
    a = np.asarray(a)
    if a.size <= meta["full_limit"] or a.ndim != 2:
        return a if a.size <= meta["full_limit"] else a.reshape(-1)[::(meta.get("stride1d") or s[0] * s[1])]
    return a[::s[0], ::s[1]]


def loss_inputs(meta):
    B, C, Tn, salt = meta["B"], meta["C"], meta["T"], meta["salt"]
    pred = recipe.gaussian("loss_pred", (B, C, Tn), salt + 400)
    target = recipe.gaussian("loss_target", (B, C, Tn), salt + 401)
    lr = (0.7 * recipe.gaussian("loss_target", (B, C, Tn), salt + 401)
          + 0.5 * recipe.gaussian("loss_lr", (B, C, Tn), salt + 402)).astype(np.float32)
    return pred, target, lr


@pytest.mark.parametrize("name", ["train_loss_mod3_T24", "train_loss_mod3_T23", "train_loss_mod3_T1378"])
def test_twin_matches_reference_mod3_loss(name):
    """The reference's settings (rw = 1), rw = 0.25, and use_charbonnier_loss = False with rw = 0.25: total and every term within
    2e-6 relative, d total / d pred within rel-L2 1e-4 of the reference's autograd (fp32 inside its latent classes)."""
    z, meta = load_golden(name)
    x = loss_inputs(meta)
    kw = dict(latent_weight=meta["lw"], freq_weight=meta["fw"], ms_weight=meta["mw"], consistency_weight=meta["cw"])
    for tag, eps, rw in (("", meta["eps"], meta["rw"]), ("_rw025", meta["eps"], 0.25), ("_mse_rw025", 0.0, 0.25)):
        terms, dpred = M3.mod3_loss(*x, recon_eps=eps, recon_weight=rw, **kw)
        dev = {"total": abs(terms["total"] - float(z["total" + tag])) / abs(float(z["total" + tag])),
               "recon": abs(terms["mse"] - float(z["recon" + tag])) / abs(float(z["recon" + tag]))}
        if not tag:
            dev.update({k: abs(terms[k] - float(z[k])) / abs(float(z[k])) for k in ("freq", "ms", "consistency", "latent")})
        r = rel_l2(dpred, z["dpred" + tag])
        print(f"{name}{tag}: worst term {max(dev, key=dev.get)} {max(dev.values()):.2e} (gate {TOTAL_TOL:.0e}), dpred rel-L2 {r:.2e} "
              f"(gate {DPRED_TOL:.0e})")
        assert terms["reconstruction"] == terms["mse"]
        for k, v in dev.items():
            assert v <= TOTAL_TOL, (tag, k, v)
        assert r <= DPRED_TOL, (tag, r)


def test_twin_with_default_reconstruction_is_the_v3mod2_oracle():
    """eps = 0, rw = 1 is mse + lw * latent: the v3mod2 oracle's numbers (the gradient to the rounding of the MSE part taken out
    and put back)."""
    from oracle import latent_loss_oracle as LO
    _, meta = load_golden("train_loss_mod3_T23")
    x = loss_inputs(meta)
    terms, dpred = M3.mod3_loss(*x, recon_eps=0.0, recon_weight=1.0)
    ref, dref = LO.latent_loss(*x)
    assert all(terms[k] == ref[k] for k in M3.TERMS)
    assert rel_l2(dpred, dref) <= 1e-15


def step_oracle(meta):
    cfg = recipe.CONFIGS[meta["cfg"]]
    C, B, Tn, salt = cfg["input_channels"], meta["B"], meta["T"], meta["salt"]
    sd = recipe.make_state_dict(cfg, "ln", salt)
    hr = recipe.gaussian("train_hr", (B, C, Tn), salt + 300).astype(np.float64)
    lr = recipe.gaussian("train_lr", (B, C, Tn), salt + 301).astype(np.float64)
    noise = recipe.gaussian("train_noise", (B, C, Tn), salt + 302).astype(np.float64)
    cn = meta["cond_noise_ratio"] * recipe.gaussian("train_cnoise", (B, C, Tn), salt + 303).astype(np.float64)
    t = np.asarray(meta["t"], np.float32).astype(np.float64)
    tv = t.reshape(B, 1, 1)
    orc = OT.TrainOracle(cfg, sd, "ln")
    pred = orc.forward(tv * hr + (1 - tv) * noise, t, lr + cn)
    terms, dpred = M3.mod3_loss(pred, hr, lr, recon_eps=meta["eps"], recon_weight=meta["rw"], latent_weight=meta["lw"],
                                freq_weight=meta["fw"], ms_weight=meta["mw"], consistency_weight=meta["cw"])
    return terms, orc.backward(dpred), pred


@pytest.mark.parametrize("name", ["train_micro_mod3fw0_T24", "train_tiny_mod3fw0_T128"])
def test_train_oracle_with_the_twin_matches_reference_mod3_step(name):
    """LayerNorm model + Charbonnier + latent perceptual loss against the clean LR latent (train_ddp_v3mod3.py:920-969), fw = 0:
    TrainOracle.forward / .backward driven by the twin's d loss / d pred against the reference's autograd; tolerances of
    test_train_oracle_v3mod2_step_matches_reference."""
    z, meta = load_golden(name)
    assert meta["fw"] == 0.0 and meta["eps"] > 0
    terms, grads, pred = step_oracle(meta)
    assert abs(terms["total"] - float(z["loss64"])) <= 1e-6 * float(z["loss64"])
    assert abs(terms["mse"] - float(z["recon"])) <= 1e-9 * float(z["recon"])
    assert abs(np.linalg.norm(pred) - float(z["pred_l2"])) <= 1e-9 * float(z["pred_l2"])
    assert sorted(grads) == sorted(meta["names"])
    for k in meta["names"]:
        ref_l2 = float(z["gl2_" + k])
        assert abs(np.linalg.norm(grads[k]) - ref_l2) <= 2e-4 * max(ref_l2, 1e-30), k   # the reference runs its FFT terms in fp32
        assert rel_l2(gsub(grads[k], meta), z["g_" + k]) <= 5e-4, k


@pytest.mark.parametrize("name", ["train_micro_mod3_T24", "train_tiny_mod3_T128"])
def test_reference_settings_step_loss_matches_the_twin(name):
    """fw = 0.5 (the reference's settings): the loss value and its two parts; the gradients of these fixtures are compared on the
    GPU through the oracle backward only (the log-magnitude gradient is ill-conditioned, see `mod2_step_case`)."""
    z, meta = load_golden(name)
    terms, _, _ = step_oracle(meta)
    assert abs(terms["total"] - float(z["loss64"])) <= 1e-6 * float(z["loss64"])
    assert abs(terms["latent"] - float(z["latent"])) <= 2e-6 * float(z["latent"])


def test_fit_parser_has_the_mod3_flags_with_the_reference_defaults():
    a = F.build_parser().parse_args([])
    assert (a.loss, a.reconstruction_weight, a.charbonnier_eps) == ("mse", 1.0, 1e-6)
    assert (a.latent_loss_weight, a.freq_loss_weight, a.ms_loss_weight, a.consistency_weight) == (0.3, 0.5, 0.5, 0.1)
    a = F.build_parser().parse_args(["--loss", "charbonnier_latent", "--reconstruction-weight", "0.5", "--charbonnier-eps", "1e-3",
                                     "--freq-loss-weight", "0.25", "--ms-loss-weight", "0.75", "--consistency-weight", "0.2",
                                     "--ema-decay", "0.999", "--grad-accum-steps", "2", "--amp-dtype", "fp16", "--resume"])
    assert (a.loss, a.reconstruction_weight, a.charbonnier_eps) == ("charbonnier_latent", 0.5, 1e-3)
    assert (a.freq_loss_weight, a.ms_loss_weight, a.consistency_weight) == (0.25, 0.75, 0.2)
    assert (a.ema_decay, a.grad_accum_steps, a.amp_dtype, a.resume) == (0.999, 2, "fp16", "auto")
    assert F._loss_keywords(a) == dict(reconstruction_weight=0.5, charbonnier_eps=1e-3, freq_loss_weight=0.25,
                                       ms_loss_weight=0.75, consistency_weight=0.2)
    assert F.CHARBONNIER_TAG == "Train/Charbonnier_Loss" and F.TRAIN_TAGS["mse"] == "Train/MSE_Loss"


def test_fit_rejects_a_bad_loss_selection_before_the_gpu_is_needed():
    """`run` checks the loss flags first: these raise ValueError on a machine without a GPU (the next statement would raise JatError)."""
    def args(*more):
        return F.build_parser().parse_args(["--data-dir", "/nonexistent"] + list(more))
    with pytest.raises(ValueError, match="loss must be"):
        F.run(args("--loss", "charbonier_latent"))
    with pytest.raises(ValueError, match="latent"):
        F.run(args("--loss", "charbonnier"))                                  # the default latent weight 0.3
    with pytest.raises(ValueError, match="'charbonnier'"):
        F.run(args("--loss", "charbonnier_latent", "--latent-loss-weight", "0"))
    with pytest.raises(ValueError, match="charbonnier_eps"):
        F.run(args("--loss", "charbonnier_latent", "--charbonnier-eps=-1e-6"))
    with pytest.raises(ValueError, match="finite"):
        F.run(args("--loss", "charbonnier_latent", "--reconstruction-weight", "nan"))


def test_trainer_argument_errors_come_before_any_gpu_need():
    """model = None and no GPU: a ValueError can only come from the checks at the top of __init__."""
    with pytest.raises(ValueError, match="'charbonnier'"):                    # the default latent_loss_weight is 0
        Trainer(None, 1, 4, loss="charbonnier_latent")
    with pytest.raises(ValueError, match="'charbonnier'"):
        Trainer(None, 1, 4, loss="charbonnier_latent", latent_loss_weight=0.0)
    with pytest.raises(ValueError, match="charbonnier_eps"):
        Trainer(None, 1, 4, loss="charbonnier_latent", latent_loss_weight=0.3, charbonnier_eps=-1e-6)
    with pytest.raises(ValueError, match="charbonnier_eps"):
        Trainer(None, 1, 4, loss="charbonnier_latent", latent_loss_weight=0.3, charbonnier_eps=float("nan"))
    for kw in (dict(reconstruction_weight=float("nan")), dict(latent_loss_weight=float("inf")), dict(freq_loss_weight=float("nan")),
               dict(ms_loss_weight=float("-inf")), dict(consistency_weight=float("nan"))):
        with pytest.raises(ValueError, match="finite"):
            Trainer(None, 1, 4, loss="charbonnier_latent", **dict(dict(latent_loss_weight=0.3), **kw))
    with pytest.raises(ValueError, match="finite"):
        Trainer(None, 1, 4, loss="mse", reconstruction_weight=float("nan"))
    # the earlier spellings keep their errors; the message now names the new one
    with pytest.raises(ValueError, match="latent") as e:
        Trainer(None, 1, 4, loss="charbonnier", latent_loss_weight=0.3)
    assert "charbonnier_latent" in str(e.value)
    with pytest.raises(ValueError, match="loss must be"):
        Trainer(None, 1, 4, loss="charbonier")


def test_loss_config_carries_the_nine_values_in_abi_order():
    """The four loss selections `Trainer` accepts -> the argument list of jat_trainer_set_loss_ex / jat_k_latent_loss_ex (recon_eps,
    recon_weight, latent_weight, freq, ms, consistency, phase ratio, strict, soft), and the names the loss had as attributes."""
    from jatsr_amd.train import LossConfig, check_loss_arguments
    sub, bands = (0.25, 0.75, 0.2), (0.4, 0.25, 0.5)
    for loss, lw, rw, eps, recon_eps in (("mse", 0.0, 1.0, 1e-6, 0.0), ("mse", 0.3, 0.5, 1e-3, 0.0),
                                         ("charbonnier", 0.0, 2.0, 1e-3, 1e-3), ("charbonnier_latent", 0.3, 0.5, 1e-4, 1e-4)):
        c = check_loss_arguments(loss, lw, rw, eps, sub, bands)
        assert isinstance(c, LossConfig) and c.abi() == (recon_eps, rw, lw) + sub + bands, loss
        assert (c.name, c.charbonnier_eps, c.recon_eps, c.reconstruction_weight, c.has_latent) == (loss, eps, recon_eps, rw, lw != 0.0)
        assert all(type(v) is float for v in c.abi())
    # what is left out keeps the defaults of Trainer's signature and of the library's LossSpec
    assert check_loss_arguments("mse", 0).abi() == (0.0, 1.0, 0.0, 0.5, 0.5, 0.1, 0.3, 0.30, 0.36)
    assert len(L.SIGNATURES["jat_trainer_set_loss_ex"][1]) == 1 + len(check_loss_arguments("mse", 0).abi())
    # the work buffers of the two validation calls, as the entry points size them
    assert LossConfig.recon_work_bytes() == 4104
    assert LossConfig.latent_work_bytes(6, 35) == 512 + 192 and LossConfig.latent_work_bytes(1, 32) == 256 + 32
    # and the rejected selections raise what they raised
    for args, match in ((("charbonier", 0.0), "loss must be"), (("charbonnier", 0.3), "latent"), (("charbonnier_latent", 0.0), "'charbonnier'"),
                        (("charbonnier_latent", 0.3, 1.0, -1e-6), "charbonnier_eps"), (("mse", 0.0, float("nan")), "finite"),
                        (("mse", 0.3, 1.0, 1e-6, (0.5, float("inf"), 0.1)), "finite")):
        with pytest.raises(ValueError, match=match):
            check_loss_arguments(*args)


def test_new_symbols_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "jat_hip.h")).read()
    for name, doubles in (("jat_trainer_set_loss_ex", 9), ("jat_k_latent_loss_ex", 9)):
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in L.SIGNATURES
        assert sum(1 for a in L.SIGNATURES[name][1] if a is L.C.c_double) == doubles
    decl = header[header.index("int jat_k_latent_loss_ex("):]
    decl = decl[:decl.index(";")]
    assert decl.index("recon_eps") < decl.index("recon_weight") < decl.index("latent_weight") < decl.index("loss_scale")
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "jat_trainer_set_loss_ex" in text and "jat_k_latent_loss_ex" in text and "charbonnier_latent" in text
