#!/usr/bin/env python3
"""Generate tests/golden/train_loss_mod3_*.npz and train_*_mod3*_T*.npz: the V3-MOD3 trainer's loss and one of its steps, computed by
the REFERENCE's own functions under torch autograd.

Build container only (needs the reference checkout beside the repository, as oracle/gen_golden_train.py does, and CPU PyTorch):

    python tools/gen_golden_mod3.py            # all cases
    python tools/gen_golden_mod3.py loss       # a subset: loss, step

What is pinned.  `charbonnier_loss` (train_ddp_v3mod3.py:57-85) and the four loss classes (:88-355) are taken from the file itself
with `ast` at generation time (the module cannot be imported: tensorboard, process group); the two statements that combine them
(:955-969; validation :1138-1159) are issued here:

    recon = charbonnier_loss(pred, hr, eps)           or F.mse_loss(pred, hr) with use_charbonnier_loss = False
    loss  = reconstruction_weight * recon + latent_loss_weight * CombinedLatentPerceptualLoss(pred, hr, lr)[0]

Loss fixtures use the inputs of the v3mod2 loss fixtures (oracle/gen_golden_train.py `loss_case`), T1378 on 16 rows.  Step fixtures
follow `mod2_step_case`: JaT_AudioSR_V2 (LayerNorm), dropout = drop_path = 0, injected condition noise.  Only metadata and expected
VALUES are written.
"""
from __future__ import annotations

import ast
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import jatsr_amd.recipe as recipe  # noqa: E402
from oracle import gen_golden_train as G  # noqa: E402  (ref_model, sub, step_inputs; puts the reference on sys.path)

SOURCE = "train_ddp_v3mod3.py"
CLASSES = ("FrequencyDomainLatentLoss", "MultiScaleLatentLoss", "HybridConsistencyLoss", "CombinedLatentPerceptualLoss")
# TrainConfig of train_ddp_v3mod3.py:408-422
DEFAULTS = dict(eps=1e-6, rw=1.0, lw=0.3, fw=0.5, mw=0.5, cw=0.1)


def ref_mod3():
    """-> (charbonnier_loss, CombinedLatentPerceptualLoss) of the mod3 trainer."""
    import torch.nn as nn
    import torch.nn.functional as F
    tree = ast.parse(open(os.path.join(G.REF, SOURCE), encoding="utf-8").read())
    body = [n for n in tree.body if (isinstance(n, ast.ClassDef) and n.name in CLASSES)
            or (isinstance(n, ast.FunctionDef) and n.name == "charbonnier_loss")]
    assert len(body) == 5, [n.name for n in body]
    ns = {"torch": torch, "nn": nn, "F": F}
    exec(compile(ast.Module(body=body, type_ignores=[]), SOURCE, "exec"), ns)
    return ns["charbonnier_loss"], ns["CombinedLatentPerceptualLoss"]


def mod3_total(charb, fn, pred, target, lr, eps, rw, lw):
    """The trainer's statements :955-969.  eps == 0: use_charbonnier_loss = False."""
    recon = charb(pred, target, eps=eps) if eps > 0 else torch.nn.functional.mse_loss(pred, target)
    lat, terms = fn(pred, target, lr)
    return rw * recon + lw * lat, recon, lat, terms


def loss_case(name, B, C, T, salt=0, **over):
    """Value and d/d pred of the mod3 loss on the recipe tensors of the v3mod2 loss fixtures; fp32 inside the latent classes, as the
    reference forces.  Three settings: the reference's (rw = 1), rw = 0.25, and MSE (use_charbonnier_loss = False) with rw = 0.25."""
    s = dict(DEFAULTS, **over)
    charb, Loss = ref_mod3()
    fn = Loss(freq_weight=s["fw"], ms_weight=s["mw"], consistency_weight=s["cw"], low_freq_phase_ratio=0.3)
    target = torch.from_numpy(recipe.gaussian("loss_target", (B, C, T), salt + 401))
    lr = torch.from_numpy(0.7 * recipe.gaussian("loss_target", (B, C, T), salt + 401)
                          + 0.5 * recipe.gaussian("loss_lr", (B, C, T), salt + 402)).float()
    rec = {}
    for tag, eps, rw in (("", s["eps"], s["rw"]), ("_rw025", s["eps"], 0.25), ("_mse_rw025", 0.0, 0.25)):
        pred = torch.from_numpy(recipe.gaussian("loss_pred", (B, C, T), salt + 400)).requires_grad_(True)
        total, recon, lat, terms = mod3_total(charb, fn, pred, target, lr, eps, rw, s["lw"])
        total.backward()
        rec.update({"total" + tag: np.float64(total.item()), "recon" + tag: np.float64(recon.item()), "dpred" + tag: pred.grad.numpy()})
        if not tag:
            rec.update(freq=np.float64(terms["freq_loss"]), ms=np.float64(terms["ms_loss"]),
                       consistency=np.float64(terms["consistency_loss"]), latent=np.float64(terms["total_latent_loss"]))
    rec["meta"] = json.dumps(dict(case=name, B=B, C=C, T=T, salt=salt, torch=torch.__version__, source=SOURCE, **s))
    path = os.path.join(G.GOLD, f"train_loss_mod3_{name}.npz")
    np.savez_compressed(path, **rec)
    print(f"[golden] train_loss_mod3_{name}: total={rec['total']:.6f} recon={rec['recon']:.6f} latent={rec['latent']:.5f} "
          f"({os.path.getsize(path) / 1024:.0f} KiB)")


def step_case(name, cfg_name, B, T, t_list, salt=0, strides=(7, 5), cond_noise_ratio=0.05, **over):
    """One mod3 step end to end (train_ddp_v3mod3.py:920-969): LayerNorm model, condition noise on the model input, the loss against
    the clean LR latent; fp64 model, gradients of every parameter."""
    s = dict(DEFAULTS, **over)
    charb, Loss = ref_mod3()
    fn = Loss(freq_weight=s["fw"], ms_weight=s["mw"], consistency_weight=s["cw"], low_freq_phase_ratio=0.3)
    cfg = recipe.CONFIGS[cfg_name]
    hr, lr, noise = G.step_inputs(cfg, B, T, salt)
    cnoise = cond_noise_ratio * recipe.gaussian("train_cnoise", hr.shape, salt + 303)
    t = np.asarray(t_list, dtype=np.float32)
    m = G.ref_model(cfg, "ln", salt, torch.float64)
    hr_t, lr_t, nz, cn = (torch.from_numpy(a).double() for a in (hr, lr, noise, cnoise))
    tt = torch.from_numpy(t).double()
    tv = tt.view(-1, 1, 1)
    pred = m(tv * hr_t + (1 - tv) * nz, tt, lr_t + cn)
    loss, recon, lat, _ = mod3_total(charb, fn, pred, hr_t, lr_t, s["eps"], s["rw"], s["lw"])
    loss.backward()
    rec = {"loss64": np.float64(loss.item()), "recon": np.float64(recon.item()), "latent": np.float64(lat.item()),
           "pred_l2": np.float64(pred.detach().norm().item())}
    for k, p in m.named_parameters():
        rec["g_" + k] = G.sub(p.grad.numpy(), strides)
        rec["gl2_" + k] = np.float64(p.grad.norm().item())
    rec["meta"] = json.dumps(dict(case=name, cfg=cfg_name, B=B, T=T, t=[float(v) for v in t], norm="ln", salt=salt,
                                  cond_noise_ratio=cond_noise_ratio, full_limit=G.FULL_LIMIT, strides=strides, stride1d=None,
                                  torch=torch.__version__, source=SOURCE, names=[k for k, _ in m.named_parameters()], **s))
    path = os.path.join(G.GOLD, f"train_{name}.npz")
    np.savez_compressed(path, **rec)
    print(f"[golden] train_{name}: loss={rec['loss64']:.6f} ({s['rw']} * recon {rec['recon']:.6f} + {s['lw']} * latent "
          f"{rec['latent']:.5f}; {os.path.getsize(path) / 1024:.0f} KiB)")


def main(which):
    os.makedirs(G.GOLD, exist_ok=True)
    torch.set_num_threads(min(os.cpu_count() or 8, 16))
    allc = not which
    if allc or "loss" in which:
        loss_case("T24", 2, 32, 24)
        loss_case("T23", 2, 32, 23, salt=4)               # prime T: the direct-DFT kernel
        loss_case("T1378", 1, 16, 1378, salt=3)           # the trainer's crop, 16 rows
    if allc or "step" in which:
        step_case("micro_mod3_T24", "micro", 2, 24, [0.1, 0.85], salt=2)
        step_case("tiny_mod3_T128", "tiny", 2, 128, [0.2, 0.9], salt=1, strides=(61, 53))
        # fw = 0 twins: without the ill-conditioned log-magnitude term (see mod2_step_case in oracle/gen_golden_train.py) the whole
        # gradient chain is comparable with the reference's autograd directly
        # Their stored gradients are what the GPU test compares with, tensor by tensor, and a Charbonnier step's gradient error is
        # noise-like at a few 1e-2, not the few 1e-3 of an MSE step: the strided sample of a large matrix has to be big
        # enough to estimate a rel-L2 (m samples: about 1 / sqrt(2 m) relative scatter, more where a few rows carry the norm).  The
        # (61, 53) of the tiny cases leaves 25 values of a 512 x 512 weight.  Odd strides as dense as the 1 MiB limit on a fixture
        # allows: >= 2000 values of every micro matrix, >= 400 of every tiny one.
        step_case("micro_mod3fw0_T24", "micro", 2, 24, [0.1, 0.85], salt=2, strides=(5, 3), fw=0.0)
        step_case("tiny_mod3fw0_T128", "tiny", 2, 128, [0.2, 0.9], salt=1, strides=(29, 23), fw=0.0)


if __name__ == "__main__":
    main(sys.argv[1:])
