#!/usr/bin/env python3
"""How much the parameter gradients of one training step move when only the PREDICTION moves by what a bf16 forward moves it
(rel-L2 4.5e-3, measured on the GPU for the micro and tiny step fixtures): fp64 numpy throughout (oracle forward, the loss twin
tests/mod3_loss_ref.py, oracle backward), no GPU, nothing of the product path.  White noise of that size is added to the fp64
prediction and the per-tensor rel-L2 change of every gradient is reported against the 6e-2 gate of the step tests.

    python tools/mod3_conditioning.py

Charbonnier with eps = 1e-6 has the gradient e / sqrt(e^2 + eps) / n, +-1/n for |e| >> 1e-3: every element the perturbation carries
across pred == target changes by 2/n.  The MSE gradient 2e/n moves by the perturbation itself.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import jatsr_amd.recipe as recipe  # noqa: E402
import mod3_loss_ref as M3  # noqa: E402
from helpers import load_golden, rel_l2  # noqa: E402
from oracle import jat_oracle_train as OT  # noqa: E402

PERTURBATION, GATE, TRIALS = 4.5e-3, 6e-2, 3


def main():
    for name in ("train_micro_mod2fw0_T24", "train_micro_mod3fw0_T24", "train_tiny_mod3fw0_T128"):
        _, meta = load_golden(name)
        cfg = recipe.CONFIGS[meta["cfg"]]
        C, B, T, salt = cfg["input_channels"], meta["B"], meta["T"], meta["salt"]
        hr, lr, noise = (recipe.gaussian(k, (B, C, T), salt + 300 + i).astype(np.float64)
                         for i, k in enumerate(("train_hr", "train_lr", "train_noise")))
        cn = 0.05 * recipe.gaussian("train_cnoise", (B, C, T), salt + 303).astype(np.float64)
        t = np.asarray(meta["t"], np.float32).astype(np.float64)
        tv = t.reshape(B, 1, 1)
        orc = OT.TrainOracle(cfg, recipe.make_state_dict(cfg, "ln", salt), "ln")
        pred = orc.forward(tv * hr + (1 - tv) * noise, t, lr + cn)
        kw = dict(recon_eps=meta.get("eps", 0.0), recon_weight=meta.get("rw", 1.0), latent_weight=meta["lw"],
                  freq_weight=meta["fw"], ms_weight=meta["mw"], consistency_weight=meta["cw"])
        dp0 = M3.mod3_loss(pred, hr, lr, **kw)[1]
        g0 = orc.backward(dp0)
        gn = np.sqrt(sum(float((g * g).sum()) for g in g0.values()))
        rng = np.random.default_rng(0)
        for trial in range(TRIALS):
            d = rng.standard_normal(pred.shape)
            d *= PERTURBATION * np.linalg.norm(pred) / np.linalg.norm(d)
            dp1 = M3.mod3_loss(pred + d, hr, lr, **kw)[1]
            g1 = orc.backward(dp1)
            r = [rel_l2(g1[k], g0[k]) for k in g0 if np.linalg.norm(g0[k]) >= 1e-3 * gn]
            print(f"{name} (recon eps {kw['recon_eps']:g}) trial {trial}: d loss/d pred moves by rel-L2 {rel_l2(dp1, dp0):.3f}; gradients "
                  f"per tensor: median {np.median(r):.2e}, worst {max(r):.2e}, {sum(v > GATE for v in r)} of {len(r)} over {GATE:g}")


if __name__ == "__main__":
    main()
