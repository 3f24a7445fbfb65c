"""fp64 twin of the V3-MOD3 trainer's loss (train_ddp_v3mod3.py:57-85,400-434,955-969) — TEST INFRASTRUCTURE, numpy only.

    loss = reconstruction_weight * recon + latent_weight * CombinedLatentPerceptualLoss(pred, target, lr)
    recon = charbonnier_loss(pred, target, eps) = mean(sqrt((pred - target)^2 + eps))     for eps > 0
          = F.mse_loss(pred, target)                                                      for eps == 0 (use_charbonnier_loss = False)

Composed from the two oracles the project already pins to the reference: `oracle.latent_loss_oracle.latent_loss` (mse + lw * latent
and its gradient; tests/test_train_cpu.py) and `oracle.jat_oracle_train.charbonnier_loss` (same file).  The MSE part of the former is
taken out again, 2 e / n, and the weighted reconstruction term put in its place.  tests/test_mod3_cpu.py pins this composition to
the reference's own mod3 functions under autograd (tests/golden/train_loss_mod3_*.npz, tools/gen_golden_mod3.py).
"""
import numpy as np

from oracle import jat_oracle_train as OT
from oracle import latent_loss_oracle as LO

TERMS = ("total", "mse", "freq", "ms", "consistency", "latent")      # the six slots of the kernels' out6, in order


def mod3_loss(pred, target, lr, recon_eps=1e-6, recon_weight=1.0, latent_weight=0.3, freq_weight=0.5, ms_weight=0.5,
              consistency_weight=0.1, low_freq_phase_ratio=0.3, strict_cutoff=0.30, soft_cutoff=0.36):
    """-> (terms, d total / d pred) in fp64.  pred, target, lr: [B, C, T].  terms has the keys of the v3mod2 oracle; "mse" is the
    un-weighted reconstruction term whatever its kind (the slot the kernels report it in) and "reconstruction" the same value."""
    terms, d = LO.latent_loss(pred, target, lr, latent_weight=latent_weight, freq_weight=freq_weight, ms_weight=ms_weight,
                              consistency_weight=consistency_weight, low_freq_phase_ratio=low_freq_phase_ratio,
                              strict_cutoff=strict_cutoff, soft_cutoff=soft_cutoff)
    e = np.asarray(pred, np.float64) - np.asarray(target, np.float64)
    mse_grad = 2.0 * e / e.size
    if recon_eps > 0:
        recon, drecon = OT.charbonnier_loss(pred, target, recon_eps)
    else:
        recon, drecon = float(terms["mse"]), mse_grad
    out = dict(terms, mse=recon, reconstruction=recon, total=recon_weight * recon + latent_weight * terms["latent"])
    return out, d - mse_grad + recon_weight * drecon
