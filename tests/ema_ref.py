"""fp64 numpy twin of the fused AdamW + EMA pass (csrc/train.hip adamw_ema_kernel) and of the decay schedule
(jatsr_amd.train.ema_decay_at).  The AdamW formulas are those of tests/test_gpu_train_kernels.py::test_adamw."""
import math

import numpy as np


def ema_decay_at(n, decay, warmup=True):
    """Decay of EMA update number n (1-based): min(decay, (1 + n) / (10 + n)) with warm-up, else decay."""
    return min(float(decay), (1.0 + n) / (10.0 + n)) if warmup else float(decay)


def ema_update(e, p_new, decay):
    """e + (1 - decay) * (p_new - e): the increment form the kernel uses."""
    return e + (1.0 - float(decay)) * (np.asarray(p_new, np.float64) - e)


def adamw_ema_step(p, g, m, v, e, lr, beta1, beta2, eps, wd, max_norm, loss_scale, step, decay):
    """clip_grad_norm_(max_norm) of g / loss_scale, one AdamW step, then the EMA of the new parameters.
    -> dict(p, m, v, e, norm): norm = L2 norm of the unscaled gradients.  A non-finite norm changes nothing."""
    p, g, m, v, e = (np.asarray(x, np.float64) for x in (p, g, m, v, e))
    gs = g / loss_scale
    norm = float(np.sqrt((gs * gs).sum()))
    if not math.isfinite(norm):
        return dict(p=p, m=m, v=v, e=e, norm=norm)
    coef = min(1.0, max_norm / (norm + 1e-6)) if max_norm > 0 else 1.0
    gr = gs * coef
    m = beta1 * m + (1 - beta1) * gr
    v = beta2 * v + (1 - beta2) * gr * gr
    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    p = p * (1 - lr * wd) - lr / bc1 * m / (np.sqrt(v) / math.sqrt(bc2) + eps)
    return dict(p=p, m=m, v=v, e=ema_update(e, p, decay), norm=norm)
