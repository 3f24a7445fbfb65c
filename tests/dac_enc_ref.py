"""CPU restatement of transformers' DacEncoder.forward and DacResidualVectorQuantizer.forward in eval mode
(models/dac/modeling_dac.py:86-100, 103-173, 175-234, 283-345, 444-475) in torch fp64 — test infrastructure only, pinned to
the committed fixtures (tests/golden/dac44k_enc_*.npz) by tests/test_dac_encoder_cpu.py so that the GPU tests can use it at
shapes no fixture covers.  Parameters are the folded encoder state under DacModel names (`encoder.*`, `quantizer.*`)."""
import numpy as np
import torch
import torch.nn.functional as F

from dac_ref import snake


def _t(sd, k):
    return torch.as_tensor(np.asarray(sd[k]), dtype=torch.float64)


def res_unit(x, sd, pre, dil):
    y = F.conv1d(snake(x, _t(sd, pre + ".snake1.alpha")), _t(sd, pre + ".conv1.weight"), _t(sd, pre + ".conv1.bias"),
                 padding=3 * dil, dilation=dil)
    y = F.conv1d(snake(y, _t(sd, pre + ".snake2.alpha")), _t(sd, pre + ".conv2.weight"), _t(sd, pre + ".conv2.bias"))
    return x + y


def block(x, sd, i, stride):
    p = f"encoder.block.{i}"
    for u, d in zip((1, 2, 3), (1, 3, 9)):
        x = res_unit(x, sd, f"{p}.res_unit{u}", d)
    x = snake(x, _t(sd, p + ".snake1.alpha"))
    return F.conv1d(x, _t(sd, p + ".conv1.weight"), _t(sd, p + ".conv1.bias"), stride=stride, padding=(stride + 1) // 2)


def encode_hidden(audio, sd, strides=(2, 4, 8, 8)):
    """audio [B, 1, L] -> encoder output hidden [B, 1024, floor(L / prod(strides))] in fp64 (numpy in, numpy out)."""
    with torch.no_grad():
        x = torch.as_tensor(np.asarray(audio), dtype=torch.float64)
        x = F.conv1d(x, _t(sd, "encoder.conv1.weight"), _t(sd, "encoder.conv1.bias"), padding=3)
        for i, s in enumerate(strides):
            x = block(x, sd, i, s)
        x = snake(x, _t(sd, "encoder.snake1.alpha"))
        return F.conv1d(x, _t(sd, "encoder.conv2.weight"), _t(sd, "encoder.conv2.bias"), padding=1).numpy()


def quantize(hidden, sd, n_q=9, forced_codes=None):
    """RVQ of hidden [B, 1024, T] in fp64 -> dict(z [B, 1024, T], codes int64 [B, n_q, T], latents [B, 8 n_q, T],
    scores [B, n_q, T, codebook_size]: <normalize(e), normalize(c_j)> of every candidate at each decision).
    forced_codes [B, >= n_q, T]: follow these codes instead of the own argmax (a teacher-forced reference)."""
    with torch.no_grad():
        r = torch.as_tensor(np.asarray(hidden), dtype=torch.float64)
        z = torch.zeros_like(r)
        codes, lats, scores = [], [], []
        for i in range(n_q):
            p = f"quantizer.quantizers.{i}."
            e = F.conv1d(r, _t(sd, p + "in_proj.weight"), _t(sd, p + "in_proj.bias"))            # [B, 8, T]
            cb = _t(sd, p + "codebook.weight")                                                     # [K, 8]
            en = F.normalize(e.permute(0, 2, 1), dim=-1)
            sc = en @ F.normalize(cb, dim=-1).t()                                                  # [B, T, K]
            idx = sc.argmax(-1)   # first maximal index
            if forced_codes is not None:
                idx = torch.as_tensor(np.asarray(forced_codes)[:, i], dtype=torch.int64)
            q = F.conv1d(cb[idx].permute(0, 2, 1), _t(sd, p + "out_proj.weight"), _t(sd, p + "out_proj.bias"))
            z = z + q
            r = r - q
            codes.append(idx)
            lats.append(e)
            scores.append(sc)
        return {"z": z.numpy(), "codes": torch.stack(codes, 1).numpy(), "latents": torch.cat(lats, 1).numpy(),
                "scores": torch.stack(scores, 1).numpy()}


def margins(scores):
    """top-1 minus top-2 score of every decision, [B, n_q, T]."""
    s = np.sort(scores, axis=-1)
    return s[..., -1] - s[..., -2]
