"""CPU restatement of transformers' DacDecoder.forward (models/dac/modeling_dac.py:86-100,175-210,236-264,407-441) in
torch fp64 — test infrastructure only, pinned to the committed fixtures (tests/golden/dac44k_*.npz) by
tests/test_dac_cpu.py so that the GPU tests can use it at shapes no fixture covers."""
import numpy as np
import torch
import torch.nn.functional as F


def snake(x, alpha):
    a = torch.as_tensor(alpha, dtype=x.dtype).reshape(1, -1, 1)
    return x + (a + 1e-9).reciprocal() * torch.sin(a * x).pow(2)


def _t(sd, k):
    return torch.as_tensor(np.asarray(sd[k]), dtype=torch.float64)


def conv7(x, sd, pre, dil=1):
    return F.conv1d(x, _t(sd, pre + ".weight"), _t(sd, pre + ".bias"), padding=3 * dil, dilation=dil)


def conv_t(x, sd, pre, stride):
    return F.conv_transpose1d(x, _t(sd, pre + ".weight"), _t(sd, pre + ".bias"), stride=stride, padding=(stride + 1) // 2)


def res_unit(x, sd, pre, dil):
    y = conv7(snake(x, _t(sd, pre + ".snake1.alpha")), sd, pre + ".conv1", dil)
    y = F.conv1d(snake(y, _t(sd, pre + ".snake2.alpha")), _t(sd, pre + ".conv2.weight"), _t(sd, pre + ".conv2.bias"))
    return x + y


def block(x, sd, i, stride):
    p = f"block.{i}"
    x = conv_t(snake(x, _t(sd, p + ".snake1.alpha")), sd, p + ".conv_t1", stride)
    for u, d in zip((1, 2, 3), (1, 3, 9)):
        x = res_unit(x, sd, f"{p}.res_unit{u}", d)
    return x


def decode(z, sd, strides=(8, 8, 4, 2)):
    """z [B, latent, T] -> audio [B, 1, T * prod(strides)] in fp64 (numpy in, numpy out)."""
    with torch.no_grad():
        x = conv7(torch.as_tensor(np.asarray(z), dtype=torch.float64), sd, "conv1")
        for i, s in enumerate(strides):
            x = block(x, sd, i, s)
        x = snake(x, _t(sd, "snake1.alpha"))
        return torch.tanh(conv7(x, sd, "conv2")).numpy()
