"""DAC 44.1 kHz decoder: latent [B, 1024, T] -> audio [B, 1, T * 512] on the GPU.

The reference ends inference by decoding latents with the Descript Audio Codec (infer_test_v3m2.py:97-104, :408-437;
`dac_codec.decode`).  The computation is transformers' `DacDecoder.forward` (models/dac/modeling_dac.py:407-441): conv1,
four upsampling blocks (snake -> ConvTranspose1d, three dilated residual units), snake -> conv2 -> tanh.  All arithmetic
runs in the HIP kernels of csrc/dac.hip behind `jat_dac_*` (include/jat_hip.h); torch is only the container here.

Weights come from a file path (there is no download): a transformers `DacModel` / `DacDecoder` state dict (`.safetensors`,
`.pt`, `.bin`; plain `weight`, `weight_g`/`weight_v` or `parametrizations.weight.original0/1`), or a descript `dac` package
checkpoint (`.pth`, {"state_dict", "metadata"}).  The `dac` package key map (`decoder.model.{0..6}` ...) follows the
package's published module layout; no such file was available to confirm it against, so it rests on that layout alone.
Weight norm is folded as w = g * v / ||v|| over every dim but 0 (torch's `_weight_norm(v, g, 0)`, ConvTranspose1d too).

This module does not import `transformers`.
"""
from __future__ import annotations

import ctypes as C
import json
import re
from collections import OrderedDict

import numpy as np
import torch
from torch import nn

from . import _lib as L
from . import recipe

PRECISIONS = {"bf16x3": 0, "bf16": 1}
SAMPLE_RATE, HOP_LENGTH = 44100, 512


def _check(rc: int):
    # every failure of the decoder ABI (bad shape, missing weight, HIP error) surfaces as JatError
    if rc != L.JAT_OK:
        raise L.JatError(f"libjat_hip error {rc}: {L.lib().jat_last_error().decode('utf-8', 'replace')}")


# ---- weight files ------------------------------------------------------------------------------------------------------
_ST_DTYPES = {"F32": np.float32, "F16": np.float16, "F64": np.float64}


def read_safetensors(path) -> "OrderedDict[str, torch.Tensor]":
    """Minimal `.safetensors` reader (8-byte little-endian header length, JSON header, raw little-endian data)."""
    with open(path, "rb") as f:
        n = int.from_bytes(f.read(8), "little")
        header = json.loads(f.read(n))
        data = f.read()
    out = OrderedDict()
    for k, v in header.items():
        if k == "__metadata__":
            continue
        a, b = v["data_offsets"]
        if v["dtype"] == "BF16":
            arr = (np.frombuffer(data[a:b], dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)
        elif v["dtype"] in _ST_DTYPES:
            arr = np.frombuffer(data[a:b], dtype=_ST_DTYPES[v["dtype"]])
        else:
            continue   # integer buffers (none in the decoder)
        out[k] = torch.from_numpy(arr.astype(np.float32).reshape(v["shape"]))
    return out


def _dac_pkg_name(k: str):
    """descript `dac` package decoder key -> transformers DacDecoder key (None when not a decoder key)."""
    m = re.match(r"decoder\.model\.(\d+)\.(.*)$", k)
    if not m:
        return None
    i, rest = int(m.group(1)), m.group(2)
    if i == 0:
        return "conv1." + rest
    if i == 5:
        return "snake1." + rest
    if i == 6:
        return "conv2." + rest
    if not 1 <= i <= 4:
        return None
    blk = f"block.{i - 1}."
    m = re.match(r"block\.(\d+)\.(.*)$", rest)
    if not m:
        return None
    j, rest = int(m.group(1)), m.group(2)
    if j == 0:
        return blk + "snake1." + rest
    if j == 1:
        return blk + "conv_t1." + rest
    if j in (2, 3, 4):
        m = re.match(r"block\.(\d+)\.(.*)$", rest)
        if not m or int(m.group(1)) > 3:
            return None
        sub = ("snake1", "conv1", "snake2", "conv2")[int(m.group(1))]
        return f"{blk}res_unit{j - 1}.{sub}.{m.group(2)}"
    return None


def fold_weight_norm(g: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """w = g * v / ||v||, the norm over every dim but 0 (torch._weight_norm(v, g, 0)); computed in fp64."""
    v64, g64 = v.double(), g.double()
    norm = v64.reshape(v64.shape[0], -1).norm(dim=1).reshape([-1] + [1] * (v64.dim() - 1))
    return (g64.reshape(norm.shape) * v64 / norm).float()


def decoder_state_dict(raw: dict, dims: dict | None = None) -> "OrderedDict[str, torch.Tensor]":
    """Any supported checkpoint dict -> folded fp32 decoder parameters under DacDecoder names, checked against the shapes
    of `dims` (default: the 44.1 kHz model).  Encoder / quantizer keys are ignored; a missing or mis-shaped decoder key
    raises KeyError / ValueError naming it."""
    if "state_dict" in raw and isinstance(raw["state_dict"], dict):
        raw = raw["state_dict"]
    names = {}
    for k, v in raw.items():
        if not torch.is_tensor(v):
            continue
        if k.startswith("decoder.model."):
            n = _dac_pkg_name(k)
        elif k.startswith("decoder."):
            n = k[len("decoder."):]
        elif k.startswith(("encoder.", "quantizer.")):
            n = None
        else:
            n = k
        if n is not None:
            names[n] = v
    shapes = recipe.dac_param_shapes(**{**recipe.DAC44K, **(dims or {})})
    out = OrderedDict()
    for name, shape in shapes.items():
        if name.endswith(".weight"):
            base = name[: -len(".weight")]
            if name in names:
                w = names[name].float()
            elif base + ".weight_g" in names and base + ".weight_v" in names:
                w = fold_weight_norm(names[base + ".weight_g"], names[base + ".weight_v"])
            elif base + ".parametrizations.weight.original0" in names:
                w = fold_weight_norm(names[base + ".parametrizations.weight.original0"],
                                     names[base + ".parametrizations.weight.original1"])
            else:
                raise KeyError(f"DAC decoder weight missing: {name}")
        else:
            if name not in names:
                raise KeyError(f"DAC decoder parameter missing: {name}")
            w = names[name].float()
        if tuple(w.shape) != tuple(shape):
            raise ValueError(f"DAC decoder parameter {name} has shape {tuple(w.shape)}, expected {tuple(shape)}")
        out[name] = w.contiguous()
    return out


def load_decoder_file(path, dims: dict | None = None) -> "OrderedDict[str, torch.Tensor]":
    path = str(path)
    if path.endswith(".safetensors"):
        raw = read_safetensors(path)
    else:
        raw = torch.load(path, map_location="cpu", weights_only=False)
    return decoder_state_dict(raw, dims)


# ---- device handle -----------------------------------------------------------------------------------------------------
class _Handle:
    def __init__(self, named: dict, dims: dict, max_B: int, max_T: int, device):
        L.require_gpu()
        self.ptr = C.c_void_p()
        self.max_B, self.max_T, self.device = max_B, max_T, device
        st = list(dims["strides"])
        cfg = L.JatDacConfig(dims["latent_channels"], dims["channels"], len(st), (C.c_int32 * 4)(*(st + [0] * (4 - len(st)))))
        keep = [v.detach().to(device, torch.float32).contiguous() for v in named.values()]
        refs = (L.JatTensorRef * len(keep))()
        for i, (k, v) in enumerate(zip(named.keys(), keep)):
            refs[i] = L.JatTensorRef(k.encode(), v.data_ptr(), v.numel())
        with torch.cuda.device(device):
            _check(L.lib().jat_dac_decoder_create(C.byref(cfg), refs, len(keep), max_B, max_T, L.stream_ptr(),
                                                  C.byref(self.ptr)))

    def __del__(self):
        try:
            if self.ptr:
                L.lib().jat_dac_decoder_destroy(self.ptr)
        except Exception:
            pass

    def workspace_bytes(self) -> int:
        n = C.c_size_t()
        _check(L.lib().jat_dac_workspace_bytes(self.ptr, C.byref(n)))
        return n.value

    def decode(self, z: torch.Tensor, audio: torch.Tensor, precision: int):
        _check(L.lib().jat_dac_decode(self.ptr, L.ptr(z), L.ptr(audio), z.shape[0], z.shape[2], precision, L.stream_ptr()))


class _Param(nn.Module):
    def __init__(self, **shapes):
        super().__init__()
        for k, shp in shapes.items():
            self.register_parameter(k, nn.Parameter(torch.zeros(shp), requires_grad=False))


class _ResUnit(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.snake1, self.snake2 = _Param(alpha=(1, c, 1)), _Param(alpha=(1, c, 1))
        self.conv1, self.conv2 = _Param(weight=(c, c, 7), bias=(c,)), _Param(weight=(c, c, 1), bias=(c,))


class _Block(nn.Module):
    def __init__(self, cin, cout, stride):
        super().__init__()
        self.snake1 = _Param(alpha=(1, cin, 1))
        self.conv_t1 = _Param(weight=(cin, cout, 2 * stride), bias=(cout,))
        self.res_unit1, self.res_unit2, self.res_unit3 = _ResUnit(cout), _ResUnit(cout), _ResUnit(cout)


class DacDecoder(nn.Module):
    """transformers' DacDecoder (modeling_dac.py:407-441) with its parameter names, computed by csrc/dac.hip.

    Parameters hold the folded (plain) weights.  `forward(z)`: z fp32 [B, latent_channels, T] on the GPU -> audio fp32
    [B, 1, T * prod(strides)].  The device handle (re-laid-out bf16 weight planes + activations) is built on the first
    call and kept; it grows with the batch and length unless max_B / max_T are given, in which case larger calls raise.
    Call `refresh()` after changing the parameters in place."""

    def __init__(self, latent_channels=1024, channels=1536, strides=(8, 8, 4, 2), precision="bf16x3", max_B=None,
                 max_T=None):
        super().__init__()
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(PRECISIONS)}, got {precision!r}")
        self.dims = {"latent_channels": latent_channels, "channels": channels, "strides": tuple(strides)}
        self.precision = precision
        self.hop_length = int(np.prod(strides))
        self.max_B, self.max_T = max_B, max_T
        self.conv1 = _Param(weight=(channels, latent_channels, 7), bias=(channels,))
        self.block = nn.ModuleList(_Block(channels >> i, channels >> (i + 1), s) for i, s in enumerate(strides))
        cf = channels >> len(strides)
        self.snake1 = _Param(alpha=(1, cf, 1))
        self.conv2 = _Param(weight=(1, cf, 7), bias=(1,))
        self._handle = None

    def refresh(self):
        self._handle = None

    def _load_from_state_dict(self, *args, **kwargs):
        self._handle = None
        return super()._load_from_state_dict(*args, **kwargs)

    def _get_handle(self, B, T, device):
        h = self._handle
        if h is not None and h.device == device and B <= h.max_B and T <= h.max_T:
            return h
        mb = self.max_B or max(B, h.max_B if h is not None else 0)
        mt = self.max_T or max(T, h.max_T if h is not None else 0)
        self._handle = None
        self._handle = _Handle(self.state_dict(), self.dims, mb, mt, device)
        return self._handle

    @torch.no_grad()
    def forward(self, z: torch.Tensor, precision: str | None = None) -> torch.Tensor:
        prec = PRECISIONS.get(precision or self.precision)
        if prec is None:
            raise ValueError(f"precision must be one of {sorted(PRECISIONS)}, got {precision!r}")
        if z.dim() != 3 or z.shape[1] != self.dims["latent_channels"]:
            raise L.JatError(f"DAC decoder expects a latent [B, {self.dims['latent_channels']}, T], got {tuple(z.shape)}")
        B, _, T = z.shape
        if B < 1 or T < 1:
            raise L.JatError(f"DAC decoder: empty latent {tuple(z.shape)}")
        if not z.is_cuda:
            raise L.JatError("DAC decoder: the latent must be a CUDA tensor (there is no CPU path)")
        if (self.max_B and B > self.max_B) or (self.max_T and T > self.max_T):
            raise L.JatError(f"DAC decoder: latent {tuple(z.shape)} exceeds max_B={self.max_B} / max_T={self.max_T}")
        z = z.detach().to(torch.float32).contiguous()
        h = self._get_handle(B, T, z.device)
        audio = torch.empty(B, 1, T * self.hop_length, dtype=torch.float32, device=z.device)
        h.decode(z, audio, prec)
        return audio


class DacCodec:
    """What the reference's `dac_codec` provides on the decode side: `.decode(z)`, `.sample_rate`, `.hop_length`."""

    def __init__(self, decoder: DacDecoder):
        self.decoder = decoder
        self.sample_rate = SAMPLE_RATE
        self.hop_length = decoder.hop_length

    def decode(self, z: torch.Tensor) -> torch.Tensor:
        return self.decoder(z)


def load_dac_codec(path, device="cuda", precision="bf16x3") -> DacCodec:
    """Decoder of the 44.1 kHz DAC from a weight file (infer_test_v3m2.py:97-104 downloads it; here it is a path)."""
    sd = load_decoder_file(path)
    dec = DacDecoder(precision=precision)
    dec.load_state_dict(sd)
    return DacCodec(dec.to(device))


# ---- per-kernel entry points (tests) -----------------------------------------------------------------------------------
def pack_weight(kind: int, w: np.ndarray, cin: int, cout: int, k_or_stride: int) -> np.ndarray:
    """torch-layout fp32 weight -> [N, taps, cin] (jat_dac_pack_weight; kind 0 Conv1d, 1 ConvTranspose1d)."""
    w = np.ascontiguousarray(w, dtype=np.float32)
    taps, N = (3, k_or_stride * cout) if kind == 1 else (k_or_stride, cout)
    out = np.empty((N, taps, cin), np.float32)
    _check(L.lib().jat_dac_pack_weight(kind, w.ctypes.data, cin, cout, k_or_stride, out.ctypes.data))
    return out


def split_planes(x: torch.Tensor):
    """fp32 CUDA tensor -> (hi, lo) bf16 planes as int16 tensors (jat_k_dac_split)."""
    x = x.contiguous()
    hi = torch.empty(x.shape, dtype=torch.int16, device=x.device)
    lo = torch.empty_like(hi)
    _check(L.lib().jat_k_dac_split(L.ptr(x), L.ptr(hi), L.ptr(lo), x.numel(), L.stream_ptr()))
    return hi, lo


def conv(a, w_packed, bias, B, T, cin, N, cch, taps, dil=1, res=None, alpha=None, out32=True, precision="bf16x3"):
    """One jat_k_dac_conv on channels-last fp32 input a [B*T, cin] (split here) -> (out32 or None, snake planes or None)."""
    dev = a.device
    a_hi, a_lo = split_planes(a)
    w_hi, w_lo = split_planes(torch.from_numpy(np.ascontiguousarray(w_packed)).to(dev))
    o32 = torch.empty(B * T, N, dtype=torch.float32, device=dev) if out32 else None
    o_hi = o_lo = None
    if alpha is not None:
        o_hi = torch.empty(B * T, N, dtype=torch.int16, device=dev)
        o_lo = torch.empty_like(o_hi)
    _check(L.lib().jat_k_dac_conv(L.ptr(a_hi), L.ptr(a_lo), L.ptr(w_hi), L.ptr(w_lo), L.ptr(bias), L.ptr(res), L.ptr(o32),
                                  L.ptr(alpha), L.ptr(o_hi), L.ptr(o_lo), B, T, cin, N, cch, taps, dil,
                                  PRECISIONS[precision], L.stream_ptr()))
    return o32, (None if o_hi is None else (o_hi, o_lo))


def planes_to_float(hi: torch.Tensor, lo: torch.Tensor | None = None) -> torch.Tensor:
    f = (hi.to(torch.int32) << 16).view(torch.float32)
    if lo is not None:
        f = f + (lo.to(torch.int32) << 16).view(torch.float32)
    return f
