"""DAC 44.1 kHz codec on the GPU: decoder latent [B, 1024, T] -> audio [B, 1, T * 512], and encoder + residual vector
quantizer audio -> (z, codes, latents).

The encode side (`DacEncoder`, `DacCodec.encode`) is what the reference's data preparation calls
(prepare_dataset_v5.py:206-219: `z, _, _, _, _ = dac_model.encode(audio)`): transformers' DacEncoder.forward
(modeling_dac.py:444-475) and DacResidualVectorQuantizer.forward in eval mode (:283-345), in csrc/dac.hip +
csrc/dac_enc.hip behind `jat_dac_encode`.  `encoder_state_dict` reads the same file layouts as `decoder_state_dict`.

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
    return _fold(names, recipe.dac_param_shapes(**{**recipe.DAC44K, **(dims or {})}), "DAC decoder")


def _fold(names: dict, shapes: dict, what: str) -> "OrderedDict[str, torch.Tensor]":
    """names (model key -> tensor, weight norm unfolded or not) -> the folded fp32 parameters of `shapes`."""
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
                raise KeyError(f"{what} weight missing: {name}")
        else:
            if name not in names:
                raise KeyError(f"{what} parameter missing: {name}")
            w = names[name].float()
        if tuple(w.shape) != tuple(shape):
            raise ValueError(f"{what} parameter {name} has shape {tuple(w.shape)}, expected {tuple(shape)}")
        out[name] = w.contiguous()
    return out


def _dac_pkg_encoder_name(k: str):
    """descript `dac` package encoder key -> transformers DacModel key (None when not an encoder key).  The package's
    Encoder is `block = [conv1, EncoderBlock x 4, Snake1d, conv2]`, each EncoderBlock `[ResidualUnit x 3, Snake1d,
    strided conv]`, each ResidualUnit `[Snake1d, conv k7, Snake1d, conv k1]`; quantizer keys already match."""
    m = re.match(r"encoder\.block\.(\d+)\.(.*)$", k)
    if not m:
        return None
    i, rest = int(m.group(1)), m.group(2)
    if i == 0:
        return "encoder.conv1." + rest
    if i == 5:
        return "encoder.snake1." + rest
    if i == 6:
        return "encoder.conv2." + rest
    if not 1 <= i <= 4:
        return None
    blk = f"encoder.block.{i - 1}."
    m = re.match(r"block\.(\d+)\.(.*)$", rest)
    if not m:
        return None
    j, rest = int(m.group(1)), m.group(2)
    if j == 3:
        return blk + "snake1." + rest
    if j == 4:
        return blk + "conv1." + rest
    if j in (0, 1, 2):
        m = re.match(r"block\.(\d+)\.(.*)$", rest)
        if not m or int(m.group(1)) > 3:
            return None
        sub = ("snake1", "conv1", "snake2", "conv2")[int(m.group(1))]
        return f"{blk}res_unit{j + 1}.{sub}.{m.group(2)}"
    return None


def encoder_state_dict(raw: dict, dims: dict | None = None) -> "OrderedDict[str, torch.Tensor]":
    """Any supported checkpoint dict -> folded fp32 encoder and quantizer parameters under transformers' DacModel names
    (`encoder.*`, `quantizer.quantizers.{i}.*`), checked against the shapes of `dims` (default: the 44.1 kHz model).
    Reads the layouts decoder_state_dict reads; the descript `dac` key map (`encoder.block.{0..6}` ...) rests on that
    package's published module layout only.  A missing or mis-shaped key raises KeyError / ValueError naming it."""
    if "state_dict" in raw and isinstance(raw["state_dict"], dict):
        raw = raw["state_dict"]
    names = {}
    for k, v in raw.items():
        if not torch.is_tensor(v):
            continue
        if re.match(r"encoder\.block\.\d+\.(weight|bias|alpha|block\.)", k):   # descript layout
            n = _dac_pkg_encoder_name(k)
        elif k.startswith(("encoder.", "quantizer.")):
            n = k
        else:
            n = None
        if n is not None:
            names[n] = v
    return _fold(names, recipe.dac_encoder_param_shapes(**{**recipe.DAC44K_ENC, **(dims or {})}), "DAC encoder")


def _read_weight_file(path) -> dict:
    path = str(path)
    if path.endswith(".safetensors"):
        return read_safetensors(path)
    return torch.load(path, map_location="cpu", weights_only=False)


def load_decoder_file(path, dims: dict | None = None) -> "OrderedDict[str, torch.Tensor]":
    return decoder_state_dict(_read_weight_file(path), dims)


def load_encoder_file(path, dims: dict | None = None) -> "OrderedDict[str, torch.Tensor]":
    return encoder_state_dict(_read_weight_file(path), dims)


def _has_encoder(raw: dict) -> bool:
    if "state_dict" in raw and isinstance(raw["state_dict"], dict):
        raw = raw["state_dict"]
    return any(k.startswith("encoder.") for k in raw) and any(k.startswith("quantizer.") for k in raw)


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


class _EncHandle:
    def __init__(self, named: dict, dims: dict, max_B: int, max_T: int, device):
        L.require_gpu()
        self.ptr = C.c_void_p()
        self.max_B, self.max_T, self.device = max_B, max_T, device
        st = list(dims["strides"])
        cfg = L.JatDacEncoderConfig(dims["channels"], dims["hidden_size"], len(st),
                                    (C.c_int32 * 4)(*(st + [0] * (4 - len(st)))), dims["n_codebooks"],
                                    dims["codebook_size"], dims["codebook_dim"])
        keep = [v.detach().to(device, torch.float32).contiguous() for v in named.values()]
        refs = (L.JatTensorRef * len(keep))()
        for i, (k, v) in enumerate(zip(named.keys(), keep)):
            refs[i] = L.JatTensorRef(k.encode(), v.data_ptr(), v.numel())
        with torch.cuda.device(device):
            _check(L.lib().jat_dac_encoder_create(C.byref(cfg), refs, len(keep), max_B, max_T, L.stream_ptr(),
                                                  C.byref(self.ptr)))

    def __del__(self):
        try:
            if self.ptr:
                L.lib().jat_dac_encoder_destroy(self.ptr)
        except Exception:
            pass

    def workspace_bytes(self) -> int:
        n = C.c_size_t()
        _check(L.lib().jat_dac_encoder_workspace_bytes(self.ptr, C.byref(n)))
        return n.value

    def encode(self, audio, z, codes, latents, hidden, B, T, n_q, precision):
        _check(L.lib().jat_dac_encode(self.ptr, L.ptr(audio), L.ptr(z), L.ptr(codes), L.ptr(latents), L.ptr(hidden), B, T,
                                      n_q, precision, L.stream_ptr()))


class _EncBlock(nn.Module):
    def __init__(self, c, stride):
        super().__init__()
        self.res_unit1, self.res_unit2, self.res_unit3 = _ResUnit(c), _ResUnit(c), _ResUnit(c)
        self.snake1 = _Param(alpha=(1, c, 1))
        self.conv1 = _Param(weight=(2 * c, c, 2 * stride), bias=(2 * c,))


class _Encoder(nn.Module):
    def __init__(self, channels, hidden_size, strides):
        super().__init__()
        self.conv1 = _Param(weight=(channels, 1, 7), bias=(channels,))
        self.block = nn.ModuleList(_EncBlock(channels << i, s) for i, s in enumerate(strides))
        cf = channels << len(strides)
        self.snake1 = _Param(alpha=(1, cf, 1))
        self.conv2 = _Param(weight=(hidden_size, cf, 3), bias=(hidden_size,))


class _VQ(nn.Module):
    def __init__(self, hidden_size, codebook_size, codebook_dim):
        super().__init__()
        self.in_proj = _Param(weight=(codebook_dim, hidden_size, 1), bias=(codebook_dim,))
        self.out_proj = _Param(weight=(hidden_size, codebook_dim, 1), bias=(hidden_size,))
        self.codebook = _Param(weight=(codebook_size, codebook_dim))


class _RVQ(nn.Module):
    def __init__(self, n_codebooks, *dims):
        super().__init__()
        self.quantizers = nn.ModuleList(_VQ(*dims) for _ in range(n_codebooks))


class DacEncoder(nn.Module):
    """transformers' DacModel encode path — DacEncoder (modeling_dac.py:444-475) and DacResidualVectorQuantizer in eval
    mode (:283-345) — with its parameter names (`encoder.*`, `quantizer.quantizers.{i}.*`), computed by csrc/dac.hip and
    csrc/dac_enc.hip.

    Parameters hold the folded (plain) weights.  `forward(audio, n_quantizers=None, precision=None)`: audio fp32
    [B, 1, T * hop_length] on the GPU -> (z [B, hidden_size, T], codes int64 [B, n_q, T], latents [B, 8 n_q, T]).
    The length must be a multiple of hop_length (DacCodec.encode pads).  The convs run in `precision` (bf16x3 / bf16),
    the quantizer in fp32.  The device handle is built on the first call and grows like DacDecoder's."""

    def __init__(self, channels=64, hidden_size=1024, strides=(2, 4, 8, 8), n_codebooks=9, codebook_size=1024,
                 codebook_dim=8, precision="bf16x3", max_B=None, max_T=None):
        super().__init__()
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(PRECISIONS)}, got {precision!r}")
        self.dims = {"channels": channels, "hidden_size": hidden_size, "strides": tuple(strides),
                     "n_codebooks": n_codebooks, "codebook_size": codebook_size, "codebook_dim": codebook_dim}
        self.precision = precision
        self.hop_length = int(np.prod(strides))
        self.max_B, self.max_T = max_B, max_T
        self.encoder = _Encoder(channels, hidden_size, strides)
        self.quantizer = _RVQ(n_codebooks, hidden_size, codebook_size, codebook_dim)
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
        self._handle = _EncHandle(self.state_dict(), self.dims, mb, mt, device)
        return self._handle

    @torch.no_grad()
    def forward(self, audio: torch.Tensor, n_quantizers: int | None = None, precision: str | None = None,
                return_hidden: bool = False):
        prec = PRECISIONS.get(precision or self.precision)
        if prec is None:
            raise ValueError(f"precision must be one of {sorted(PRECISIONS)}, got {precision!r}")
        nq = self.dims["n_codebooks"] if n_quantizers is None else int(n_quantizers)
        if not 1 <= nq <= self.dims["n_codebooks"]:
            raise L.JatError(f"DAC encoder: n_quantizers {nq} outside 1..{self.dims['n_codebooks']}")
        if audio.dim() != 3 or audio.shape[1] != 1:
            raise L.JatError(f"DAC encoder expects audio [B, 1, L], got {tuple(audio.shape)}")
        B, _, n = audio.shape
        if B < 1 or n < self.hop_length or n % self.hop_length:
            raise L.JatError(f"DAC encoder: length {n} is not a positive multiple of {self.hop_length} "
                             "(DacCodec.encode pads)")
        if not audio.is_cuda:
            raise L.JatError("DAC encoder: the audio must be a CUDA tensor (there is no CPU path)")
        T = n // self.hop_length
        if (self.max_B and B > self.max_B) or (self.max_T and T > self.max_T):
            raise L.JatError(f"DAC encoder: audio {tuple(audio.shape)} exceeds max_B={self.max_B} / max_T={self.max_T}")
        audio = audio.detach().to(torch.float32).contiguous()
        h = self._get_handle(B, T, audio.device)
        dev, H = audio.device, self.dims["hidden_size"]
        z = torch.empty(B, H, T, dtype=torch.float32, device=dev)
        codes = torch.empty(B, nq, T, dtype=torch.int32, device=dev)
        lat = torch.empty(B, self.dims["codebook_dim"] * nq, T, dtype=torch.float32, device=dev)
        hid = torch.empty(B, H, T, dtype=torch.float32, device=dev) if return_hidden else None
        h.encode(audio, z, codes, lat, hid, B, T, nq, prec)
        out = (z, codes.long(), lat)
        return out + (hid,) if return_hidden else out


class DacCodec:
    """What the reference's `dac_codec` / `dac_model` provides: `.decode(z)`, `.encode(audio)`, `.sample_rate`,
    `.hop_length`."""

    def __init__(self, decoder: DacDecoder, encoder: DacEncoder | None = None):
        self.decoder = decoder
        self.encoder = encoder
        self.sample_rate = SAMPLE_RATE
        self.hop_length = decoder.hop_length

    def decode(self, z: torch.Tensor) -> torch.Tensor:
        return self.decoder(z)

    def encode(self, audio_data: torch.Tensor, n_quantizers: int | None = None):
        """descript's `DAC.encode` (prepare_dataset_v5.py:206-219: `z, _, _, _, _ = dac_model.encode(audio)`):
        audio [B, 1, L] -> (z [B, 1024, T], codes [B, n_q, T], latents [B, 8 n_q, T], None, None) with
        T = ceil(L / 512).  The audio is zero-padded on the right to a multiple of 512 as `DAC.preprocess` does, so for
        other L the last frames differ from an unpadded transformers `DacModel.encode` (which gives floor(L / 512)
        frames).  The codec's training losses are not computed."""
        if self.encoder is None:
            raise L.JatError("DAC codec: the weight file has no encoder / quantizer weights (decode only)")
        if audio_data.dim() == 2:
            audio_data = audio_data[:, None]
        n = audio_data.shape[-1]
        pad = (-n) % self.hop_length
        if pad or n == 0:
            audio_data = torch.nn.functional.pad(audio_data, (0, pad if n else self.hop_length))
        z, codes, latents = self.encoder(audio_data, n_quantizers=n_quantizers)
        return z, codes, latents, None, None


def load_dac_codec(path, device="cuda", precision="bf16x3") -> DacCodec:
    """The 44.1 kHz DAC from a weight file (infer_test_v3m2.py:97-104 downloads it; here it is a path).  The encoder is
    loaded too when the file holds encoder and quantizer keys; a decoder-only file gives a decode-only codec."""
    raw = _read_weight_file(path)
    dec = DacDecoder(precision=precision)
    dec.load_state_dict(decoder_state_dict(raw))
    enc = None
    if _has_encoder(raw):
        enc = DacEncoder(precision=precision)
        enc.load_state_dict(encoder_state_dict(raw))
        enc = enc.to(device)
    return DacCodec(dec.to(device), enc)


# ---- per-kernel entry points (tests) -----------------------------------------------------------------------------------
def pack_weight(kind: int, w: np.ndarray, cin: int, cout: int, k_or_stride: int) -> np.ndarray:
    """torch-layout fp32 weight -> [N, taps, cin] (jat_dac_pack_weight; kind 0 Conv1d, 1 ConvTranspose1d, 2 strided
    Conv1d over super-rows: [cout, 3, s * cin])."""
    w = np.ascontiguousarray(w, dtype=np.float32)
    if kind == 2:
        return _pack2(w, cin, cout, k_or_stride)
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


def _pack2(w, cin, cout, s):
    out = np.empty((cout, 3, s * cin), np.float32)
    _check(L.lib().jat_dac_pack_weight(2, w.ctypes.data, cin, cout, s, out.ctypes.data))
    return out


def head(audio: torch.Tensor, w, bias, alpha=None, out32=True, precision="bf16x3"):
    """jat_k_dac_head: audio fp32 [B, L] (CUDA) -> (out32 [B*L, C] or None, snake planes or None)."""
    audio = audio.contiguous()
    B, n = audio.shape
    Cc = w.shape[0]
    dev = audio.device
    o32 = torch.empty(B * n, Cc, dtype=torch.float32, device=dev) if out32 else None
    o_hi = o_lo = None
    if alpha is not None:
        o_hi = torch.empty(B * n, Cc, dtype=torch.int16, device=dev)
        o_lo = torch.empty_like(o_hi) if precision == "bf16x3" else None
    _check(L.lib().jat_k_dac_head(L.ptr(audio), L.ptr(w), L.ptr(bias), L.ptr(alpha), L.ptr(o32), L.ptr(o_hi), L.ptr(o_lo),
                                  B, n, Cc, L.stream_ptr()))
    return o32, (None if o_hi is None else (o_hi, o_lo))


def rvq(hidden_cl: torch.Tensor, sd: dict, B: int, T: int, n_q: int = 9, hidden_size: int = 1024):
    """jat_k_dac_rvq on channels-last fp32 hidden [B*T, hidden_size] with the quantizer parameters of `sd` (DacModel names,
    torch tensors on the device) -> (z [B, H, T], codes int32 [B, n_q, T], latents [B, 8 n_q, T], hidden [B, H, T])."""
    dev = hidden_cl.device
    stack = lambda k: torch.stack([sd[f"quantizer.quantizers.{i}.{k}"].reshape(-1) for i in range(n_q)]).to(dev).contiguous()
    w_in, b_in, cb, w_out, b_out = (stack(k) for k in ("in_proj.weight", "in_proj.bias", "codebook.weight",
                                                      "out_proj.weight", "out_proj.bias"))
    z = torch.empty(B, 1024, T, dtype=torch.float32, device=dev)
    codes = torch.empty(B, n_q, T, dtype=torch.int32, device=dev)
    lat = torch.empty(B, 8 * n_q, T, dtype=torch.float32, device=dev)
    hid = torch.empty(B, 1024, T, dtype=torch.float32, device=dev)
    _check(L.lib().jat_k_dac_rvq(L.ptr(hidden_cl.contiguous()), L.ptr(w_in), L.ptr(b_in), L.ptr(cb), L.ptr(w_out),
                                 L.ptr(b_out), L.ptr(z), L.ptr(codes), L.ptr(lat), L.ptr(hid), B, T, hidden_size, n_q,
                                 L.stream_ptr()))
    return z, codes, lat, hid
