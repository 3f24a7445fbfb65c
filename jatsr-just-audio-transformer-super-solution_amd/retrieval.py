"""Latent feature retrieval — the first item of the reference's roadmap (DOCs/future_work.md): a bank of high-resolution
training latent frames, an exact nearest-neighbour lookup per generated frame (what `faiss.IndexFlatL2`, k = 1, returns) and
the RVC-style blend  enhanced = (1 - index_rate) * pred_hr + index_rate * retrieved.

The bank lives on the GPU as fp16 rows of normalised frames (csrc/retrieval.hip: pack, search, blend; C ABI `jat_bank_*` in
include/jat_hip.h).  `key="hr"` looks a frame up by its own (generated) content, `key="lr"` by the LR input at that position
(the roadmap's `search_by_lr`); the blended-in value is the HR frame either way.

    python -m jatsr_amd.retrieval build --data-dir data_processed --out bank.pt --max-frames 100000
    python -m jatsr_amd.infer ... --index-bank bank.pt --index-rate 0.4
    python -m jatsr_amd.infer ... --index-bank bank.pt --index-rate 0.4 --index-k 8

`--index-k K` (`search_topk`, `blend_topk`, `retrieve(k=K)`) mixes in the inverse-square-distance weighted mean of
the K nearest frames, 1 <= K <= 8, as RVC's index does with K = 8, instead of the single nearest one: the retrieved track then
varies continuously with the query instead of jumping where the arg-min changes.

Multi-scale retrieval (`MultiScaleBank`; the roadmap's `MultiScaleFeatureBank`): one bank per time scale s in
{1, 2, 4, 8} whose rows are the mean of s consecutive normalised frames.  The prediction is pooled to each scale, looked up with
the same search and blend, brought back to the frame rate by linear interpolation and the scales' tracks are mixed in with
weights that sum to 1, at the one index rate: a coarse lookup sees 23, 46 or 93 ms of context instead of 11.6 ms.

    python -m jatsr_amd.retrieval build --data-dir data_processed --out bank_ms.pt --max-frames 100000 --scales 1,2,4
    python -m jatsr_amd.infer ... --index-bank bank_ms.pt --index-rate 0.4 [--index-scale-weights 2,1,1]

k-means compaction (`kmeans`, `--clusters K`; what RVC's index training does with a large feature set): a pool of
up to 2^22 frames is clustered on the GPU and the K centroids are stored as the bank, a bank file of the existing format:

    python -m jatsr_amd.retrieval build --data-dir data_processed --out bank_km.pt --clusters 10000 [--pool-frames 1000000]

IVF index (`IVFBank`, `--ivf`; the `IVF{n},Flat` index RVC trains and searches with nprobe = 1): the rows are grouped
by their nearest of n k-means centroids and a search scans only the lists of the `nprobe` centroids nearest to the query, so its
cost no longer grows with the bank.  Within the probed lists the result is the exact search's, bit for bit; outside them a
nearer row can be missed.  The bank file gets format 3; a multi-scale IVF is out of scope.

    python -m jatsr_amd.retrieval build --data-dir data_processed --out bank_ivf.pt --max-frames 1000000 --ivf [--ivf-lists N] [--ivf-nprobe P]
    python -m jatsr_amd.infer ... --index-bank bank_ivf.pt --index-rate 0.4 [--index-nprobe 8]

Voicing-aware index rates (`f0_classes`, `rate_track`, `mix_rates`): the index rate as a per-frame track derived
from a pitch track, in the place of one scalar.  Unvoiced frames get `index_rate * protect` (RVC's `protect`: consonants and
breaths keep more of the prediction), voiced frames whose F0 is not steady `index_rate * unstable`, steady ones `index_rate`.
Every `retrieve` takes such a track as `index_rate`.

    python -m jatsr_amd.infer ... --index-bank bank.pt --index-rate 0.4 --index-protect 0.33 [--index-unstable 0.7] [--index-smooth 2]

Whether retrieval improves audio quality is not established here: nothing in this repository was run with trained weights.
"""
from __future__ import annotations

import argparse
import ctypes as C
import glob
import os

import torch

from . import _lib as L

STAT_KEYS = ("hr_mean", "hr_std", "lr_mean", "lr_std")
FORMAT = 1            # a single bank
FORMAT_MS = 2         # a multi-scale bank: one single-bank dictionary per scale
FORMAT_IVF = 3        # an IVF index: a single-bank dictionary (rows grouped by list), the centroid keys, offsets, order, nprobe


def frame_plan(lengths, max_frames):
    """Which frames of each file enter a bank of at most `max_frames` rows -> [(first, stride, count)] per file.

    One global stride s = ceil(total / max_frames); file f contributes the frames whose position in the concatenation of all
    files is a multiple of s.  So sum(count) = ceil(total / s) <= max_frames, and the plan depends on the lengths alone."""
    lengths = [int(n) for n in lengths]
    max_frames = int(max_frames)
    if max_frames < 1:
        raise ValueError(f"max_frames {max_frames} must be at least 1")
    if any(n < 0 for n in lengths):
        raise ValueError("negative file length")
    total = sum(lengths)
    s = max(1, -(-total // max_frames))
    plan, offset = [], 0
    for n in lengths:
        first = (-offset) % s
        plan.append((first, s, 0 if first >= n else (n - 1 - first) // s + 1))
        offset += n
    return plan


def check_index_rate(index_rate):
    """The index rate as a float in [0, 1]; ValueError otherwise (a NaN is outside)."""
    r = float(index_rate)
    if not 0.0 <= r <= 1.0:
        raise ValueError(f"index_rate {index_rate!r} outside [0, 1]")
    return r


def index_rate_arg(text):
    """argparse type of --index-rate."""
    try:
        return check_index_rate(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


def check_index_k(index_k):
    """The number of nearest frames as an int in 1..8 (JAT_BANK_MAX_K); ValueError otherwise."""
    try:
        k = int(index_k)
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"index_k {index_k!r} outside 1..{L.BANK_MAX_K}")
    if k != index_k or isinstance(index_k, bool) or not 1 <= k <= L.BANK_MAX_K:
        raise ValueError(f"index_k {index_k!r} outside 1..{L.BANK_MAX_K}")
    return k


def index_k_arg(text):
    """argparse type of --index-k."""
    try:
        return check_index_k(int(text))
    except ValueError:
        raise argparse.ArgumentTypeError(f"index_k {text!r} outside 1..{L.BANK_MAX_K}")


def check_dist2_floor(dist2_floor):
    """The distance floor of the top-k blend as a positive finite float; ValueError otherwise (a NaN is not positive)."""
    f = C.c_float(float(dist2_floor)).value          # as the fp32 the kernel gets
    if not 0.0 < f < float("inf"):
        raise ValueError(f"dist2_floor {dist2_floor!r} must be positive and finite")
    return f


def check_scales(scales):
    """The time scales of a multi-scale bank as a tuple: 1 to 4 of 1, 2, 4, 8, strictly ascending.  Takes a sequence of ints or
    text such as "1,2,4"; ValueError otherwise."""
    try:
        if isinstance(scales, str):
            scales = [int(v) for v in scales.split(",")]
        out = tuple(scales)
    except (TypeError, ValueError):
        raise ValueError(f"scales {scales!r}: expected 1 to {L.BANK_MAX_SCALES} of {L.BANK_SCALES}, ascending")
    if not 1 <= len(out) <= L.BANK_MAX_SCALES:
        raise ValueError(f"scales {scales!r}: expected 1 to {L.BANK_MAX_SCALES} of them")
    for v in out:
        if isinstance(v, bool) or not isinstance(v, int) or v not in L.BANK_SCALES:
            raise ValueError(f"scales {scales!r}: {v!r} is not one of {L.BANK_SCALES}")
    if any(b <= a for a, b in zip(out, out[1:])):
        raise ValueError(f"scales {scales!r} must ascend strictly")
    return out


def scales_arg(text):
    """argparse type of --scales."""
    try:
        return check_scales(str(text))
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


def check_scale_weights(weights, n):
    """The n scale weights the mix runs with: positive finite numbers, normalised in fp64 to sum 1, each then rounded to fp32
    (returned as Python floats holding those fp32 values).  None: all equal.  n = 1 gives exactly 1.0.  Takes a sequence or
    text such as "2,1,1"; ValueError otherwise."""
    n = int(n)
    if weights is None:
        weights = [1.0] * n
    try:
        if isinstance(weights, str):
            weights = weights.split(",")
        w = [float(v) for v in weights]
    except (TypeError, ValueError):
        raise ValueError(f"scale weights {weights!r}: expected {n} positive numbers")
    if len(w) != n:
        raise ValueError(f"scale weights {weights!r}: {len(w)} of them for {n} scales")
    if not all(0.0 < v < float("inf") for v in w):
        raise ValueError(f"scale weights {weights!r} must be positive and finite")
    total = sum(w)
    out = tuple(C.c_float(v / total).value for v in w)
    if not all(0.0 < v < float("inf") for v in out) or not 0.0 < total < float("inf"):
        raise ValueError(f"scale weights {weights!r} must be positive and finite after normalisation in fp32")
    return out


def scale_weights_arg(text):
    """argparse type of --index-scale-weights and --scale-weights: the raw numbers; they are normalised against the bank."""
    try:
        w = [float(v) for v in str(text).split(",")]
        check_scale_weights(w, len(w))
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))
    return w


def _stats_cpu(stats, channels):
    out = {}
    for k in STAT_KEYS:
        if k not in stats:
            raise KeyError(f"statistics lack {k!r}")
        v = torch.as_tensor(stats[k]).detach().to("cpu", torch.float32).reshape(-1).clone()
        if v.numel() != channels:
            raise ValueError(f"{k} has {v.numel()} entries, expected {channels}")
        out[k] = v
    return out


def pack_state(keys, values, key, stats):
    """The dictionary a bank file holds: fp16 rows [N, C] (`values` None unless key == "lr"), the key kind, the channel count
    and the statistics the rows were normalised with.  Host code on CPU tensors."""
    if key not in ("hr", "lr"):
        raise ValueError(f"key {key!r} must be 'hr' or 'lr'")
    if keys.dim() != 2 or keys.dtype != torch.float16:
        raise ValueError(f"keys must be fp16 [N, C], got {keys.dtype} {tuple(keys.shape)}")
    if (values is not None) != (key == "lr"):
        raise ValueError("values are stored exactly when key == 'lr'")
    if values is not None and (values.shape != keys.shape or values.dtype != torch.float16):
        raise ValueError(f"values {values.dtype} {tuple(values.shape)} do not match keys {tuple(keys.shape)}")
    channels = int(keys.shape[1])
    return {"format": FORMAT, "keys": keys.detach().cpu().contiguous(),
            "values": None if values is None else values.detach().cpu().contiguous(), "key": key, "channels": channels,
            "stats": _stats_cpu(stats, channels)}


def unpack_state(d):
    """Validate a bank dictionary -> (keys, values, key, channels, stats)."""
    if isinstance(d, dict) and d.get("format") == FORMAT_MS:
        raise ValueError("this is a multi-scale bank (format 2), not a single bank: load it with retrieval.load_bank")
    if isinstance(d, dict) and d.get("format") == FORMAT_IVF:
        raise ValueError("this is an IVF index (format 3), not a single bank: load it with retrieval.load_bank")
    for k in ("keys", "values", "key", "channels", "stats"):
        if k not in d:
            raise KeyError(f"bank file lacks {k!r} (keys: {sorted(d.keys())})")
    st = pack_state(d["keys"], d["values"], d["key"], d["stats"])
    if st["channels"] != int(d["channels"]):
        raise ValueError(f"bank file: channels {d['channels']} but rows of {st['channels']}")
    if st["keys"].shape[0] < 1:
        raise ValueError("bank file holds no rows")
    return st["keys"], st["values"], st["key"], st["channels"], st["stats"]


def same_stats(a, b):
    """Whether two statistics dictionaries hold the same fp32 values."""
    return all(torch.equal(torch.as_tensor(a[k]).detach().to("cpu", torch.float32).reshape(-1),
                           torch.as_tensor(b[k]).detach().to("cpu", torch.float32).reshape(-1)) for k in STAT_KEYS)


class LatentBank:
    """A GPU-resident bank of normalised fp16 latent frames with exact nearest-neighbour search and index-rate blend."""

    def __init__(self, channels, capacity, key="hr", device="cuda"):
        if key not in ("hr", "lr"):
            raise ValueError(f"key {key!r} must be 'hr' or 'lr'")
        L.require_gpu()
        self.channels, self.capacity, self.key = int(channels), int(capacity), key
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.stats = None          # CPU fp32 copies of the statistics the rows were normalised with
        self._dev_stats = None
        self._work = None
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            L.check(L.lib().jat_bank_create(self.channels, self.capacity, 1 if key == "lr" else 0, C.byref(self._h)))

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                L.lib().jat_bank_destroy(h)
            except Exception:
                pass

    def __len__(self):
        n = C.c_int32()
        L.check(L.lib().jat_bank_size(self._h, C.byref(n)))
        return n.value

    def clear(self):
        L.check(L.lib().jat_bank_clear(self._h))

    # ---- statistics -----------------------------------------------------------------------------------------------------
    def _set_stats(self, stats):
        st = _stats_cpu(stats, self.channels)
        if self.stats is None:
            self.stats = st
            self._dev_stats = {k: v.to(self.device) for k, v in st.items()}
        elif not same_stats(self.stats, st):
            raise ValueError("the bank's rows were normalised with other statistics than the ones given")

    def check_stats(self, stats):
        """ValueError unless `stats` are the statistics this bank was built with."""
        if self.stats is None:
            raise ValueError("the bank holds no statistics yet (nothing was added)")
        if not same_stats(self.stats, _stats_cpu(stats, self.channels)):
            raise ValueError("the bank's rows were normalised with other statistics than the ones given")

    def _vec(self, v):
        if v is None:
            return None
        v = torch.as_tensor(v).to(self.device, torch.float32).contiguous().view(-1)
        if v.numel() != self.channels:
            raise ValueError(f"statistics vector of {v.numel()} entries, expected {self.channels}")
        return v

    # ---- building -------------------------------------------------------------------------------------------------------
    def add(self, hr_latent, stats, lr_latent=None, first=0, stride=1, count=None, window=1):
        """Append frames first, first + stride, ... (`count` of them; default: to the end) of a [C, len] latent array,
        fp16 or fp32, normalised with `stats`.  key == "lr" needs the LR array of the same shape: its frames are the keys.
        window in (2, 4, 8): each row is the mean of the `window` normalised frames that start there, fewer at the end of the
        array (`jat_bank_add_pooled`, what a `MultiScaleBank` holds at that scale); window = 1 makes the call it always made."""
        if window not in L.BANK_SCALES or isinstance(window, bool):
            raise ValueError(f"window {window!r} is not one of {L.BANK_SCALES}")
        self._set_stats(stats)
        if (lr_latent is not None) != (self.key == "lr"):
            raise ValueError("lr_latent is given exactly when the bank's key is 'lr'")
        if hr_latent.dim() != 2 or hr_latent.shape[0] != self.channels:
            raise ValueError(f"latent {tuple(hr_latent.shape)}, expected [{self.channels}, len]")
        if lr_latent is not None and lr_latent.shape != hr_latent.shape:
            raise ValueError(f"lr_latent {tuple(lr_latent.shape)} does not match hr_latent {tuple(hr_latent.shape)}")
        n = int(hr_latent.shape[1])
        first, stride = int(first), int(stride)
        if count is None:
            count = 0 if first >= n or stride < 1 else (n - 1 - first) // stride + 1
        dt = torch.float16 if hr_latent.dtype == torch.float16 else torch.float32
        hr = hr_latent.to(self.device, dt).contiguous()
        lr = None if lr_latent is None else lr_latent.to(self.device, dt).contiguous()
        s = self._dev_stats
        with torch.cuda.device(self.device):
            if self.key == "lr":
                src = (L.ptr(lr), L.ptr(hr), int(dt == torch.float16), n, first, stride, int(count))
                st = (L.ptr(s["lr_mean"]), L.ptr(s["lr_std"]), L.ptr(s["hr_mean"]), L.ptr(s["hr_std"]), L.stream_ptr())
            else:
                src = (L.ptr(hr), None, int(dt == torch.float16), n, first, stride, int(count))
                st = (L.ptr(s["hr_mean"]), L.ptr(s["hr_std"]), None, None, L.stream_ptr())
            if window == 1:
                rc = L.lib().jat_bank_add(self._h, *src, *st)
            else:
                rc = L.lib().jat_bank_add_pooled(self._h, *src, int(window), *st)
        L.check(rc)
        hr.record_stream(torch.cuda.current_stream(self.device))
        if lr is not None:
            lr.record_stream(torch.cuda.current_stream(self.device))
        return int(count)

    def rows(self, which="keys", full=False):
        """The stored fp16 rows as a tensor VIEW of the bank's memory ([size, C]; full: all `capacity` rows) and, for the
        keys, the fp32 norms.  `which`: "keys" or "values"."""
        p, q = C.c_void_p(), C.c_void_p()
        L.check(L.lib().jat_bank_rows(self._h, L.BANK_KEYS if which == "keys" else L.BANK_VALUES, C.byref(p), C.byref(q)))
        n = self.capacity if full else len(self)
        rows = _device_view(p.value, (n, self.channels), torch.float16, self.device, self)
        norms = _device_view(q.value, (n,), torch.float32, self.device, self) if q.value else None
        return rows, norms

    def load_rows(self, keys, values=None):
        """Append ready fp16 rows [N, C] (values exactly when key == "lr"); the norms are recomputed on the device."""
        keys = keys.to(self.device, torch.float16).contiguous()
        values = None if values is None else values.to(self.device, torch.float16).contiguous()
        if keys.dim() != 2 or keys.shape[1] != self.channels or (values is not None and values.shape != keys.shape):
            raise ValueError(f"rows {tuple(keys.shape)}, expected [N, {self.channels}]")
        with torch.cuda.device(self.device):
            L.check(L.lib().jat_bank_load_rows(self._h, L.ptr(keys), L.ptr(values), int(keys.shape[0]), L.stream_ptr()))
        keys.record_stream(torch.cuda.current_stream(self.device))
        if values is not None:
            values.record_stream(torch.cuda.current_stream(self.device))

    # ---- use ------------------------------------------------------------------------------------------------------------
    def _x(self, x, name="x"):
        if x.dim() != 3 or x.shape[1] != self.channels or x.dtype != torch.float32 or not x.is_cuda:
            raise ValueError(f"{name}: expected a CUDA fp32 [B, {self.channels}, T] tensor, got {x.dtype} {tuple(x.shape)}")
        return x.contiguous()

    def workspace_bytes(self, n_queries):
        n = C.c_size_t()
        L.check(L.lib().jat_bank_search_workspace_bytes(self._h, int(n_queries), C.byref(n)))
        return n.value

    def search(self, x, mean=None, std=None):
        """x fp32 [B, C, T] (normalised, or un-normalised with the key statistics given) -> (idx int32 [B, T], dist2 fp32
        [B, T]): the nearest key row of every frame, the lowest index on equal distance, and its squared distance."""
        x = self._x(x)
        B, _, T = x.shape
        if B < 1 or T < 1:
            raise ValueError(f"x {tuple(x.shape)}: B and T must be positive")
        need = self.workspace_bytes(B * T)
        if self._work is None or self._work.numel() < need:
            self._work = torch.empty(need, dtype=torch.uint8, device=self.device)
        idx = torch.empty(B, T, dtype=torch.int32, device=self.device)
        dist2 = torch.empty(B, T, dtype=torch.float32, device=self.device)
        mean, std = self._vec(mean), self._vec(std)
        with torch.cuda.device(self.device):
            L.check(L.lib().jat_bank_search(self._h, L.ptr(x), L.ptr(mean), L.ptr(std), B, T, L.ptr(idx), L.ptr(dist2),
                                            L.ptr(self._work), self._work.numel(), L.stream_ptr()))
        return idx, dist2

    def blend(self, x, idx, index_rate, mean=None, std=None, out=None):
        """(1 - index_rate) * x + index_rate * value[idx]; with the value statistics the value is de-normalised first.
        out: where to write ([B, C, T] fp32 contiguous; may be x)."""
        r = check_index_rate(index_rate)
        if out is None:
            x = self._x(x)
            out = torch.empty_like(x)
        else:
            if not x.is_contiguous() or not out.is_contiguous() or out.shape != x.shape or out.dtype != torch.float32:
                raise ValueError("blend(out=...): x and out must be contiguous fp32 tensors of one shape")
            x = self._x(x)
        B, _, T = x.shape
        if idx.shape != (B, T) or idx.dtype != torch.int32 or not idx.is_cuda:
            raise ValueError(f"idx: expected CUDA int32 [{B}, {T}], got {idx.dtype} {tuple(idx.shape)}")
        idx = idx.contiguous()
        mean, std = self._vec(mean), self._vec(std)
        with torch.cuda.device(self.device):
            L.check(L.lib().jat_bank_blend(self._h, L.ptr(x), L.ptr(idx), L.ptr(mean), L.ptr(std), r, L.ptr(out), B, T,
                                           L.stream_ptr()))
        return out

    def topk_workspace_bytes(self, n_queries, k):
        n = C.c_size_t()
        L.check(L.lib().jat_bank_topk_workspace_bytes(self._h, int(n_queries), int(k), C.byref(n)))
        return n.value

    def search_topk(self, x, k, mean=None, std=None):
        """The k nearest key rows of every frame, 1 <= k <= 8, ordered by (distance, index) -> (idx int32 [B, T, k], dist2
        fp32 [B, T, k]).  A bank of fewer than k rows fills the tail with idx -1 and dist2 +inf.  The first j columns are
        the result for k = j, and k = 1 is `search`."""
        k = check_index_k(k)
        x = self._x(x)
        B, _, T = x.shape
        if B < 1 or T < 1:
            raise ValueError(f"x {tuple(x.shape)}: B and T must be positive")
        need = self.topk_workspace_bytes(B * T, k)
        if self._work is None or self._work.numel() < need:
            self._work = torch.empty(need, dtype=torch.uint8, device=self.device)
        idx = torch.empty(B, T, k, dtype=torch.int32, device=self.device)
        dist2 = torch.empty(B, T, k, dtype=torch.float32, device=self.device)
        mean, std = self._vec(mean), self._vec(std)
        with torch.cuda.device(self.device):
            L.check(L.lib().jat_bank_search_topk(self._h, L.ptr(x), L.ptr(mean), L.ptr(std), B, T, k, L.ptr(idx), L.ptr(dist2),
                                                 L.ptr(self._work), self._work.numel(), L.stream_ptr()))
        return idx, dist2

    def blend_topk(self, x, idx, dist2, index_rate, mean=None, std=None, out=None, dist2_floor=1e-6):
        """(1 - index_rate) * x + index_rate * v with v the inverse-square-distance weighted mean of the k value rows idx
        [B, T, k] names: weights (max(dist2_0, floor) / max(dist2_j, floor))^2 normalised to sum 1 — RVC's square(1 / score)
        wherever the distances exceed the floor; entries with idx < 0 carry no weight.  With the value statistics v is
        de-normalised first.  out: where to write ([B, C, T] fp32 contiguous; may be x)."""
        r = check_index_rate(index_rate)
        floor = check_dist2_floor(dist2_floor)
        if out is None:
            x = self._x(x)
            out = torch.empty_like(x)
        else:
            if not x.is_contiguous() or not out.is_contiguous() or out.shape != x.shape or out.dtype != torch.float32:
                raise ValueError("blend_topk(out=...): x and out must be contiguous fp32 tensors of one shape")
            x = self._x(x)
        B, _, T = x.shape
        if idx.dim() != 3 or idx.shape[:2] != (B, T) or idx.dtype != torch.int32 or not idx.is_cuda:
            raise ValueError(f"idx: expected CUDA int32 [{B}, {T}, k], got {idx.dtype} {tuple(idx.shape)}")
        k = check_index_k(int(idx.shape[2]))
        if dist2.shape != idx.shape or dist2.dtype != torch.float32 or not dist2.is_cuda:
            raise ValueError(f"dist2: expected CUDA fp32 {tuple(idx.shape)}, got {dist2.dtype} {tuple(dist2.shape)}")
        idx, dist2 = idx.contiguous(), dist2.contiguous()
        mean, std = self._vec(mean), self._vec(std)
        with torch.cuda.device(self.device):
            L.check(L.lib().jat_bank_blend_topk(self._h, L.ptr(x), L.ptr(idx), L.ptr(dist2), k, L.ptr(mean), L.ptr(std), r,
                                                floor, L.ptr(out), B, T, L.stream_ptr()))
        return out

    def retrieve(self, x, index_rate, stats=None, query=None, k=1, dist2_floor=1e-6, neighbours=False):
        """Search + blend on a de-normalised HR latent x [B, C, T].  The query is x under the HR statistics (key == "hr") or
        `query`, the un-normalised LR latent of the same shape, under the LR statistics (key == "lr"); the retrieved HR
        frame is de-normalised in the blend.  stats: must be the statistics the bank was built with (default: those).
        k > 1: the inverse-square-distance weighted mean of the k nearest frames (`search_topk`, `blend_topk`) takes the
        place of the single nearest one; k = 1 makes exactly the calls it always made.  neighbours: return (y, idx, dist2)
        with the lists the blend used.  index_rate may be a per-frame track, an fp32 tensor [B, T] (or [T] for B = 1) on the
        bank's device with values in [0, 1] (`rate_track`): this call at rate 1.0, then `mix_rates`."""
        if is_rate_track(index_rate):
            return _retrieve_with_track(self, x, index_rate, neighbours=neighbours, stats=stats, query=query, k=k,
                                        dist2_floor=dist2_floor)
        check_index_rate(index_rate)
        k = check_index_k(k)
        check_dist2_floor(dist2_floor)
        if stats is not None:
            self.check_stats(stats)
        elif self.stats is None:
            raise ValueError("the bank holds no statistics yet (nothing was added)")
        s = self._dev_stats
        if self.key == "lr":
            if query is None:
                raise ValueError("a bank keyed by LR frames needs the LR latent as `query`")
            if query.shape != x.shape:
                raise ValueError(f"query {tuple(query.shape)} does not match x {tuple(x.shape)}")
            q, mean, std = query.to(self.device, torch.float32), s["lr_mean"], s["lr_std"]
        else:
            q, mean, std = x, s["hr_mean"], s["hr_std"]
        if k == 1:
            idx, dist2 = self.search(q, mean, std)
            y = self.blend(x, idx, index_rate, s["hr_mean"], s["hr_std"])
        else:
            idx, dist2 = self.search_topk(q, k, mean, std)
            y = self.blend_topk(x, idx, dist2, index_rate, s["hr_mean"], s["hr_std"], dist2_floor=dist2_floor)
        return (y, idx, dist2) if neighbours else y

    # ---- k-means compaction (C ABI: include/jat_hip_km.h) --------------------------------------------------------
    def assign(self, pool, first=0, count=None, idx=None, changed=None):
        """`self` holds the centroids: the nearest centroid of pool rows first .. first + count - 1 (default: to the end of
        the pool) -> (idx int32 [count], dist2 fp32 [count]), the lowest index on equal distance.  idx: the buffer to
        overwrite (default: a fresh one filled with -1); changed: an int32 tensor of one element that is incremented by the
        number of entries of idx that differ from what the buffer held."""
        if not isinstance(pool, LatentBank):
            raise ValueError("assign: the pool is a LatentBank")
        first = int(first)
        count = len(pool) - first if count is None else int(count)
        if count < 1 or first < 0:
            raise ValueError(f"assign: rows {first} .. +{count} of a pool of {len(pool)}")
        if idx is None:
            idx = torch.full((count,), -1, dtype=torch.int32, device=self.device)
        elif idx.shape != (count,) or idx.dtype != torch.int32 or idx.device != self.device or not idx.is_contiguous():
            raise ValueError(f"idx: expected a contiguous int32 [{count}] tensor on {self.device}")
        if changed is not None and (changed.numel() != 1 or changed.dtype != torch.int32 or changed.device != self.device):
            raise ValueError(f"changed: expected an int32 tensor of one element on {self.device}")
        dist2 = torch.empty(count, dtype=torch.float32, device=self.device)
        need = C.c_size_t()
        L.check(L.lib().jat_bank_assign_workspace_bytes(pool._h, self._h, count, C.byref(need)))
        if self._work is None or self._work.numel() < need.value:
            self._work = torch.empty(need.value, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            L.check(L.lib().jat_bank_assign(pool._h, first, count, self._h, L.ptr(idx), L.ptr(dist2), L.ptr(changed),
                                            L.ptr(self._work), self._work.numel(), L.stream_ptr()))
        return idx, dist2

    def cluster_update(self, pool, idx, check=True):
        """`self` holds the centroids: every centroid with members moves to the mean of the pool rows idx [N] assigns to it
        (exact integer sums, one rounding per conversion; an empty cluster keeps its row) -> counts int32 [K].  An idx entry
        outside [0, K) is skipped on the device; check: wait for the counts and raise ValueError unless they sum to N."""
        N, K = len(pool), len(self)
        if idx.shape != (N,) or idx.dtype != torch.int32 or idx.device != self.device or not idx.is_contiguous():
            raise ValueError(f"idx: expected a contiguous int32 [{N}] tensor on {self.device}")
        counts = torch.empty(max(K, 1), dtype=torch.int32, device=self.device)
        need = C.c_size_t()
        L.check(L.lib().jat_bank_cluster_update_workspace_bytes(pool._h, K, C.byref(need)))
        work = torch.empty(need.value, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            L.check(L.lib().jat_bank_cluster_update(pool._h, L.ptr(idx), self._h, L.ptr(counts), L.ptr(work), work.numel(),
                                                    L.stream_ptr()))
        work.record_stream(torch.cuda.current_stream(self.device))
        if check and int(counts.sum()) != N:
            raise ValueError(f"cluster_update: {N - int(counts.sum())} entries of idx lie outside [0, {K}); they were skipped")
        return counts

    # ---- files ----------------------------------------------------------------------------------------------------------
    def state(self):
        keys, _ = self.rows("keys")
        values = self.rows("values")[0] if self.key == "lr" else None
        if self.stats is None:
            raise ValueError("an empty bank cannot be saved")
        return pack_state(keys.cpu(), None if values is None else values.cpu(), self.key, self.stats)

    def save(self, path):
        torch.save(self.state(), path)

    @classmethod
    def from_state(cls, d, device="cuda", capacity=None):
        keys, values, key, channels, stats = unpack_state(d)
        bank = cls(channels, max(int(keys.shape[0]), int(capacity or 0)), key=key, device=device)
        bank._set_stats(stats)
        bank.load_rows(keys, values)
        return bank

    @classmethod
    def load(cls, path, device="cuda"):
        return cls.from_state(torch.load(path, map_location="cpu", weights_only=False), device=device)

    @classmethod
    def from_data_dir(cls, data_dir, stats, split="train", max_frames=100_000, key="hr", device="cuda", clusters=None,
                      pool_frames=None, kmeans_iters=10):
        """A bank over the `split` of a prepared data set (`python -m jatsr_amd.prepare`): the frames `frame_plan` names,
        files in sorted order, one file uploaded at a time.  clusters=K: those frames (`pool_frames` of them at most, default
        min(total, 2^22); `max_frames` is not used) are only the pool, and the bank holds the centroids `kmeans` leaves
        (DESIGN §26); the report is kept as `bank.kmeans_report`."""
        if clusters is None:
            files, channels, plan = _plan_data_dir(data_dir, split, max_frames)
            return _fill_from_files(cls(channels, sum(c for _, _, c in plan), key=key, device=device), files, plan, stats)
        files, channels, plan = _plan_data_dir(data_dir, split, check_pool_frames(pool_frames))
        pool = _fill_from_files(cls(channels, sum(c for _, _, c in plan), key=key, device=device), files, plan, stats)
        bank, report = kmeans(pool, clusters, iters=kmeans_iters)
        bank.kmeans_report = report
        return bank


def _plan_data_dir(data_dir, split, max_frames):
    """The sorted latent files of a split, their channel count and the `frame_plan` over their lengths."""
    from .data import _load_fp16
    folder = os.path.join(str(data_dir), split)
    files = sorted(glob.glob(os.path.join(folder, "*.pt")))
    if not files:
        raise ValueError(f"No .pt files found in {folder}")
    lengths, channels = [], None
    for path in files:
        hr, _ = _load_fp16(path)
        if channels is None:
            channels = int(hr.shape[0])
        if hr.shape[0] != channels:
            raise ValueError(f"{path}: {hr.shape[0]} channels, the files before it have {channels}")
        lengths.append(int(hr.shape[1]))
    return files, channels, frame_plan(lengths, max_frames)


def _fill_from_files(bank, files, plan, stats):
    """`bank.add` of every file's planned frames (a LatentBank, or a MultiScaleBank: the same window starts at every scale)."""
    from .data import _load_fp16
    for path, (first, stride, count) in zip(files, plan):
        if count == 0:
            continue
        hr, lr = _load_fp16(path)
        bank.add(hr, stats, lr_latent=lr if bank.key == "lr" else None, first=first, stride=stride, count=count)
    return bank


# ---- multi-scale retrieval (C ABI: include/jat_hip_ms.h) ------------------------------------------------------------
def _frames(x, name="x"):
    if x.dim() != 3 or x.dtype != torch.float32 or not x.is_cuda or min(x.shape) < 1:
        raise ValueError(f"{name}: expected a CUDA fp32 [B, C, T] tensor, got {x.dtype} {tuple(x.shape)}")
    return x.contiguous()


def _stat_vec(v, channels, device):
    if v is None:
        return None
    v = torch.as_tensor(v).to(device, torch.float32).contiguous().view(-1)
    if v.numel() != channels:
        raise ValueError(f"statistics vector of {v.numel()} entries, expected {channels}")
    return v


def pooled_length(T, scale):
    """Frames of a [.., T] track pooled at `scale`: ceil(T / scale)."""
    return -(-int(T) // int(scale))


def pool_frames(x, scales, mean=None, std=None, outs=None):
    """x fp32 [B, C, T] -> one [B, C, ceil(T / s)] tensor per scale s of `scales` (each of 2, 4, 8, ascending), in ONE launch
    that reads x once: the mean of the s frames that start at t = 0, s, 2 s, ... (normalised first when mean / std are given;
    ascending sequential adds, one division; the last window of a row may hold fewer frames and divides by their number).
    outs: where to write (contiguous fp32 tensors of those shapes)."""
    x = _frames(x)
    scales = check_scales(scales)
    if scales[0] == 1:
        raise ValueError(f"scales {scales!r}: scale 1 is x itself and takes no buffer")
    B, Cc, T = x.shape
    if (mean is None) != (std is None):
        raise ValueError("mean and std are given together or not at all")
    mean, std = _stat_vec(mean, Cc, x.device), _stat_vec(std, Cc, x.device)
    if outs is None:
        outs = [torch.empty(B, Cc, pooled_length(T, s), dtype=torch.float32, device=x.device) for s in scales]
    outs = list(outs)
    for s, o in zip(scales, outs):
        if tuple(o.shape) != (B, Cc, pooled_length(T, s)) or o.dtype != torch.float32 or not o.is_contiguous() or o.device != x.device:
            raise ValueError(f"outs: scale {s} needs a contiguous fp32 [{B}, {Cc}, {pooled_length(T, s)}] tensor on {x.device}")
    if len(outs) != len(scales):
        raise ValueError(f"outs: {len(outs)} tensors for {len(scales)} scales")
    n = len(scales)
    with torch.cuda.device(x.device):
        L.check(L.lib().jat_bank_pool_frames(L.ptr(x), L.ptr(mean), L.ptr(std), B, Cc, T, n, (C.c_int32 * n)(*scales),
                                             (C.c_void_p * n)(*[o.data_ptr() for o in outs]), L.stream_ptr()))
    return outs


def mix_scales(x, scales, tracks, weights, index_rate, out=None):
    """(1 - index_rate) x + index_rate sum_i weights[i] u_i with u_i the track of scale scales[i] ([B, C, ceil(T / s)] fp32)
    brought to T frames by linear interpolation with half-pixel centres (F.interpolate(mode="linear", align_corners=False); a
    track of scale 1 is taken as it is).  weights are used as given (`check_scale_weights` makes them sum to 1).  out: where
    to write; may be x, may not be a track."""
    x = _frames(x)
    scales = check_scales(scales)
    r = check_index_rate(index_rate)
    B, Cc, T = x.shape
    tracks, w = [t for t in tracks], [float(v) for v in weights]
    n = len(scales)
    if len(tracks) != n or len(w) != n:
        raise ValueError(f"{len(tracks)} tracks and {len(w)} weights for {n} scales")
    if not all(0.0 < C.c_float(v).value < float("inf") for v in w):
        raise ValueError(f"scale weights {weights!r} must be positive and finite")
    for s, t in zip(scales, tracks):
        if tuple(t.shape) != (B, Cc, pooled_length(T, s)) or t.dtype != torch.float32 or not t.is_contiguous() or t.device != x.device:
            raise ValueError(f"tracks: scale {s} needs a contiguous fp32 [{B}, {Cc}, {pooled_length(T, s)}] tensor on {x.device}")
    if out is None:
        out = torch.empty_like(x)
    elif out.shape != x.shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != x.device:
        raise ValueError("mix_scales(out=...): out must be a contiguous fp32 tensor of x's shape")
    with torch.cuda.device(x.device):
        L.check(L.lib().jat_bank_mix_scales(L.ptr(x), n, (C.c_int32 * n)(*scales), (C.c_void_p * n)(*[t.data_ptr() for t in tracks]),
                                            (C.c_float * n)(*w), r, L.ptr(out), B, Cc, T, L.stream_ptr()))
    return out


def pack_ms_state(scales, weights, banks):
    """The dictionary a multi-scale bank file holds: format 2, the scales, the normalised fp32 weights and one single-bank
    dictionary (`pack_state`) per scale, all of one key kind, channel count, row count and set of statistics."""
    scales = check_scales(scales)
    weights = tuple(float(v) for v in weights)       # as `check_scale_weights` returned them: not normalised a second time
    if len(weights) != len(scales) or not all(0.0 < v < float("inf") and v == C.c_float(v).value for v in weights) or \
            abs(sum(weights) - 1.0) > 1e-6:
        raise ValueError(f"scale weights {weights!r}: expected {len(scales)} positive fp32 values that sum to 1")
    banks = [dict(b) for b in banks]
    if len(banks) != len(scales):
        raise ValueError(f"{len(banks)} banks for {len(scales)} scales")
    first = unpack_state(banks[0])
    for b in banks:
        keys, _, key, channels, stats = unpack_state(b)
        if (key, channels, int(keys.shape[0])) != (first[2], first[3], int(first[0].shape[0])) or not same_stats(stats, first[4]):
            raise ValueError("the banks of a multi-scale bank share key kind, channels, row count and statistics")
    return {"format": FORMAT_MS, "scales": list(scales), "weights": list(weights), "banks": banks}


def unpack_ms_state(d):
    """Validate a multi-scale bank dictionary -> (scales, weights, [single-bank dictionaries])."""
    if not isinstance(d, dict) or d.get("format") != FORMAT_MS:
        raise ValueError("not a multi-scale bank (format 2); a single bank loads with LatentBank.load or retrieval.load_bank")
    for k in ("scales", "weights", "banks"):
        if k not in d:
            raise KeyError(f"multi-scale bank file lacks {k!r} (keys: {sorted(d.keys())})")
    st = pack_ms_state(d["scales"], d["weights"], d["banks"])
    return tuple(st["scales"]), tuple(st["weights"]), st["banks"]


class MultiScaleBank:
    """One `LatentBank` per time scale (the roadmap's MultiScaleFeatureBank): the bank of scale s holds, for the same window
    starts, the mean of s consecutive normalised frames.  `retrieve` pools the prediction to each scale, looks it up with the
    single bank's search and blend, interpolates each retrieved track back to the frame rate and mixes
        y = (1 - index_rate) x + index_rate sum_i weights[i] u_i,        weights summing to 1.
    scales = (1,) is a `LatentBank`, bit for bit."""

    def __init__(self, channels, capacity, scales=(1, 2, 4), key="hr", weights=None, device="cuda"):
        self.scales = check_scales(scales)
        self.weights = check_scale_weights(weights, len(self.scales))
        self._adopt([LatentBank(channels, capacity, key=key, device=device) for _ in self.scales])

    def _adopt(self, banks):
        self.banks = list(banks)
        b = self.banks[0]
        self.channels, self.capacity, self.key, self.device = b.channels, b.capacity, b.key, b.device

    @staticmethod
    def roadmap_rate(r, n):
        """The index rate at which this family, with equal weights, is the roadmap's (x + r sum_s up_s) / (1 + n r)."""
        return n * r / (1.0 + n * r)

    @property
    def stats(self):
        return self.banks[0].stats

    def check_stats(self, stats):
        self.banks[0].check_stats(stats)

    def set_weights(self, weights):
        """Other scale weights (positive numbers, normalised to sum 1) than the ones the bank was built or loaded with."""
        self.weights = check_scale_weights(weights, len(self.scales))

    def __len__(self):
        """Rows per scale."""
        return len(self.banks[0])

    def clear(self):
        for b in self.banks:
            b.clear()

    def add(self, hr_latent, stats, lr_latent=None, first=0, stride=1, count=None):
        """`LatentBank.add` at every scale: the windows of scale s start at the same frames first, first + stride, ... and
        hold s frames (fewer at the end of the array).  The arrays are uploaded once."""
        dt = torch.float16 if hr_latent.dtype == torch.float16 else torch.float32
        hr = hr_latent.to(self.device, dt)
        lr = None if lr_latent is None else lr_latent.to(self.device, dt)
        n = 0
        for s, b in zip(self.scales, self.banks):
            n = b.add(hr, stats, lr_latent=lr, first=first, stride=stride, count=count, window=s)
        return n

    def retrieve(self, x, index_rate, stats=None, query=None, k=1, dist2_floor=1e-6, neighbours=False):
        """`LatentBank.retrieve` over every scale, on a de-normalised HR latent x [B, C, T]: one `pool_frames` launch pools the
        query (x under the HR statistics, or the LR latent `query` under the LR statistics for key == "lr") to the scales
        above 1; each scale's bank is searched (`search`, or `search_topk` for k > 1, the same k at every scale) and its
        de-normalised HR rows are written over that scale's pooled buffer by `blend` / `blend_topk` at rate 1; one `mix_scales`
        launch interpolates and mixes.  Nothing waits for the device.  neighbours: (y, [idx per scale], [dist2 per scale]).
        index_rate may be a per-frame track as in `LatentBank.retrieve` (its range check waits for the device)."""
        if is_rate_track(index_rate):
            return _retrieve_with_track(self, x, index_rate, neighbours=neighbours, stats=stats, query=query, k=k,
                                        dist2_floor=dist2_floor)
        r = check_index_rate(index_rate)
        k = check_index_k(k)
        check_dist2_floor(dist2_floor)
        if self.scales == (1,):                      # the single bank itself: the calls and the bits of LatentBank.retrieve
            out = self.banks[0].retrieve(x, r, stats=stats, query=query, k=k, dist2_floor=dist2_floor, neighbours=neighbours)
            return (out[0], [out[1]], [out[2]]) if neighbours else out
        if stats is not None:
            self.check_stats(stats)
        elif self.stats is None:
            raise ValueError("the bank holds no statistics yet (nothing was added)")
        s = self.banks[0]._dev_stats
        x = self.banks[0]._x(x)
        if self.key == "lr":
            if query is None:
                raise ValueError("a bank keyed by LR frames needs the LR latent as `query`")
            if query.shape != x.shape:
                raise ValueError(f"query {tuple(query.shape)} does not match x {tuple(x.shape)}")
            q, mean, std = self.banks[0]._x(query.to(self.device, torch.float32), "query"), s["lr_mean"], s["lr_std"]
        else:
            q, mean, std = x, s["hr_mean"], s["hr_std"]
        coarse = [v for v in self.scales if v > 1]
        pooled = dict(zip(coarse, pool_frames(q, coarse, mean, std)))
        tracks, idxs, dists = [], [], []
        for scale, bank in zip(self.scales, self.banks):
            # scale 1: the query with its statistics, as the single bank does, and a fresh track; above: the pooled, already
            # normalised query, and the track written over it (0 * pooled + 1 * v, the blend at rate 1)
            qs, m, sd, base, out = (q, mean, std, x, None) if scale == 1 else (pooled[scale], None, None, pooled[scale], pooled[scale])
            if k == 1:
                idx, dist2 = bank.search(qs, m, sd)
                tracks.append(bank.blend(base, idx, 1.0, s["hr_mean"], s["hr_std"], out=out))
            else:
                idx, dist2 = bank.search_topk(qs, k, m, sd)
                tracks.append(bank.blend_topk(base, idx, dist2, 1.0, s["hr_mean"], s["hr_std"], out=out, dist2_floor=dist2_floor))
            idxs.append(idx)
            dists.append(dist2)
        y = mix_scales(x, self.scales, tracks, self.weights, r)
        return (y, idxs, dists) if neighbours else y

    # ---- files ----------------------------------------------------------------------------------------------------------
    def state(self):
        return pack_ms_state(self.scales, self.weights, [b.state() for b in self.banks])

    def save(self, path):
        torch.save(self.state(), path)

    @classmethod
    def from_state(cls, d, device="cuda", capacity=None):
        scales, weights, banks = unpack_ms_state(d)
        self = cls.__new__(cls)
        self.scales, self.weights = scales, weights
        self._adopt([LatentBank.from_state(b, device=device, capacity=capacity) for b in banks])
        return self

    @classmethod
    def load(cls, path, device="cuda"):
        return cls.from_state(torch.load(path, map_location="cpu", weights_only=False), device=device)

    @classmethod
    def from_data_dir(cls, data_dir, stats, split="train", max_frames=100_000, key="hr", device="cuda", scales=(1, 2, 4),
                      weights=None, clusters=None, pool_frames=None, kmeans_iters=10):
        """`LatentBank.from_data_dir` at every scale: ONE `frame_plan` names the window starts of all scales.  clusters=K: the
        pooled rows of each scale are clustered on their own with the same K (`kmeans`).  The banks of a
        multi-scale file share their row count, so an empty cluster is NOT dropped here: it stays at the pool row it started
        from.  The reports are kept as `bank.kmeans_report`, one per scale."""
        if clusters is None:
            files, channels, plan = _plan_data_dir(data_dir, split, max_frames)
            bank = cls(channels, sum(c for _, _, c in plan), scales=scales, key=key, weights=weights, device=device)
            return _fill_from_files(bank, files, plan, stats)
        files, channels, plan = _plan_data_dir(data_dir, split, check_pool_frames(pool_frames))
        pool = cls(channels, sum(c for _, _, c in plan), scales=scales, key=key, weights=weights, device=device)
        _fill_from_files(pool, files, plan, stats)
        done = [kmeans(b, clusters, iters=kmeans_iters, drop_empty=False) for b in pool.banks]
        self = cls.__new__(cls)
        self.scales, self.weights = pool.scales, pool.weights
        self._adopt([b for b, _ in done])
        self.kmeans_report = [r for _, r in done]
        return self


def check_clusters(n_clusters):
    """The number of clusters as a positive int; ValueError otherwise."""
    if isinstance(n_clusters, bool) or not isinstance(n_clusters, int) or n_clusters < 1:
        raise ValueError(f"clusters {n_clusters!r} must be a positive integer")
    return n_clusters


def check_pool_frames(pool_frames):
    """The upper bound on the rows of a k-means pool: None is 2^22 (JAT_KM_MAX_POOL), else an int in 1..2^22."""
    if pool_frames is None:
        return L.KM_MAX_POOL
    if isinstance(pool_frames, bool) or not isinstance(pool_frames, int) or not 1 <= pool_frames <= L.KM_MAX_POOL:
        raise ValueError(f"pool_frames {pool_frames!r} outside 1..{L.KM_MAX_POOL}")
    return pool_frames


def seed_positions(n_rows, n_clusters):
    """The pool rows the centroids start from: i N // K for i < K, K distinct positions for K <= N."""
    return [i * int(n_rows) // int(n_clusters) for i in range(int(n_clusters))]


def sum_dist2(dist2):
    """The sum of an fp32 device tensor in fp64 in one fixed order (`jat_bank_sum_dist2`) -> a device tensor of one double."""
    if dist2.dtype != torch.float32 or not dist2.is_cuda or dist2.numel() < 1:
        raise ValueError(f"dist2: expected a non-empty CUDA fp32 tensor, got {dist2.dtype} {tuple(dist2.shape)}")
    dist2 = dist2.contiguous()
    out = torch.empty(1, dtype=torch.float64, device=dist2.device)
    with torch.cuda.device(dist2.device):
        L.check(L.lib().jat_bank_sum_dist2(L.ptr(dist2), dist2.numel(), L.ptr(out), L.stream_ptr()))
    return out


def _bank_of_rows(like, keys, values, capacity=None):
    bank = LatentBank(like.channels, capacity or int(keys.shape[0]), key=like.key, device=like.device)
    if like.stats is not None:
        bank._set_stats(like.stats)
    bank.load_rows(keys, values)
    return bank


def kmeans(pool, n_clusters, iters=10, drop_empty=True):
    """Lloyd's k-means over the rows of `pool` (a LatentBank of 1..2^22 rows) on the GPU -> (LatentBank of the centroids, report).

    The centroids start from pool rows i N // K; an iteration is `assign` (nearest centroid, the lowest index on equal
    distance) then `cluster_update` (every centroid to the exactly summed mean of its members; an empty cluster stays where it
    is).  It stops after `iters` iterations, or before the update of an iteration whose assignment changed nothing.  With
    drop_empty the clusters without members (duplicated seed rows end so) are left out, the rest in ascending order.  The
    result is an ordinary bank of the pool's key kind and statistics.  report: requested and kept K, N, iterations, the inertia
    (sum of squared distances, fp64) and the number of changed assignments per iteration, min / median / max cluster size."""
    if not isinstance(pool, LatentBank):
        raise ValueError("kmeans: the pool is a LatentBank")
    K, N = check_clusters(n_clusters), len(pool)
    if isinstance(iters, bool) or not isinstance(iters, int) or iters < 1:
        raise ValueError(f"iters {iters!r} must be a positive integer")
    if N > L.KM_MAX_POOL:
        raise ValueError(f"kmeans: a pool of {N} rows exceeds {L.KM_MAX_POOL}")
    if K > N:
        raise ValueError(f"kmeans: {K} clusters for a pool of {N} rows")
    paired = pool.key == "lr"
    seeds = torch.tensor(seed_positions(N, K), dtype=torch.int64, device=pool.device)
    cent = _bank_of_rows(pool, pool.rows("keys")[0][seeds], pool.rows("values")[0][seeds] if paired else None)
    idx = torch.full((N,), -1, dtype=torch.int32, device=pool.device)
    changed = torch.zeros(1, dtype=torch.int32, device=pool.device)
    inertia, moved, counts = [], [], None
    for _ in range(iters):
        changed.zero_()
        _, dist2 = cent.assign(pool, idx=idx, changed=changed)
        inertia.append(float(sum_dist2(dist2)))
        moved.append(int(changed))
        if moved[-1] == 0:
            break                       # the update of the same assignment is the one already made
        counts = cent.cluster_update(pool, idx)
    n = counts.cpu().tolist()
    keep = [i for i in range(K) if n[i] > 0] if drop_empty else list(range(K))
    if len(keep) < K:
        pick = torch.tensor(keep, dtype=torch.int64, device=pool.device)
        cent = _bank_of_rows(pool, cent.rows("keys")[0][pick], cent.rows("values")[0][pick] if paired else None)
    kept = sorted(n[i] for i in keep)
    report = {"clusters": K, "kept": len(keep), "rows": N, "iterations": len(moved), "inertia": inertia, "changed": moved,
              "size_min": kept[0], "size_median": kept[len(kept) // 2], "size_max": kept[-1]}
    return cent, report


# ---- IVF index (C ABI: include/jat_hip_ivf.h) ---------------------------------------------------------------------
def default_nlist(n_rows):
    """The number of lists RVC's index training uses for N rows, min(int(16 sqrt(N)), N // 39), floored at 1."""
    import math
    n = int(n_rows)
    if n < 1:
        raise ValueError(f"default_nlist: {n_rows!r} rows")
    return max(1, min(int(16 * math.sqrt(n)), n // 39))


def check_nprobe(nprobe):
    """The number of probed lists as an int in 1..8 (JAT_IVF_MAX_NPROBE); ValueError otherwise."""
    if isinstance(nprobe, bool) or not isinstance(nprobe, int) or not 1 <= nprobe <= L.IVF_MAX_NPROBE:
        raise ValueError(f"nprobe {nprobe!r} outside 1..{L.IVF_MAX_NPROBE}")
    return nprobe


def nprobe_arg(text):
    """argparse type of --ivf-nprobe and --index-nprobe."""
    try:
        return check_nprobe(int(text))
    except ValueError:
        raise argparse.ArgumentTypeError(f"nprobe {text!r} outside 1..{L.IVF_MAX_NPROBE}")


def check_offsets(offsets, n_lists, n_rows):
    """The list offsets of an IVF index as a CPU int32 tensor [n_lists + 1]: they start at 0, never descend and end at the
    number of rows (every row belongs to a list); ValueError otherwise."""
    o = torch.as_tensor(offsets).detach().to("cpu")
    if o.dim() != 1 or o.numel() != int(n_lists) + 1 or o.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"offsets: expected {int(n_lists) + 1} integers, got {o.dtype} {tuple(o.shape)}")
    o = o.to(torch.int64)
    if int(o[0]) != 0 or bool((o[1:] < o[:-1]).any()) or int(o[-1]) != int(n_rows):
        raise ValueError(f"offsets must start at 0, never descend and end at {int(n_rows)} rows")
    return o.to(torch.int32)


def pack_ivf_state(bank, centroids, offsets, order, nprobe):
    """The dictionary an IVF bank file holds: format 3, the single-bank dictionary of the grouped rows (`pack_state`), the
    fp16 centroid keys [nlist, C], offsets int32 [nlist + 1], order int32 [N] (a permutation) and nprobe."""
    bank = dict(bank)
    keys, _, _, channels, _ = unpack_state(bank)
    n = int(keys.shape[0])
    centroids = torch.as_tensor(centroids).detach().cpu().contiguous()
    if centroids.dim() != 2 or centroids.dtype != torch.float16 or centroids.shape[1] != channels or not 1 <= centroids.shape[0] <= n:
        raise ValueError(f"centroids must be fp16 [1..{n}, {channels}], got {centroids.dtype} {tuple(centroids.shape)}")
    offsets = check_offsets(offsets, centroids.shape[0], n)
    order = torch.as_tensor(order).detach().cpu()
    if order.dim() != 1 or order.numel() != n or order.dtype not in (torch.int32, torch.int64) or \
            not torch.equal(torch.sort(order.to(torch.int64)).values, torch.arange(n)):
        raise ValueError(f"order must be a permutation of 0..{n - 1}")
    return {"format": FORMAT_IVF, "bank": bank, "centroids": centroids, "offsets": offsets, "order": order.to(torch.int32),
            "nprobe": check_nprobe(nprobe)}


def unpack_ivf_state(d):
    """Validate an IVF bank dictionary -> (single-bank dictionary, centroids, offsets, order, nprobe)."""
    if not isinstance(d, dict) or d.get("format") != FORMAT_IVF:
        raise ValueError("not an IVF index (format 3); other bank files load with retrieval.load_bank")
    for k in ("bank", "centroids", "offsets", "order", "nprobe"):
        if k not in d:
            raise KeyError(f"IVF bank file lacks {k!r} (keys: {sorted(d.keys())})")
    st = pack_ivf_state(d["bank"], d["centroids"], d["offsets"], d["order"], d["nprobe"])
    return st["bank"], st["centroids"], st["offsets"], st["order"], st["nprobe"]


def group_rows(bank, idx, nlist, check=True):
    """The rows of `bank` grouped by list (`jat_bank_group`): idx int32 [N] as `assign` writes it -> (grouped LatentBank,
    offsets int32 [nlist + 1], order int32 [N]).  Inside a list the rows ascend by their original number; order[p] is the
    original row of position p.  An idx entry outside [0, nlist) is placed behind all lists on the device; check: wait for the
    offsets and raise ValueError when there is one."""
    if not isinstance(bank, LatentBank):
        raise ValueError("group_rows: the bank is a LatentBank")
    N = len(bank)
    if isinstance(nlist, bool) or not isinstance(nlist, int):
        raise ValueError(f"nlist {nlist!r} must be an integer")
    if idx.shape != (N,) or idx.dtype != torch.int32 or idx.device != bank.device or not idx.is_contiguous():
        raise ValueError(f"idx: expected a contiguous int32 [{N}] tensor on {bank.device}")
    need = C.c_size_t()
    L.check(L.lib().jat_bank_group_workspace_bytes(bank._h, nlist, C.byref(need)))
    dst = LatentBank(bank.channels, N, key=bank.key, device=bank.device)
    if bank.stats is not None:
        dst._set_stats(bank.stats)
    offsets = torch.empty(nlist + 1, dtype=torch.int32, device=bank.device)
    order = torch.empty(N, dtype=torch.int32, device=bank.device)
    work = torch.empty(need.value, dtype=torch.uint8, device=bank.device)
    with torch.cuda.device(bank.device):
        L.check(L.lib().jat_bank_group(bank._h, L.ptr(idx), nlist, dst._h, L.ptr(offsets), L.ptr(order), L.ptr(work),
                                       work.numel(), L.stream_ptr()))
    work.record_stream(torch.cuda.current_stream(bank.device))
    if check and int(offsets[-1]) != N:
        raise ValueError(f"group_rows: {N - int(offsets[-1])} entries of idx lie outside [0, {nlist}); they belong to no list")
    return dst, offsets, order


class IVFBank:
    """An inverted-file index over a `LatentBank` (RVC's `IVF{n},Flat`): `.bank` holds the rows grouped by list, `.centroids`
    the coarse quantiser (a LatentBank of nlist rows), `.offsets` int32 [nlist + 1] the lists' positions, `.order` int32 [N] the
    original row of every position, `.nprobe` how many lists a search scans.  Every index a search returns is a position in
    `.bank`, so `blend`, `blend_topk` and `rows` are the bank's own.  Within the probed lists the result is the exact search's,
    bit for bit; `nprobe >= nlist` is `bank.search_topk`."""

    def __init__(self, bank, centroids, offsets, order, nprobe=1):
        if not isinstance(bank, LatentBank) or not isinstance(centroids, LatentBank):
            raise ValueError("IVFBank: the bank and the centroids are LatentBanks")
        if bank.channels != centroids.channels:
            raise ValueError(f"IVFBank: bank of {bank.channels} channels, centroids of {centroids.channels}")
        if bank.device != centroids.device:
            raise ValueError(f"IVFBank: bank on {bank.device}, centroids on {centroids.device}")
        self.bank, self.centroids, self.nprobe = bank, centroids, check_nprobe(nprobe)
        self.offsets = offsets.to(bank.device, torch.int32).contiguous()
        self.order = order.to(bank.device, torch.int32).contiguous()
        if self.offsets.shape != (len(centroids) + 1,) or self.order.shape != (len(bank),):
            raise ValueError(f"IVFBank: offsets {tuple(self.offsets.shape)} / order {tuple(self.order.shape)} for "
                             f"{len(centroids)} lists over {len(bank)} rows")
        self._work = None

    # ---- what the bank answers itself --------------------------------------------------------------------------------------
    key = property(lambda self: self.bank.key)
    stats = property(lambda self: self.bank.stats)
    channels = property(lambda self: self.bank.channels)
    device = property(lambda self: self.bank.device)
    nlist = property(lambda self: len(self.centroids))

    def check_stats(self, stats):
        self.bank.check_stats(stats)

    def __len__(self):
        return len(self.bank)

    def rows(self, which="keys", full=False):
        return self.bank.rows(which, full)

    def blend(self, *args, **kwargs):
        return self.bank.blend(*args, **kwargs)

    def blend_topk(self, *args, **kwargs):
        return self.bank.blend_topk(*args, **kwargs)

    def list_sizes(self):
        """Rows per list, int64 [nlist] on the CPU."""
        o = self.offsets.cpu().to(torch.int64)
        return o[1:] - o[:-1]

    # ---- building -------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_centroids(cls, bank, centroids, nprobe=1):
        """The index of `bank` under a given coarse quantiser (a LatentBank of 1..N rows of the same key kind): `assign`, then
        `group_rows`.  The bank itself is left as it is; the index holds a grouped copy."""
        nprobe = check_nprobe(nprobe)
        if not isinstance(bank, LatentBank) or not isinstance(centroids, LatentBank):
            raise ValueError("IVFBank: the bank and the centroids are LatentBanks")
        if len(bank) > L.IVF_MAX_ROWS:
            raise ValueError(f"IVFBank: a bank of {len(bank)} rows exceeds {L.IVF_MAX_ROWS}")
        idx, _ = centroids.assign(bank)
        grouped, offsets, order = group_rows(bank, idx, len(centroids))
        return cls(grouped, centroids, offsets, order, nprobe)

    @classmethod
    def build(cls, bank, nlist=None, iters=10, nprobe=1):
        """k-means with `nlist` clusters (default: `default_nlist`; empty clusters dropped), then `from_centroids` ->
        (index, report): the k-means report plus the lists' min / median / max size."""
        nprobe = check_nprobe(nprobe)
        if not isinstance(bank, LatentBank):
            raise ValueError("IVFBank: the bank is a LatentBank")
        nlist = default_nlist(len(bank)) if nlist is None else check_clusters(nlist)
        cent, report = kmeans(bank, nlist, iters=iters, drop_empty=True)
        ivf = cls.from_centroids(bank, cent, nprobe)
        sizes = sorted(ivf.list_sizes().tolist())
        report = dict(report, lists=len(cent), list_min=sizes[0], list_median=sizes[len(sizes) // 2], list_max=sizes[-1],
                      nprobe=nprobe)
        return ivf, report

    # ---- use ------------------------------------------------------------------------------------------------------------------
    def workspace_bytes(self, n_queries, k, nprobe):
        n = C.c_size_t()
        L.check(L.lib().jat_ivf_search_workspace_bytes(self.bank._h, self.centroids._h, int(n_queries), int(k), int(nprobe),
                                                       C.byref(n)))
        return n.value

    def search_topk(self, x, k, mean=None, std=None, nprobe=None, probes=False):
        """The k nearest rows of every frame among the lists of its `nprobe` (default: the index's) nearest centroids, ordered
        by (distance, position) -> (idx int32 [B, T, k], dist2 fp32 [B, T, k]); with probes also the probed lists int32
        [B, T, nprobe] (-1: fewer lists than probes).  Fewer candidates than k: the tail is idx -1 and dist2 +inf."""
        k = check_index_k(k)
        nprobe = self.nprobe if nprobe is None else check_nprobe(nprobe)
        x = self.bank._x(x)
        B, _, T = x.shape
        if B < 1 or T < 1:
            raise ValueError(f"x {tuple(x.shape)}: B and T must be positive")
        need = self.workspace_bytes(B * T, k, nprobe)
        if self._work is None or self._work.numel() < need:
            self._work = torch.empty(need, dtype=torch.uint8, device=self.device)
        idx = torch.empty(B, T, k, dtype=torch.int32, device=self.device)
        dist2 = torch.empty(B, T, k, dtype=torch.float32, device=self.device)
        pr = torch.empty(B, T, nprobe, dtype=torch.int32, device=self.device) if probes else None
        mean, std = self.bank._vec(mean), self.bank._vec(std)
        with torch.cuda.device(self.device):
            L.check(L.lib().jat_ivf_search(self.bank._h, self.centroids._h, L.ptr(self.offsets), L.ptr(x), L.ptr(mean),
                                           L.ptr(std), B, T, k, nprobe, L.ptr(idx), L.ptr(dist2), L.ptr(pr), L.ptr(self._work),
                                           self._work.numel(), L.stream_ptr()))
        return (idx, dist2, pr) if probes else (idx, dist2)

    def search(self, x, mean=None, std=None, nprobe=None):
        """`search_topk` with k = 1 -> (idx int32 [B, T], dist2 fp32 [B, T])."""
        idx, dist2 = self.search_topk(x, 1, mean, std, nprobe=nprobe)
        return idx[..., 0], dist2[..., 0]

    def retrieve(self, x, index_rate, stats=None, query=None, k=1, dist2_floor=1e-6, neighbours=False):
        """`LatentBank.retrieve` with the IVF search in the place of the exact one; the blends are the bank's own.  index_rate
        may be a per-frame track as there."""
        if is_rate_track(index_rate):
            return _retrieve_with_track(self, x, index_rate, neighbours=neighbours, stats=stats, query=query, k=k,
                                        dist2_floor=dist2_floor)
        check_index_rate(index_rate)
        k = check_index_k(k)
        check_dist2_floor(dist2_floor)
        if stats is not None:
            self.check_stats(stats)
        elif self.stats is None:
            raise ValueError("the bank holds no statistics yet (nothing was added)")
        s = self.bank._dev_stats
        if self.key == "lr":
            if query is None:
                raise ValueError("a bank keyed by LR frames needs the LR latent as `query`")
            if query.shape != x.shape:
                raise ValueError(f"query {tuple(query.shape)} does not match x {tuple(x.shape)}")
            q, mean, std = query.to(self.device, torch.float32), s["lr_mean"], s["lr_std"]
        else:
            q, mean, std = x, s["hr_mean"], s["hr_std"]
        if k == 1:
            idx, dist2 = self.search(q, mean, std)
            idx, dist2 = idx.contiguous(), dist2.contiguous()
            y = self.bank.blend(x, idx, index_rate, s["hr_mean"], s["hr_std"])
        else:
            idx, dist2 = self.search_topk(q, k, mean, std)
            y = self.bank.blend_topk(x, idx, dist2, index_rate, s["hr_mean"], s["hr_std"], dist2_floor=dist2_floor)
        return (y, idx, dist2) if neighbours else y

    # ---- files ----------------------------------------------------------------------------------------------------------------
    def state(self):
        return pack_ivf_state(self.bank.state(), self.centroids.rows("keys")[0].cpu(), self.offsets.cpu(), self.order.cpu(),
                              self.nprobe)

    def save(self, path):
        torch.save(self.state(), path)

    @classmethod
    def from_state(cls, d, device="cuda"):
        bank_d, centroids, offsets, order, nprobe = unpack_ivf_state(d)
        bank = LatentBank.from_state(bank_d, device=device)
        cent = LatentBank(bank.channels, int(centroids.shape[0]), key="hr", device=device)   # only the keys are used
        cent.load_rows(centroids)
        return cls(bank, cent, offsets, order, nprobe)

    @classmethod
    def load(cls, path, device="cuda"):
        return cls.from_state(torch.load(path, map_location="cpu", weights_only=False), device=device)


# ---- voicing-aware index rates (C ABI: include/jat_hip_rate.h) ------------------------------------------------------
def check_half_window(half_window):
    """The half window of the stability count as an int in 0..32 (JAT_RATE_MAX_HALF_WINDOW); ValueError otherwise."""
    if isinstance(half_window, bool) or not isinstance(half_window, int) or not 0 <= half_window <= L.RATE_MAX_HALF_WINDOW:
        raise ValueError(f"half_window {half_window!r} outside 0..{L.RATE_MAX_HALF_WINDOW}")
    return half_window


def check_smooth(smooth):
    """The half width of the rate smoothing as an int in 0..16 (JAT_RATE_MAX_SMOOTH); ValueError otherwise."""
    if isinstance(smooth, bool) or not isinstance(smooth, int) or not 0 <= smooth <= L.RATE_MAX_SMOOTH:
        raise ValueError(f"smooth {smooth!r} outside 0..{L.RATE_MAX_SMOOTH}")
    return smooth


def smooth_arg(text):
    """argparse type of --index-smooth."""
    try:
        return check_smooth(int(text))
    except ValueError:
        raise argparse.ArgumentTypeError(f"smooth {text!r} outside 0..{L.RATE_MAX_SMOOTH}")


def check_rate_factor(name, value):
    """A factor on the index rate (protect, unstable) as a float in [0, 1]; ValueError otherwise (a NaN is outside)."""
    v = float(value)
    if not 0.0 <= v <= 1.0:
        raise ValueError(f"{name} {value!r} outside [0, 1]")
    return v


def protect_arg(text):
    """argparse type of --index-protect."""
    try:
        return check_rate_factor("protect", text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


def unstable_arg(text):
    """argparse type of --index-unstable."""
    try:
        return check_rate_factor("unstable", text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


def cents_ratio(cents):
    """float32(2 ** (cents / 1200)): the frequency ratio `jat_f0_classes` compares with.  It must come out finite and above 1
    in fp32 (so cents is positive and at least about 1e-4); ValueError otherwise."""
    try:
        r = C.c_float(2.0 ** (float(cents) / 1200.0)).value
    except OverflowError:
        r = float("inf")
    if not 1.0 < r < float("inf"):
        raise ValueError(f"cents {cents!r}: the ratio {r!r} must be finite and above 1 in fp32")
    return r


def default_min_count(half_window):
    """2 W + 1 - W // 2 agreeing frames of the 2 W + 1 in the window: 7 of 9 at the default W = 4."""
    w = check_half_window(half_window)
    return 2 * w + 1 - w // 2


def rate_table(index_rate, protect=1.0, unstable=1.0):
    """The three rates of the classes {not live, unstable, stable}: float32(R protect), float32(R unstable), float32(R), the
    products taken in double (returned as Python floats holding those fp32 values)."""
    r = check_index_rate(index_rate)
    p, u = check_rate_factor("protect", protect), check_rate_factor("unstable", unstable)
    return (C.c_float(r * p).value, C.c_float(r * u).value, C.c_float(r).value)


def f0_classes(f0, voiced, half_window=4, cents=50.0, min_count=None, counts=False):
    """The F0-stability class of every frame of a pitch track (`jat_f0_classes`): f0 fp32 and voiced bool / uint8, [F] or
    [B, F], as `pitch.yin` / `pitch.pyin` return them -> (cls uint8, summary int32 [2] or [B, 2] = {live frames, stable
    frames}), on the device.  A frame is live when its flag is set and its f0 is positive and finite; a live frame is stable
    (2) when at least `min_count` (default `default_min_count`: 7 of 9) frames of the `half_window` frames on either side of it,
    itself included, are live and within `cents` of it, unstable (1) otherwise; 0: not live.  counts: also the counts int32."""
    if not (isinstance(f0, torch.Tensor) and isinstance(voiced, torch.Tensor)) or not (f0.is_cuda and voiced.is_cuda):
        raise ValueError("f0_classes: f0 and voiced must be CUDA tensors (there is no CPU path)")
    if f0.dtype != torch.float32 or voiced.dtype not in (torch.bool, torch.uint8) or f0.shape != voiced.shape or \
            f0.dim() not in (1, 2) or f0.numel() < 1 or f0.device != voiced.device:
        raise ValueError("f0_classes: f0 float32 and voiced bool / uint8 of one shape [F] or [B, F] on one device, not empty")
    w = check_half_window(half_window)
    ratio = cents_ratio(cents)
    m = default_min_count(w) if min_count is None else min_count
    if isinstance(m, bool) or not isinstance(m, int) or not 1 <= m <= 2 * w + 1:
        raise ValueError(f"min_count {min_count!r} outside 1..{2 * w + 1}")
    batched = f0.dim() == 2
    f = f0.detach().reshape(-1, f0.shape[-1]).contiguous()
    v = voiced.detach().reshape(f.shape).contiguous()
    v = v.view(torch.uint8) if v.dtype == torch.bool else v
    B, F = f.shape
    with torch.cuda.device(f.device):
        cls = torch.empty(B, F, dtype=torch.uint8, device=f.device)
        cnt = torch.empty(B, F, dtype=torch.int32, device=f.device) if counts else None
        summary = torch.empty(B, 2, dtype=torch.int32, device=f.device)
        L.check(L.lib().jat_f0_classes(L.ptr(f), L.ptr(v), B, F, w, ratio, m, L.ptr(cls), L.ptr(cnt), L.ptr(summary),
                                       L.stream_ptr()))
    out = (cls, summary, cnt) if counts else (cls, summary)
    return out if batched else tuple(t[0] for t in out)


def rate_track(cls, frames, index_rate, protect=1.0, unstable=1.0, smooth=2):
    """Classes to a per-frame index rate (`jat_rate_track`): cls uint8 [F] or [B, F] on the device -> rates fp32 [frames] or
    [B, frames].  A stable frame gets `index_rate`, an unstable one `index_rate * unstable`, a frame that is not live (or
    behind the end of the pitch track) `index_rate * protect`; the track is then averaged over `smooth` frames on either side
    (0: not at all) in a form that leaves a frame farther than `smooth` from any change of class at its table value exactly.
    protect = 1 and unstable = 1 change nothing.  `protect` is the plain factor on the rate of unvoiced frames: RVC's slider of
    that name means "off" at 0.5 and defaults to 0.33; here 1 is off and RVC's default corresponds to 0.33."""
    if not isinstance(cls, torch.Tensor) or not cls.is_cuda or cls.dtype != torch.uint8 or cls.dim() not in (1, 2) or \
            cls.numel() < 1:
        raise ValueError("rate_track: cls must be a CUDA uint8 tensor [F] or [B, F], not empty")
    if isinstance(frames, bool) or not isinstance(frames, int) or frames < 1:
        raise ValueError(f"rate_track: frames {frames!r} must be a positive integer")
    table = rate_table(index_rate, protect, unstable)
    s = check_smooth(smooth)
    c = cls.detach().reshape(-1, cls.shape[-1]).contiguous()
    B, F = c.shape
    with torch.cuda.device(c.device):
        r = torch.empty(B, frames, dtype=torch.float32, device=c.device)
        L.check(L.lib().jat_rate_track(L.ptr(c), B, F, frames, (C.c_float * 3)(*table), s, L.ptr(r), L.stream_ptr()))
    return r if cls.dim() == 2 else r[0]


def check_rates(rates, B, T, device):
    """A per-frame index-rate track for x [B, C, T]: an fp32 tensor [B, T] (or [T] for B = 1) on `device` with every value in
    [0, 1] (checked on the host: this waits for the device) -> the contiguous [B, T] tensor; ValueError otherwise."""
    if not isinstance(rates, torch.Tensor):
        raise ValueError(f"index rates: expected a tensor, got {type(rates).__name__}")
    device = torch.device(device)
    if rates.device != device:
        raise ValueError(f"index rates: on {rates.device}, expected {device}")
    if rates.dtype != torch.float32:
        raise ValueError(f"index rates: dtype {rates.dtype}, expected float32")
    if tuple(rates.shape) != (B, T) and not (B == 1 and tuple(rates.shape) == (T,)):
        raise ValueError(f"index rates: shape {tuple(rates.shape)}, expected [{B}, {T}]" + (f" or [{T}]" if B == 1 else ""))
    r = rates.detach().reshape(B, T).contiguous()
    if not bool(((r >= 0.0) & (r <= 1.0)).all()):
        raise ValueError("index rates: a value outside [0, 1] (or a NaN)")
    return r


def _mix_rates(x, v, rates, out):
    B, Cc, T = x.shape
    with torch.cuda.device(x.device):
        L.check(L.lib().jat_rate_mix(L.ptr(x), L.ptr(v), L.ptr(rates), L.ptr(out), B, Cc, T, L.stream_ptr()))
    return out


def mix_rates(x, v, rates, out=None):
    """(1 - r) x + r v with r = rates[b, t], one rate per frame (`jat_rate_mix`): x and v fp32 [B, C, T], rates fp32 [B, T] (or
    [T] for B = 1) in [0, 1].  A constant track gives the bits of `blend` / `blend_topk` / `mix_scales` at that rate when v is
    what they return at rate 1.  out: where to write; may be x or v."""
    x, v = _frames(x), _frames(v, "v")
    if v.shape != x.shape or v.device != x.device:
        raise ValueError(f"v {tuple(v.shape)} on {v.device} does not match x {tuple(x.shape)} on {x.device}")
    rates = check_rates(rates, x.shape[0], x.shape[2], x.device)
    if out is None:
        out = torch.empty_like(x)
    elif out.shape != x.shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != x.device:
        raise ValueError("mix_rates(out=...): out must be a contiguous fp32 tensor of x's shape")
    return _mix_rates(x, v, rates, out)


def is_rate_track(index_rate):
    """Whether `retrieve` was given a per-frame track (a tensor with at least one dimension) and not a scalar rate."""
    return isinstance(index_rate, torch.Tensor) and index_rate.dim() > 0


def _retrieve_with_track(bank, x, rates, neighbours=False, **kw):
    """`bank.retrieve` with a per-frame rate: the bank's own call at rate 1.0 returns the retrieved track, `jat_rate_mix` blends
    it in (over the track's buffer).  neighbours: the lists of that call, unchanged."""
    if not isinstance(x, torch.Tensor) or x.dim() != 3:
        raise ValueError("x: expected a CUDA fp32 [B, C, T] tensor")
    rates = check_rates(rates, int(x.shape[0]), int(x.shape[2]), bank.device)
    out = bank.retrieve(x, 1.0, neighbours=neighbours, **kw)
    v = out[0] if neighbours else out
    y = _mix_rates(x.contiguous(), v, rates, v)
    return (y,) + tuple(out[1:]) if neighbours else y


def load_bank(path, device="cuda"):
    """A bank file of any format -> `LatentBank` (format 1), `MultiScaleBank` (format 2) or `IVFBank` (format 3)."""
    d = torch.load(path, map_location="cpu", weights_only=False)
    if isinstance(d, dict) and d.get("format") == FORMAT_IVF:
        return IVFBank.from_state(d, device=device)
    if isinstance(d, dict) and d.get("format") == FORMAT_MS:
        return MultiScaleBank.from_state(d, device=device)
    return LatentBank.from_state(d, device=device)


def _device_view(address, shape, dtype, device, owner):
    """A tensor over device memory the library owns (`owner` keeps it alive)."""
    n = 1
    for v in shape:
        n *= int(v)
    if n == 0:
        return torch.empty(shape, dtype=dtype, device=device)
    typestr = {torch.float16: "<f2", torch.float32: "<f4"}[dtype]

    class _Mem:
        __cuda_array_interface__ = {"shape": tuple(int(v) for v in shape), "typestr": typestr, "data": (int(address), False),
                                    "version": 2, "strides": None}
        _owner = owner
    return torch.as_tensor(_Mem(), device=device)


def build_parser():
    p = argparse.ArgumentParser(description="latent retrieval banks (jatsr_amd.retrieval)")
    sub = p.add_subparsers(dest="command", required=True)
    b = sub.add_parser("build", help="build a bank file from a prepared data folder")
    b.add_argument("--data-dir", required=True, help="prepared data folder (holds the split folders and the statistics)")
    b.add_argument("--out", required=True, help="bank file to write (.pt)")
    b.add_argument("--stats-file", default=None, help="normalisation statistics (default: DATA_DIR/global_stats_separated.json)")
    b.add_argument("--split", default="train")
    b.add_argument("--max-frames", type=int, default=100_000, help="upper bound on the rows of the bank")
    b.add_argument("--key", default="hr", choices=["hr", "lr"], help="what a frame is looked up by")
    b.add_argument("--device", default="cuda")
    b.add_argument("--scales", type=scales_arg, default=None, metavar="S1,S2,...",
                   help="write a multi-scale bank (format 2): one bank per time scale, each of 1, 2, 4, 8, ascending, e.g. 1,2,4 "
                        "(default: a single bank, the file as it always was)")
    b.add_argument("--scale-weights", type=scale_weights_arg, default=None, metavar="W1,W2,...",
                   help="with --scales: the share of each scale's track in the mix, normalised to sum 1 (default: equal)")
    b.add_argument("--clusters", type=int, default=None, metavar="K",
                   help="cluster a pool of frames with k-means on the GPU and store the K centroids (empty clusters dropped) "
                        "as the bank: the same file format (default: the strided frames themselves, --max-frames of them)")
    b.add_argument("--pool-frames", type=int, default=None, metavar="N",
                   help="with --clusters: upper bound on the frames that are clustered (default: all, 2^22 at most)")
    b.add_argument("--kmeans-iters", type=int, default=10, metavar="I", help="with --clusters: iterations at most")
    b.add_argument("--ivf", action="store_true",
                   help="write an IVF index (format 3): the rows grouped by their nearest of N k-means centroids, searched "
                        "through the nearest lists only.  With --clusters the bank is compacted first, then indexed.  Not "
                        "combinable with --scales: a multi-scale IVF index is out of scope")
    b.add_argument("--ivf-lists", type=int, default=None, metavar="N",
                   help="with --ivf: the number of lists (default: min(int(16 sqrt(rows)), rows // 39), as RVC trains its index)")
    b.add_argument("--ivf-nprobe", type=nprobe_arg, default=None, metavar="P",
                   help=f"with --ivf: the lists a search scans, 1..{L.IVF_MAX_NPROBE}, stored in the file (default: 1, as RVC searches)")
    return p


def main(argv=None):
    from . import io as jio
    args = build_parser().parse_args(argv)
    folder = os.path.join(args.data_dir, args.split)
    files = sorted(glob.glob(os.path.join(folder, "*.pt")))
    if not files:
        raise SystemExit(f"No .pt files found in {folder}")
    channels = int(torch.load(files[0], map_location="cpu", mmap=True, weights_only=False)["hr_latent"].shape[0])
    stats = jio.load_stats(args.stats_file or os.path.join(args.data_dir, "global_stats_separated.json"), channels=channels)
    if args.scale_weights is not None and args.scales is None:
        raise SystemExit("--scale-weights needs --scales")
    if args.ivf and args.scales is not None:
        raise SystemExit("--ivf cannot be combined with --scales: a multi-scale IVF index is out of scope")
    if not args.ivf and (args.ivf_lists is not None or args.ivf_nprobe is not None):
        raise SystemExit("--ivf-lists and --ivf-nprobe need --ivf")
    km = {}
    if args.clusters is None:
        if args.pool_frames is not None:
            raise SystemExit("--pool-frames needs --clusters")
    else:
        try:
            km = dict(clusters=check_clusters(args.clusters), pool_frames=check_pool_frames(args.pool_frames),
                      kmeans_iters=args.kmeans_iters)
            if args.kmeans_iters < 1:
                raise ValueError(f"kmeans_iters {args.kmeans_iters} must be at least 1")
        except ValueError as e:
            raise SystemExit(f"--clusters: {e}")
    if args.scales is None:
        bank = LatentBank.from_data_dir(args.data_dir, stats, split=args.split, max_frames=args.max_frames, key=args.key,
                                        device=args.device, **km)
    else:
        try:
            weights = check_scale_weights(args.scale_weights, len(args.scales))
        except ValueError as e:
            raise SystemExit(f"--scale-weights: {e}")
        bank = MultiScaleBank.from_data_dir(args.data_dir, stats, split=args.split, max_frames=args.max_frames, key=args.key,
                                            device=args.device, scales=args.scales, weights=args.scale_weights, **km)
    kmeans_report = bank.kmeans_report if km else None
    if args.ivf:
        import json
        try:
            bank, ivf_report = IVFBank.build(bank, nlist=args.ivf_lists, iters=args.kmeans_iters,
                                             nprobe=1 if args.ivf_nprobe is None else args.ivf_nprobe)
        except ValueError as e:
            raise SystemExit(f"--ivf: {e}")
        with open(args.out + ".ivf.json", "w") as f:
            json.dump(ivf_report, f, indent=1)
        print(f"IVF index: {ivf_report['lists']} lists of {ivf_report['list_min']} / {ivf_report['list_median']} / "
              f"{ivf_report['list_max']} rows (min / median / max), nprobe {bank.nprobe}; report -> {args.out}.ivf.json")
    bank.save(args.out)
    if km:
        import json
        with open(args.out + ".kmeans.json", "w") as f:
            json.dump(kmeans_report, f, indent=1)
        print(f"k-means report -> {args.out}.kmeans.json")
    print(f"bank of {len(bank)} x {bank.channels} fp16 rows (key={bank.key}) from {len(files)} files" +
          (f", scales {list(args.scales)} with weights {[round(w, 6) for w in weights]}" if args.scales else "") + f" -> {args.out}")
    return args.out


if __name__ == "__main__":
    main()
