"""Training data on MI355X: the prepared latent files kept in HBM as fp16, batches assembled by one kernel.

Replaces the reference's LatentDataset / ValidationDataset + DistributedSampler + DataLoader (train_ddp_v3mod2.py:476-597,
677-699) and the host-to-device copy and normalisation at the head of its step (:849-857):

    store = LatentStore(data_dir, "train", frames=1378, device="cuda")
    for batch in epoch_batches(len(store), 6, 28, epoch, rank, world, shuffle=True, seed=seed):
        files, starts = train_batch_plan(store.lengths, 1378, batch, seed, epoch)
        hr_norm, lr_norm = store.batch(files, starts, stats)        # fp32 [B, C, T], cropped and normalised

The index arithmetic (epoch order, rank shard, crop starts) is host code and equals the reference's; the bytes move in
`jat_latent_gather` (include/jat_hip.h).  There is no CPU path.
"""
from __future__ import annotations

import glob
import math
import os

import torch

from . import _lib as L

_M64 = (1 << 64) - 1
_GUARD = 64            # fp16 elements either side of the staging buffer, kept at _CANARY
_CANARY = 0x7C01       # an fp16 NaN pattern no latent file holds


def epoch_batches(n_files, multiplier, batch_size, epoch, rank=0, world=1, shuffle=True, seed=0):
    """The index batches of one rank for one epoch: what
    `DataLoader(ds, batch_size, sampler=DistributedSampler(ds, world, rank, shuffle, seed), drop_last=True)` yields after
    `sampler.set_epoch(epoch)` for `len(ds) = n_files * multiplier` (train_ddp_v3mod2.py:680-699, 832): `torch.randperm`
    seeded `seed + epoch`, padded by wrap-around to a multiple of `world`, sharded with stride `world`, the last partial
    batch dropped.  Sample idx is file `idx % n_files`."""
    n = int(n_files) * int(multiplier)
    if n < 1 or batch_size < 1 or not 0 <= rank < world:
        raise ValueError(f"epoch_batches: {n} samples, batch {batch_size}, rank {rank} of {world}")
    if shuffle:
        g = torch.Generator()
        g.manual_seed(int(seed) + int(epoch))
        idx = torch.randperm(n, generator=g).tolist()
    else:
        idx = list(range(n))
    total = math.ceil(n / world) * world
    pad = total - n
    if pad <= len(idx):
        idx += idx[:pad]
    else:
        idx += (idx * math.ceil(pad / len(idx)))[:pad]
    mine = idx[rank:total:world]
    return [mine[i:i + batch_size] for i in range(0, len(mine) - batch_size + 1, batch_size)]


def val_crop_start(length, frames, multiplier, sample_idx):
    """The validation set's deterministic crop start (train_ddp_v3mod2.py:573-591): the centre crop for multiplier == 1,
    else `multiplier` starts spread evenly over [0, length - frames]; 0 for a clip shorter than `frames` (it is
    loop-repeated from its first frame)."""
    if length < frames:
        return 0
    if multiplier == 1:
        return (length - frames) // 2
    segment = max(length - frames, 1)
    return min(int(segment * sample_idx / (multiplier - 1)), length - frames)


def _splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def train_crop_start(length, frames, seed, epoch, idx):
    """Training crop start, uniform on [0, length - frames] (0 for a shorter clip): a splitmix64 hash of
    (seed, epoch, idx).  The reference draws it with an unseeded, worker-local `random.randint`
    (train_ddp_v3mod2.py:527), so there is no sequence to match; this one is a function of its arguments alone, so a
    resumed run crops exactly as the uninterrupted one would have."""
    if length <= frames:
        return 0
    h = _splitmix64(int(seed) & _M64)
    h = _splitmix64(h ^ (int(epoch) & _M64))
    h = _splitmix64(h ^ (int(idx) & _M64))
    return h % (length - frames + 1)


def train_batch_plan(lengths, frames, batch, seed, epoch):
    """Index batch -> (file indices, crop starts) of a training batch."""
    n = len(lengths)
    files = [i % n for i in batch]
    return files, [train_crop_start(lengths[f], frames, seed, epoch, i) for f, i in zip(files, batch)]


def val_batch_plan(lengths, frames, batch, multiplier):
    """Index batch -> (file indices, crop starts) of a validation batch: sample_idx = idx // n_files
    (train_ddp_v3mod2.py:563-564)."""
    n = len(lengths)
    files = [i % n for i in batch]
    return files, [val_crop_start(lengths[f], frames, multiplier, i // n) for f, i in zip(files, batch)]


def _load_fp16(path):
    data = torch.load(path, map_location="cpu", mmap=True, weights_only=False)
    if "hr_latent" not in data or "lr_latent" not in data:
        raise KeyError(f"{path}: needs 'hr_latent' and 'lr_latent' (keys: {list(data.keys())})")
    hr, lr = data["hr_latent"], data["lr_latent"]
    if hr.dim() != 2 or hr.shape != lr.shape or hr.shape[-1] < 1:
        raise ValueError(f"{path}: hr_latent {tuple(hr.shape)} / lr_latent {tuple(lr.shape)}, expected two equal [C, T]")
    return hr.to(torch.float16).contiguous(), lr.to(torch.float16).contiguous()     # fp16 files: no copy, still mmap'd


class LatentStore:
    """One split of a prepared data set (`python -m jatsr_amd.prepare`) as fp16 in device memory.

    Every file's `hr_latent` / `lr_latent` is uploaded once, as stored (fp16 [C, len]); files beyond `max_resident_bytes`
    (default: half of the free device memory at construction) stay in pinned host memory as fp16, and their crops reach a
    device staging buffer through an asynchronous copy on a side stream — one batch ahead when `prefetch` is used.  Files
    shorter than `frames` are always device-resident, so the loop-repeat exists once, in the kernel."""

    def __init__(self, data_dir, split, frames, device="cuda", max_resident_bytes=None):
        L.require_gpu()
        self.dir = os.path.join(str(data_dir), split)
        self.files = sorted(glob.glob(os.path.join(self.dir, "*.pt")))
        if not self.files:
            raise ValueError(f"No .pt files found in {self.dir}")      # train_ddp_v3mod2.py:490-491
        self.frames = int(frames)
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if max_resident_bytes is None:
            max_resident_bytes = torch.cuda.mem_get_info(self.device)[0] // 2
        self.lengths, self._dev, self._host = [], [], []
        self.channels = None
        self.resident_bytes = self.host_bytes = 0
        for path in self.files:
            hr, lr = _load_fp16(path)
            if self.channels is None:
                self.channels = int(hr.shape[0])
            if hr.shape[0] != self.channels:
                raise ValueError(f"{path}: {hr.shape[0]} channels, the files before it have {self.channels}")
            nbytes = 2 * hr.numel() * 2
            self.lengths.append(int(hr.shape[1]))
            if hr.shape[1] < self.frames or self.resident_bytes + nbytes <= max_resident_bytes:
                self._dev.append((hr.to(self.device), lr.to(self.device)))
                self._host.append(None)
                self.resident_bytes += nbytes
            else:
                self._dev.append(None)
                self._host.append((torch.empty(hr.shape, dtype=torch.float16, pin_memory=True).copy_(hr),
                                   torch.empty(lr.shape, dtype=torch.float16, pin_memory=True).copy_(lr)))
                self.host_bytes += nbytes
        self._side = torch.cuda.Stream(device=self.device) if self.host_bytes else None
        self._stage_flat = None          # [_GUARD | 2 slots x (hr, lr) x B x C x frames | _GUARD] fp16
        self._stage_B = 0
        self._slot = 0
        self._slot_free = [None, None]   # event: the gather that last read the slot has run
        self._staged = None              # (key, slot, copy-done event) of a prefetched batch
        self._tables, self._table_next = None, 0     # pinned [4, B] table buffers and the events of their uploads

    def __len__(self):
        return len(self.files)

    def is_resident(self, file_idx):
        return self._dev[file_idx] is not None

    # -- host-resident files: crops -> device staging buffer on the side stream --------------------------------------
    def _stage_view(self, B):
        if self._stage_flat is None or B > self._stage_B:
            if self._stage_flat is not None:
                torch.cuda.synchronize(self.device)
            n = 2 * 2 * B * self.channels * self.frames
            flat = torch.full((n + 2 * _GUARD,), _CANARY, dtype=torch.int16, device=self.device).view(torch.float16)
            self._stage_flat, self._stage_B = flat, B
            self._slot_free, self._staged = [None, None], None
        return self._stage_flat[_GUARD:-_GUARD].view(2, 2, self._stage_B, self.channels, self.frames)

    def stage_guards(self):
        """The guard elements before and after the staging buffer as int16 (all `0x7C01` unless something wrote out of
        bounds); None while no host-resident file has been staged."""
        if self._stage_flat is None:
            return None
        bits = self._stage_flat.view(torch.int16)
        return bits[:_GUARD], bits[-_GUARD:]

    def _check(self, file_idx, starts):
        if len(file_idx) != len(starts) or not file_idx:
            raise ValueError(f"batch of {len(file_idx)} files with {len(starts)} starts")
        for f, s in zip(file_idx, starts):
            n = self.lengths[f]
            if n >= self.frames and not 0 <= s <= n - self.frames:
                raise ValueError(f"{self.files[f]}: crop start {s} outside [0, {n - self.frames}]")
            if n < self.frames and s != 0:
                raise ValueError(f"{self.files[f]}: a clip of {n} < {self.frames} frames repeats from its first frame (start 0)")

    def _stage(self, file_idx, starts):
        """Queue the copies of this batch's host-resident crops on the side stream -> (slot, event)."""
        stage = self._stage_view(len(file_idx))
        slot = self._slot
        self._slot ^= 1
        T = self.frames
        with torch.cuda.stream(self._side):
            if self._slot_free[slot] is not None:
                self._side.wait_event(self._slot_free[slot])
            for i, (f, s) in enumerate(zip(file_idx, starts)):
                if self._host[f] is not None:
                    stage[slot, 0, i].copy_(self._host[f][0][:, s:s + T], non_blocking=True)
                    stage[slot, 1, i].copy_(self._host[f][1][:, s:s + T], non_blocking=True)
            done = torch.cuda.Event()
            done.record(self._side)
        return slot, done

    def _upload_table(self, rows):
        """The batch's four tables through one of a few pinned host buffers and a non-blocking copy on the current stream: no
        stream synchronisation per batch.  A buffer is rewritten only after the copy that last read it has run."""
        B = len(rows[0])
        if self._tables is None or self._tables[0][0].shape[1] != B:
            self._tables = [[torch.empty(4, B, dtype=torch.int64, pin_memory=True), None] for _ in range(4)]
            self._table_next = 0
        slot = self._tables[self._table_next]
        self._table_next = (self._table_next + 1) % len(self._tables)
        if slot[1] is not None:
            slot[1].synchronize()
        slot[0].copy_(torch.tensor(rows, dtype=torch.int64))
        table = torch.empty(4, B, dtype=torch.int64, device=self.device)
        table.copy_(slot[0], non_blocking=True)
        slot[1] = torch.cuda.Event()
        slot[1].record(torch.cuda.current_stream(self.device))
        return table

    def _stat_vector(self, v):
        if v.dtype == torch.float32 and v.device == self.device and v.dim() == 1 and v.is_contiguous():
            return v                     # the usual case (io.load_stats on the device): nothing is copied per batch
        return v.to(self.device, torch.float32).contiguous().view(-1)

    def prefetch(self, file_idx, starts):
        """Start staging the host-resident crops of the NEXT batch while the current step runs.  No-op when every file
        of the batch is device-resident."""
        file_idx, starts = [int(f) for f in file_idx], [int(s) for s in starts]
        self._check(file_idx, starts)
        if all(self._dev[f] is not None for f in file_idx):
            return
        slot, done = self._stage(file_idx, starts)
        self._staged = ((tuple(file_idx), tuple(starts)), slot, done)

    def batch(self, file_idx, starts, stats=None, out=None):
        """-> (hr, lr) fp32 [B, C, frames] on the device: the crops `[start, start + frames)` of the given files
        (loop-repeated when a file is shorter), normalised per channel with `stats` (dict of hr_mean / hr_std / lr_mean
        / lr_std, fp32 [C] on the device) or converted as they are with stats=None.  One `jat_latent_gather` launch on the
        current stream.  `out`: a pair of tensors to write into."""
        file_idx, starts = [int(f) for f in file_idx], [int(s) for s in starts]
        self._check(file_idx, starts)
        B, C, T = len(file_idx), self.channels, self.frames
        slot = None
        if any(self._dev[f] is None for f in file_idx):
            key = (tuple(file_idx), tuple(starts))
            if self._staged is not None and self._staged[0] == key:
                _, slot, done = self._staged
            else:
                slot, done = self._stage(file_idx, starts)
            self._staged = None
            torch.cuda.current_stream(self.device).wait_event(done)
            stage = self._stage_view(B)
        rows = [[], [], [], []]
        for i, (f, s) in enumerate(zip(file_idx, starts)):
            if self._dev[f] is not None:
                hr, lr = self._dev[f]
                entry = (hr.data_ptr(), lr.data_ptr(), self.lengths[f], s)
            else:
                entry = (stage[slot, 0, i].data_ptr(), stage[slot, 1, i].data_ptr(), T, 0)
            for r, v in zip(rows, entry):
                r.append(v)
        table = self._upload_table(rows)                                    # [4, B] int64 on the device
        if out is None:
            out = (torch.empty(B, C, T, dtype=torch.float32, device=self.device),
                   torch.empty(B, C, T, dtype=torch.float32, device=self.device))
        hr_out, lr_out = out
        for t in out:
            if tuple(t.shape) != (B, C, T) or t.dtype != torch.float32 or t.device != self.device or not t.is_contiguous():
                raise ValueError(f"out: expected contiguous fp32 [{B}, {C}, {T}] on {self.device}, got {tuple(t.shape)} "
                                 f"{t.dtype} on {t.device}")
        vec = [None] * 4
        if stats is not None:
            vec = [self._stat_vector(stats[k]) for k in ("hr_mean", "hr_std", "lr_mean", "lr_std")]
            if any(v.numel() != C for v in vec):
                raise ValueError(f"stats: expected {C} entries per vector")
        L.check(L.lib().jat_latent_gather(L.ptr(table[0]), L.ptr(table[1]), L.ptr(table[2]), L.ptr(table[3]),
                                          L.ptr(vec[0]), L.ptr(vec[1]), L.ptr(vec[2]), L.ptr(vec[3]),
                                          L.ptr(hr_out), L.ptr(lr_out), B, C, T, L.stream_ptr()))
        if slot is not None:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.device))
            self._slot_free[slot] = ev
        return hr_out, lr_out
