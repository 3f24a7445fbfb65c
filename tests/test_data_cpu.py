"""Host side of the training-run driver (jatsr_amd.data, jatsr_amd.fit), no GPU: the epoch order and rank shards equal
torch's own DistributedSampler + DataLoader, the crop starts and the short-clip index map equal the reference's data sets
(tests/golden/fit_crops.npz, tools/gen_fit_golden.py), the run-folder / --resume resolution follows
train_ddp_v3mod2.py:397-424, 622-660, the parser's defaults are the reference TrainConfig's, and the two new C entry points
are declared and bound."""
import math
import os
import re
from datetime import datetime

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, Dataset
from torch.utils.data.distributed import DistributedSampler

from jatsr_amd import _lib
from jatsr_amd import data as D
from jatsr_amd import fit as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Indices(Dataset):
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return i


def torch_batches(n, batch, epoch, rank, world, shuffle, seed=0):
    ds = _Indices(n)
    sampler = DistributedSampler(ds, num_replicas=world, rank=rank, shuffle=shuffle, seed=seed)
    sampler.set_epoch(epoch)
    return [b.tolist() for b in DataLoader(ds, batch_size=batch, sampler=sampler, drop_last=True)]


def test_epoch_batches_example():
    assert D.epoch_batches(23, 1, 4, epoch=3, rank=1, world=2, shuffle=True, seed=0) == \
        [[9, 10, 17, 2], [16, 14, 22, 20], [5, 19, 8, 12]]


@pytest.mark.parametrize("n_files,mult", [(23, 1), (4, 6), (28, 6)])       # 23, 24, 168 samples
@pytest.mark.parametrize("world", [1, 2, 8])
@pytest.mark.parametrize("epoch", [0, 3])
@pytest.mark.parametrize("shuffle", [True, False])
def test_epoch_batches_equal_torch(n_files, mult, world, epoch, shuffle):
    for rank in range(world):
        for batch, seed in ((4, 0), (3, 42)):
            got = D.epoch_batches(n_files, mult, batch, epoch, rank, world, shuffle, seed)
            assert got == torch_batches(n_files * mult, batch, epoch, rank, world, shuffle, seed), (rank, batch, seed)


@pytest.mark.parametrize("n,world", [(23, 2), (23, 8), (24, 8), (168, 8), (3, 8)])
def test_shards_cover_padded_list_once(n, world):
    total = math.ceil(n / world) * world
    g = torch.Generator()
    g.manual_seed(5 + 2)
    perm = torch.randperm(n, generator=g).tolist()
    padded = (perm * math.ceil(total / n))[:total]
    shards = [sum(D.epoch_batches(n, 1, 1, 2, r, world, True, seed=5), []) for r in range(world)]
    assert all(len(s) == total // world for s in shards)
    assert [shards[i % world][i // world] for i in range(total)] == padded


def test_val_crop_start_and_short_map_equal_golden(golden_dir):
    z = np.load(os.path.join(golden_dir, "fit_crops.npz"))
    assert len(z["val_cases"]) > 100
    kinds = set()
    for (length, frames, mult, k), start in zip(z["val_cases"].tolist(), z["val_start"].tolist()):
        assert D.val_crop_start(length, frames, mult, k) == start, (length, frames, mult, k)
        kinds.add((length == frames, length == frames + 1, length > 2 * frames, mult))
    assert len(kinds) >= 6                                     # == frames, frames + 1, long; multipliers 1 and 6
    for length, frames in z["short_cases"].tolist():
        assert length < frames and D.val_crop_start(length, frames, 6, 3) == 0 and D.train_crop_start(length, frames, 1, 2, 3) == 0
        want = z[f"short_map_{frames}_{length}"]
        assert ((0 + np.arange(frames)) % length == want).all()         # the kernel's (start + j) mod len with start 0
    files, starts = D.val_batch_plan([1378, 5000, 20], 1378, [0, 1, 2, 4, 5, 16], 6)
    assert files == [0, 1, 2, 1, 2, 1] and starts == [0, 0, 0, D.val_crop_start(5000, 1378, 6, 1), 0, 5000 - 1378]


def test_train_crop_start():
    T = 1378
    for length in (T, T + 1, T + 7, 5000, 100000):
        s = [D.train_crop_start(length, T, 42, e, i) for e in range(3) for i in range(400)]
        assert min(s) >= 0 and max(s) <= length - T
        assert s == [D.train_crop_start(length, T, 42, e, i) for e in range(3) for i in range(400)]     # reproducible
        if length >= T + 7:
            assert s[:400] != s[400:800] != s[800:]                                                       # differs by epoch
            assert len(set(s)) > min(length - T, 400) // 2
            assert [D.train_crop_start(length, T, 43, 0, i) for i in range(400)] != s[:400]              # and by seed
    # uniform: every start of a short range is hit about equally often
    counts = np.bincount([D.train_crop_start(T + 9, T, 7, 0, i) for i in range(20000)], minlength=10)
    assert counts.min() > 1700 and counts.max() < 2300
    files, starts = D.train_batch_plan([T + 50, 10, T], T, [0, 1, 2, 3], 42, 1)
    assert files == [0, 1, 2, 0] and starts[1] == 0 and starts[2] == 0 and starts[0] != starts[3]
    assert "random.randint" in D.train_crop_start.__doc__ and "resume" in D.train_crop_start.__doc__


def test_run_folder_and_resume_resolution(tmp_path):
    base = str(tmp_path / "ck")
    now = datetime(2025, 3, 7, 14, 5)
    assert F.find_latest_checkpoint_dir(base) == (None, None)
    assert F.resolve_run_dir(base, None, now) == (os.path.join(base, "03071405"), None)
    assert F.resolve_run_dir(base, "auto", now) == (os.path.join(base, "03071405"), None)       # nothing to resume: new run
    for name in ("01010000", "02020000", "notadate", "1234567", "123456789"):
        os.makedirs(os.path.join(base, name))
    open(os.path.join(base, "03030000"), "w").close()                                          # a FILE with an 8-digit name
    assert F.find_latest_checkpoint_dir(base) == (os.path.join(base, "02020000"), None)
    open(os.path.join(base, "01010000", "last.pt"), "w").close()
    # the reference looks at the newest folder only (:416-424): without last.pt there, a new run starts
    assert F.resolve_run_dir(base, "auto", now) == (os.path.join(base, "03071405"), None)
    last = os.path.join(base, "02020000", "last.pt")
    open(last, "w").close()
    assert F.find_latest_checkpoint_dir(base) == (os.path.join(base, "02020000"), last)
    assert F.resolve_run_dir(base, "auto", now) == (os.path.join(base, "02020000"), last)
    assert F.resolve_run_dir(base, None, now) == (os.path.join(base, "03071405"), None)
    interval = os.path.join(base, "01010000", "interval_step_2000.pt")
    open(interval, "w").close()
    assert F.resolve_run_dir(base, interval, now) == (os.path.join(base, "01010000"), interval)
    with pytest.raises(FileNotFoundError):
        F.resolve_run_dir(base, os.path.join(base, "nope.pt"), now)
    assert re.fullmatch(r"\d{8}", os.path.basename(F.resolve_run_dir(base, None)[0]))


def test_parser_defaults_are_trainconfig():
    a = F.build_parser().parse_args([])
    # train_ddp_v3mod2.py:327-386
    assert (a.seed, a.data_dir, a.stats_file, a.frames) == (42, "data_processed_v13_final", "global_stats_separated.json", 1378)
    assert (a.batch_size, a.lr, a.weight_decay, a.warmup_steps, a.epochs, a.grad_clip) == (28, 5e-5, 0.1, 1000, 300, 1.0)
    assert (a.condition_noise_ratio, a.use_adaptive_noise, a.latent_loss_weight, a.loss) == (0.05, True, 0.3, "mse")
    assert (a.save_dir_base, a.save_interval_steps, a.log_interval) == ("checkpoints/v3mod2_full_run", 1000, 10)
    assert (a.samples_per_epoch_multiplier, a.resume, a.max_steps, a.cfg_dropout_prob) == (6, None, None, 0.0)
    assert a.model == "v2" and F.model_config(a) == dict(
        input_channels=1024, cond_channels=1024, patch_len=4, hidden_size=1280, depth=28, num_q_heads=20, num_kv_heads=4,
        bottleneck_dim=512, mlp_ratio=4.0, dropout=0.1, drop_path_rate=0.05)
    assert F.build_parser().parse_args(["--resume"]).resume == "auto"
    assert F.build_parser().parse_args(["--resume", "x/last.pt"]).resume == "x/last.pt"
    b = F.build_parser().parse_args(["--preset", "micro", "--depth", "3", "--model", "v3"])
    assert F.model_config(b)["depth"] == 3 and F.model_config(b)["input_channels"] == F.model_config(b)["cond_channels"] == 32


def test_bad_loss_is_an_argument_error_before_anything_else(tmp_path):
    a = F.build_parser().parse_args(["--loss", "charbonier", "--data-dir", str(tmp_path)])
    with pytest.raises(ValueError, match="loss must be"):
        F.run(a)
    a = F.build_parser().parse_args(["--loss", "charbonnier", "--data-dir", str(tmp_path)])       # latent weight left at 0.3
    with pytest.raises(ValueError, match="latent"):
        F.run(a)
    from jatsr_amd.train import Trainer
    with pytest.raises(ValueError, match="loss must be"):      # checked ahead of the GPU requirement and of any allocation
        Trainer(None, 1, 4, loss="huber")


def test_new_symbols_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "jat_hip.h")).read()
    for name in ("jat_latent_gather", "jat_train_monitor"):
        assert re.search(r"\bint %s\(" % name, header) and name in _lib.SIGNATURES
    assert "train_ddp_v3mod2.py:509-535" in header and "train_ddp_v3mod2.py:902-919" in header
    assert int(re.search(r"#define JAT_MONITOR_WORK_BYTES (\d+)", header).group(1)) == _lib.MONITOR_WORK_BYTES
    mk = open(os.path.join(ROOT, "jatsr-just-audio-transformer-super-solution_amd", "csrc", "Makefile")).read()
    assert "data.o jat_data.o" in mk and "data_fp16.o jat_data_fp16.o" in mk
    import jatsr_amd
    for name in ("LatentStore", "epoch_batches", "val_crop_start", "train_crop_start", "resolve_run_dir", "train_monitor"):
        assert name in jatsr_amd.__all__
