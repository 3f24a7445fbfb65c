#!/usr/bin/env python3
"""Fixture of the training data set's index arithmetic (CPU only): tests/golden/fit_crops.npz.

The reference's `LatentDataset.__getitem__` and `ValidationDataset.__getitem__` (train_ddp_v3mod2.py:476-597) are taken out
of the reference's source at run time (its module imports TensorBoard and the model, which this needs not) and run on
files whose latents hold their own frame index, hr_latent[c, j] = j: what comes back is the index map of the crop.
  val_cases  int64 [n, 4]  (length, frames, multiplier, sample_idx);  val_start int64 [n]  the first index of the crop
  short_cases int64 [m, 2] (length, frames);  short_map_<frames>_<length> int32 [frames]  the loop-repeat index map
    python tools/gen_fit_golden.py --reference /path/to/reference [--out tests/golden] [--check]"""
import argparse
import ast
import math
import os
import random
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = (1378, 512, 37)
# lengths: below frames, equal, frames + 1, long; odd and even
VAL_LENGTHS = lambda T: [1, 5, T - 1, T, T + 1, T + 2, 2 * T + 3, 5 * T, 7 * T + 11]   # noqa: E731
SHORT_LENGTHS = lambda T: sorted({1, 5, min(500, T - 1), T - 1})                       # noqa: E731
MULTIPLIERS = (1, 6)


def reference_classes(reference):
    import torch
    from torch.utils.data import Dataset
    src = open(os.path.join(reference, "train_ddp_v3mod2.py"), encoding="utf-8").read()
    want = [n for n in ast.parse(src).body if isinstance(n, ast.ClassDef) and n.name in ("LatentDataset", "ValidationDataset")]
    assert len(want) == 2, "the reference no longer defines both data sets"
    ns = dict(torch=torch, Dataset=Dataset, Path=Path, math=math, random=random, print=lambda *a, **k: None)
    exec(compile(ast.Module(body=want, type_ignores=[]), "train_ddp_v3mod2.py", "exec"), ns)
    return ns["LatentDataset"], ns["ValidationDataset"]


def index_file(folder, length):
    import torch
    idx = torch.arange(length, dtype=torch.int32).repeat(2, 1)
    torch.save({"hr_latent": idx, "lr_latent": idx.clone()}, os.path.join(folder, "a.pt"))


def build(reference):
    LatentDataset, ValidationDataset = reference_classes(reference)
    out, val_cases, val_start, short_cases = {}, [], [], []
    for T in FRAMES:
        for length in VAL_LENGTHS(T):
            for mult in MULTIPLIERS:
                with tempfile.TemporaryDirectory() as d:
                    os.makedirs(os.path.join(d, "val"))
                    index_file(os.path.join(d, "val"), length)
                    ds = ValidationDataset(d, "val", T, samples_per_epoch_multiplier=mult)
                    for k in range(mult):
                        hr, lr = ds[k]
                        m = hr[0].numpy().astype(np.int64)
                        assert hr.shape == (2, T) and (hr == lr).all()
                        if length >= T:
                            assert (np.diff(m) == 1).all()
                            val_cases.append((length, T, mult, k))
                            val_start.append(int(m[0]))
                        else:
                            assert (m == np.arange(T) % length).all()      # the loop-repeat starts at frame 0
        for length in SHORT_LENGTHS(T):
            with tempfile.TemporaryDirectory() as d:
                os.makedirs(os.path.join(d, "train"))
                index_file(os.path.join(d, "train"), length)
                hr, _ = LatentDataset(d, "train", T, samples_per_epoch_multiplier=1)[0]
                short_cases.append((length, T))
                out[f"short_map_{T}_{length}"] = hr[0].numpy().astype(np.int32)
    out["val_cases"] = np.array(val_cases, np.int64)
    out["val_start"] = np.array(val_start, np.int64)
    out["short_cases"] = np.array(short_cases, np.int64)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="folder that holds train_ddp_v3mod2.py")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    got = build(args.reference)
    path = os.path.join(args.out, "fit_crops.npz")
    if args.check:
        have = np.load(path)
        assert sorted(have.files) == sorted(got) and all((have[k] == got[k]).all() for k in got), "fixture differs"
        print(f"{path}: matches")
        return 0
    np.savez_compressed(path, **got)
    print(f"wrote {path}: {len(got['val_start'])} validation cases, {len(got['short_cases'])} short clips")
    return 0


if __name__ == "__main__":
    sys.exit(main())
