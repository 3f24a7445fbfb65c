"""Host side of latent retrieval (jatsr_amd.retrieval), no GPU: the C entry points are declared, bound and exported from both
libraries, the Makefile lists the objects, `frame_plan` keeps its count bound and is deterministic, the index rate is
validated before anything runs, and a bank dictionary survives a save / load round trip on CPU tensors."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import jatsr_amd
import retrieval_ref as R
from jatsr_amd import _lib, infer
from jatsr_amd import retrieval as RT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jatsr-just-audio-transformer-super-solution_amd", "csrc")
SYMBOLS = ("jat_bank_create", "jat_bank_destroy", "jat_bank_size", "jat_bank_clear", "jat_bank_add", "jat_bank_rows",
           "jat_bank_load_rows", "jat_bank_search_workspace_bytes", "jat_bank_search", "jat_bank_blend")


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


def test_symbols_declared_bound_and_exported(built):
    header = open(os.path.join(ROOT, "include", "jat_hip.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b(int|void) %s\(" % name, header), name
        assert name in _lib.SIGNATURES, name
    assert int(re.search(r"#define JAT_BANK_SLAB (\d+)", header).group(1)) == _lib.BANK_SLAB
    for so in ("libjat_hip.so", "libjat_hip_fp16.so"):
        nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(CSRC, so)], capture_output=True, text=True,
                            check=True).stdout
        exported = set(re.findall(r" T (jat_[a-z0-9_]+)", nm))
        assert set(SYMBOLS) <= exported, (so, set(SYMBOLS) - exported)
    for name in ("LatentBank", "frame_plan"):
        assert name in jatsr_amd.__all__


def test_makefile_lists_the_objects():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "jat_data.o retrieval.o jat_retrieval.o\n" in mk
    assert "jat_data_fp16.o retrieval_fp16.o jat_retrieval_fp16.o\n" in mk
    assert mk.count("jat_retrieval_kernels.h") == 4            # the four pattern rules' dependency lines


def test_argument_errors_need_no_gpu(built):
    """what jat_retrieval.cpp refuses ahead of any device call"""
    h = ctypes.c_void_p()
    for channels in (48, 0, 16, 1056):
        assert built.jat_bank_create(channels, 10, 0, ctypes.byref(h)) == _lib.JAT_E_INVALID and not h.value
    assert built.jat_bank_create(32, 0, 0, ctypes.byref(h)) == _lib.JAT_E_INVALID
    assert built.jat_bank_create(32, 10, 0, None) == _lib.JAT_E_INVALID
    n = ctypes.c_int32()
    assert built.jat_bank_size(None, ctypes.byref(n)) == _lib.JAT_E_INVALID
    assert built.jat_bank_search(None, None, None, None, 1, 1, None, None, None, 0, None) == _lib.JAT_E_INVALID
    assert b"null bank" in built.jat_last_error()


def covered(lengths, plan):
    """global positions of the frames a plan names"""
    pos, off = [], 0
    for n, (first, stride, count) in zip(lengths, plan):
        assert 0 <= first and stride >= 1 and count >= 0
        assert count == 0 or first + (count - 1) * stride < n
        pos += [off + first + i * stride for i in range(count)]
        off += n
    return pos


@pytest.mark.parametrize("lengths,max_frames", [([100, 1, 37, 250], 50), ([100, 1, 37, 250], 387), ([100, 1, 37, 250], 388),
                                                ([100, 1, 37, 250], 10 ** 6), ([1], 1), ([1, 1, 1, 1, 1], 2), ([7, 0, 9], 3),
                                                ([1378] * 9 + [478], 1000), ([5], 1)])
def test_frame_plan(lengths, max_frames):
    plan = RT.frame_plan(lengths, max_frames)
    total = sum(lengths)
    s = max(1, -(-total // max_frames))
    assert len(plan) == len(lengths) and all(p[1] == s for p in plan)
    pos = covered(lengths, plan)
    assert pos == list(range(0, total, s))                       # the multiples of s in the concatenation, in order
    assert len(pos) == -(-total // s) <= max_frames
    assert RT.frame_plan(list(lengths), max_frames) == plan      # deterministic
    if max_frames >= total:
        assert s == 1 and [c for _, _, c in plan] == lengths


def test_frame_plan_single_frame_file_and_errors():
    assert RT.frame_plan([1], 5) == [(0, 1, 1)]
    plan = RT.frame_plan([3, 1, 3], 3)                            # stride 3: positions 0, 3, 6 -> the single-frame file is position 3
    assert plan == [(0, 3, 1), (0, 3, 1), (2, 3, 1)]
    assert RT.frame_plan([2, 1, 3], 2) == [(0, 3, 1), (1, 3, 0), (0, 3, 1)]      # a file no multiple falls into
    with pytest.raises(ValueError):
        RT.frame_plan([4], 0)


@pytest.mark.parametrize("rate", [-0.1, 1.0001, float("nan"), float("inf"), 2])
def test_index_rate_is_validated_before_anything_runs(rate):
    with pytest.raises(ValueError, match="index_rate"):
        # no model, no latent, no GPU: the check comes first
        jatsr_amd.sample_long(None, None, None, None, None, None, bank=object(), index_rate=rate)
    with pytest.raises(ValueError, match="index_rate"):
        RT.check_index_rate(rate)
    with pytest.raises(SystemExit):
        infer.build_parser().parse_args(["--index-bank", "b.pt", "--index-rate", str(rate)])


def test_cli_parsers():
    a = infer.build_parser().parse_args([])
    assert a.index_bank is None and a.index_rate == 0.4
    a = infer.build_parser().parse_args(["--index-bank", "bank.pt", "--index-rate", "0.55"])
    assert a.index_bank == "bank.pt" and a.index_rate == 0.55
    for ok in ("0", "1", "0.3"):
        assert infer.build_parser().parse_args(["--index-rate", ok]).index_rate == float(ok)
    b = RT.build_parser().parse_args(["build", "--data-dir", "D", "--out", "bank.pt"])
    assert (b.command, b.data_dir, b.out, b.stats_file, b.max_frames, b.key, b.split) == ("build", "D", "bank.pt", None, 100_000,
                                                                                          "hr", "train")
    b = RT.build_parser().parse_args(["build", "--data-dir", "D", "--out", "o.pt", "--key", "lr", "--max-frames", "7",
                                      "--stats-file", "s.json"])
    assert (b.key, b.max_frames, b.stats_file) == ("lr", 7, "s.json")
    with pytest.raises(SystemExit):
        RT.build_parser().parse_args(["build", "--data-dir", "D", "--out", "o.pt", "--key", "both"])


@pytest.mark.parametrize("key", ["hr", "lr"])
def test_bank_dictionary_round_trip(tmp_path, key):
    C, N = 32, 11
    st = {k: torch.from_numpy(v) for k, v in R.stats(C, 4).items()}
    keys = torch.from_numpy(R.pack_rows(np.asarray(jatsr_amd.recipe.gaussian("rt_cpu", (C, N), 1)), st["hr_mean"].numpy(),
                                        st["hr_std"].numpy()))
    values = torch.flip(keys, dims=[0]).contiguous() if key == "lr" else None
    d = RT.pack_state(keys, values, key, st)
    torch.save(d, tmp_path / "bank.pt")
    k2, v2, key2, C2, st2 = RT.unpack_state(torch.load(tmp_path / "bank.pt", map_location="cpu", weights_only=False))
    assert key2 == key and C2 == C and k2.dtype == torch.float16 and torch.equal(k2, keys)
    assert (v2 is None) if key == "hr" else torch.equal(v2, values)
    assert RT.same_stats(st, st2) and all(st2[k].dtype == torch.float32 for k in RT.STAT_KEYS)
    other = dict(st, hr_std=st["hr_std"] + 1e-3)
    assert not RT.same_stats(other, st2)
    with pytest.raises(ValueError):
        RT.pack_state(keys, keys if key == "hr" else None, key, st)      # values exactly when key == "lr"
    with pytest.raises(ValueError):
        RT.pack_state(keys.float(), values, key, st)
    with pytest.raises(KeyError):
        RT.unpack_state({k: v for k, v in d.items() if k != "stats"})
    with pytest.raises(ValueError):
        RT.unpack_state(dict(d, channels=64))
