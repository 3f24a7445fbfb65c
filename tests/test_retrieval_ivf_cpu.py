"""Host side of the IVF index, no GPU: the four entry points are declared in include/jat_hip_ivf.h (and in no other
header), bound in `_lib.IVF_SIGNATURES` and exported from both libraries; the fp64 statement of tests/retrieval_ivf_ref.py on
examples worked by hand; RVC's default number of lists; the file format (format 3 round trip, formats 1 and 2 read as before);
the command line; the refusals that come before any device call; and the margins of the fixtures the GPU tests share: at most
FP64_LOOSE ranks of a case inside the near-tie allowance, no assignment of a fixture row inside it, and the planted fixture's
k-means seeds in six different clusters."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import jatsr_amd
import retrieval_ivf_ref as IVF
import retrieval_ref as R
from jatsr_amd import _lib
from jatsr_amd import retrieval as RT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jatsr-just-audio-transformer-super-solution_amd", "csrc")
SYMBOLS = ("jat_bank_group_workspace_bytes", "jat_bank_group", "jat_ivf_search_workspace_bytes", "jat_ivf_search")


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


# ---- symbols ------------------------------------------------------------------------------------------------------------
def test_symbols_declared_bound_and_exported(built):
    header = open(os.path.join(ROOT, "include", "jat_hip_ivf.h")).read()
    old = "".join(open(os.path.join(ROOT, "include", h)).read() for h in ("jat_hip.h", "jat_hip_ms.h", "jat_hip_harm.h", "jat_hip_km.h"))
    assert '#include "jat_hip.h"' in header
    others = (_lib.SIGNATURES, _lib.MS_SIGNATURES, _lib.HARM_SIGNATURES, _lib.KM_SIGNATURES)
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.IVF_SIGNATURES and not any(name in t for t in others), name
        assert name not in old, name
        assert getattr(built, name).argtypes == _lib.IVF_SIGNATURES[name][1]
    assert set(re.findall(r"\bint (jat_[a-z0-9_]+)\(", header)) == set(_lib.IVF_SIGNATURES) == set(SYMBOLS)
    assert int(re.search(r"#define JAT_IVF_MAX_NPROBE (\d+)", header).group(1)) == _lib.IVF_MAX_NPROBE == IVF.MAX_NPROBE == 8
    assert int(re.search(r"#define JAT_IVF_MAX_ROWS (\d+)", header).group(1)) == _lib.IVF_MAX_ROWS == _lib.KM_MAX_POOL
    assert [len(_lib.IVF_SIGNATURES[n][1]) for n in SYMBOLS] == [3, 9, 6, 16]
    for so in ("libjat_hip.so", "libjat_hip_fp16.so"):
        nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(CSRC, so)], capture_output=True, text=True,
                            check=True).stdout
        exported = set(re.findall(r" T (jat_[a-z0-9_]+)", nm))
        assert set(SYMBOLS) <= exported, (so, set(SYMBOLS) - exported)
    assert "IVFBank" in jatsr_amd.__all__
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "OBJS += retrieval_ivf.o jat_retrieval_ivf.o\n" in mk and "FP16OBJS += retrieval_ivf_fp16.o jat_retrieval_ivf_fp16.o\n" in mk
    assert mk.count("../../include/jat_hip_ivf.h") == 2              # the two %.cpp pattern rules
    assert mk.count("jat_retrieval_ivf_kernels.h") == 4               # every pattern rule
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "_lib.IVF_SIGNATURES" in entry                             # build() checks the new symbols in both libraries


def test_argument_errors_need_no_gpu(built):
    INV = _lib.JAT_E_INVALID
    n = ctypes.c_size_t()
    assert built.jat_bank_group_workspace_bytes(None, 3, ctypes.byref(n)) == INV
    assert b"null bank" in built.jat_last_error()
    assert built.jat_bank_group(None, None, 3, None, None, None, None, 0, None) == INV
    assert built.jat_ivf_search_workspace_bytes(None, None, 10, 1, 1, ctypes.byref(n)) == INV
    assert built.jat_ivf_search(None, None, None, None, None, None, 1, 1, 1, 1, None, None, None, None, 0, None) == INV
    assert b"null bank" in built.jat_last_error()
    for bad in (0, 9, True, 2.0, None, "3"):
        with pytest.raises(ValueError, match="nprobe"):
            RT.check_nprobe(bad)
    assert [RT.check_nprobe(v) for v in (1, 8)] == [1, 8]
    with pytest.raises(ValueError, match="rows"):
        RT.default_nlist(0)
    for bad in ([0, 3, 2, 5], [1, 2, 5], [0, 2, 4], [0, 5]):              # descending, not from 0, not to N, wrong length
        with pytest.raises(ValueError, match="offsets"):
            RT.check_offsets(torch.tensor(bad, dtype=torch.int32), 3, 5)
    assert RT.check_offsets([0, 0, 5, 5], 3, 5).dtype == torch.int32


def test_command_line():
    p = RT.build_parser()
    a = p.parse_args(["build", "--data-dir", "d", "--out", "o", "--ivf", "--ivf-lists", "7", "--ivf-nprobe", "2"])
    assert a.ivf and a.ivf_lists == 7 and a.ivf_nprobe == 2
    a = p.parse_args(["build", "--data-dir", "d", "--out", "o"])
    assert not a.ivf and a.ivf_lists is None and a.ivf_nprobe is None
    for bad in ("0", "9", "x"):
        with pytest.raises(SystemExit):
            p.parse_args(["build", "--data-dir", "d", "--out", "o", "--ivf", "--ivf-nprobe", bad])
    assert "out of scope" in p._subparsers._group_actions[0].choices["build"].format_help()
    from jatsr_amd.infer import build_parser as infer_parser
    assert infer_parser().parse_args(["--index-nprobe", "4"]).index_nprobe == 4
    assert infer_parser().parse_args([]).index_nprobe is None


# ---- the fp64 statement on examples worked by hand ---------------------------------------------------------------------------
def test_default_nlist():
    # int(16 sqrt(N)) against N // 39: the second decides below N = 389 376, the floor below N = 39
    assert [IVF.default_nlist(n) for n in (1, 38, 39, 100, 2000, 100_000, 389_376, 1_000_000, 2 ** 22)] == \
        [1, 1, 1, 2, 51, 2564, 9984, 16000, 32768]
    for n in (1, 38, 39, 77, 78, 2000, 12345, 100_000, 389_375, 389_377, 1_000_000, 2 ** 22):
        assert RT.default_nlist(n) == IVF.default_nlist(n) and 1 <= RT.default_nlist(n) <= n


def test_grouping_by_hand():
    offsets, order = IVF.group([2, 0, 2, 7, 0, -1, 2], 3)
    assert offsets.tolist() == [0, 2, 2, 5] and order.tolist() == [1, 4, 0, 2, 6, 3, 5]      # list 1 empty; rows 3 and 5 behind
    offsets, order = IVF.group([0, 0, 0], 1)
    assert offsets.tolist() == [0, 3] and order.tolist() == [0, 1, 2]


def test_search_by_hand():
    # two lists over five positions: list 0 = positions 0, 1; list 1 = positions 2, 3, 4
    offsets = np.array([0, 2, 5], np.int32)
    dc = np.array([[1.0, 2.0], [3.0, 3.0], [5.0, 4.0]])
    assert IVF.probes(dc, 1).tolist() == [[0], [0], [1]]                                      # equal distance: the lower list
    assert IVF.probes(dc, 3).tolist() == [[0, 1, -1], [0, 1, -1], [1, 0, -1]]
    d = np.array([[4.0, 1.0, 0.5, 9.0, 9.0], [2.0, 2.0, 2.0, -1.0, 2.0], [7.0, 7.0, 3.0, 3.0, 1.0]])
    idx, dist2 = IVF.search(d, offsets, IVF.probes(dc, 1), 3)
    assert idx.tolist() == [[1, 0, -1], [0, 1, -1], [4, 2, 3]]                                # query 0 misses position 2 (0.5)
    assert dist2.tolist() == [[1.0, 4.0, np.inf], [2.0, 2.0, np.inf], [1.0, 3.0, 3.0]]
    idx, dist2 = IVF.search(d, offsets, IVF.probes(dc, 2), 3)
    assert idx.tolist() == [[2, 1, 0], [3, 0, 1], [4, 2, 3]] and dist2[1].tolist() == [0.0, 2.0, 2.0]   # max(d, 0)
    idx, _ = IVF.search(d, np.array([0, 0, 5], np.int32), np.array([[0], [-1], [1]], np.int32), 2)
    assert idx.tolist() == [[-1, -1], [-1, -1], [4, 2]]                                       # an empty list, no list
    assert IVF.candidates(offsets, [1, 0]).tolist() == [0, 1, 2, 3, 4]
    loose = IVF.undecided(d, offsets, IVF.probes(dc, 2), 3, 0.5)
    assert loose.tolist() == [[True, True, False], [False, True, True], [False, True, True]]


# ---- the fixtures the GPU tests share ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(IVF.FP64_CASES))
def test_fixture_margins(name):
    c = IVF.fp64_case(name)
    C, nlist, N, B, T, nprobe, k = IVF.FP64_CASES[name]
    assert N <= 2000 and B * T <= 70 and C in (32, 96, 1024)
    assert (c["assign_gap"] > 100 * c["assign_tol"]).all()              # no row's list hangs on fp32 rounding
    sizes = np.diff(c["offsets"])
    assert c["offsets"][-1] == N and sizes.min() >= 1
    loose = int(c["loose"].sum()) + int(c["probes_loose"].sum())
    print(f"{name}: {loose} ranks inside the near-tie allowance (tol {c['tol']:.3g}), lists of {sizes.min()}..{sizes.max()} rows")
    assert loose <= IVF.FP64_LOOSE
    assert (c["idx"][:, 0] >= 0).all()


def test_default_lists_of_the_mid_case():
    assert IVF.FP64_CASES["mid"][1] == IVF.default_nlist(IVF.FP64_CASES["mid"][2]) == 51


def test_planted_fixture_and_its_seeds():
    p = IVF.planted()
    C, K, N = IVF.PLANTED
    seeds = IVF.planted_seeds()
    assert seeds == RT.seed_positions(N, K) and sorted(p["member"][seeds].tolist()) == list(range(K))
    # every query finds its own row at nprobe = 1, in fp64
    q = R.queries(p["x"])
    offsets, order = IVF.group(p["member"], K)
    grouped = p["rows"][order]
    dc, d = R.dist(q, p["centres"], np.float64), R.dist(q, grouped, np.float64)
    pr = IVF.probes(dc, 1)
    assert (pr[:, 0] == p["member"][p["own"]]).all()
    idx, _ = IVF.search(d, offsets, pr, 1)
    assert (order[idx[:, 0]] == p["own"]).all()
    two = np.sort(d, axis=1)[:, :2]
    assert ((two[:, 1] - two[:, 0]) > 0.5).all()                         # far from any tie
    # the rows' own assignment has the planted margin too: (16^2 + 16^2) between centres against 0.25^2 C of noise
    a = R.reference(p["rows"].astype(np.float32), p["centres"])
    assert (a["argmin"] == p["member"]).all() and (a["gap"] > 100).all()


# ---- files ----------------------------------------------------------------------------------------------------------------
def small_state():
    p = IVF.planted()
    C, K, N = IVF.PLANTED
    offsets, order = IVF.group(p["member"], K)
    st = {k: torch.from_numpy(v) for k, v in R.stats(C, 5).items()}
    bank = RT.pack_state(torch.from_numpy(p["rows"][order].copy()), None, "hr", st)
    return bank, torch.from_numpy(p["centres"].copy()), torch.from_numpy(offsets), torch.from_numpy(order)


def test_file_format(tmp_path):
    bank, cent, offsets, order = small_state()
    d = RT.pack_ivf_state(bank, cent, offsets, order, 2)
    assert d["format"] == RT.FORMAT_IVF == 3 and d["nprobe"] == 2 and d["bank"]["format"] == RT.FORMAT == 1
    torch.save(d, tmp_path / "ivf.pt")
    b2, c2, o2, r2, np2 = RT.unpack_ivf_state(torch.load(tmp_path / "ivf.pt", weights_only=False))
    assert torch.equal(b2["keys"], bank["keys"]) and torch.equal(c2, cent) and torch.equal(o2, offsets) and torch.equal(r2, order)
    assert np2 == 2 and o2.dtype == r2.dtype == torch.int32
    # the bank inside is a valid format-1 dictionary; formats 1 and 2 are read as before; format 3 is refused by their readers
    keys, values, key, channels, _ = RT.unpack_state(d["bank"])
    assert torch.equal(keys, bank["keys"]) and values is None and key == "hr" and channels == IVF.PLANTED[0]
    ms = RT.pack_ms_state((1, 2), RT.check_scale_weights(None, 2), [bank, bank])
    assert RT.unpack_ms_state(ms)[0] == (1, 2)
    with pytest.raises(ValueError, match="IVF index"):
        RT.unpack_state(d)
    with pytest.raises(ValueError, match="not a multi-scale"):
        RT.unpack_ms_state(d)
    with pytest.raises(ValueError, match="not an IVF index"):
        RT.unpack_ivf_state(bank)
    with pytest.raises(ValueError, match="not an IVF index"):
        RT.unpack_ivf_state(ms)
    for k in ("bank", "centroids", "offsets", "order", "nprobe"):
        with pytest.raises(KeyError, match=k):
            RT.unpack_ivf_state({a: b for a, b in d.items() if a != k})
    bad_order = order.clone()
    bad_order[0] = bad_order[1]
    for args, what in (((bank, cent.float(), offsets, order, 1), "centroids"), ((bank, cent[:, :16], offsets, order, 1), "centroids"),
                       ((bank, cent, offsets[:-1], order, 1), "offsets"), ((bank, cent, offsets, bad_order, 1), "permutation"),
                       ((bank, cent, offsets, order[:-1], 1), "permutation"), ((bank, cent, offsets, order, 9), "nprobe")):
        with pytest.raises(ValueError, match=what):
            RT.pack_ivf_state(*args)
