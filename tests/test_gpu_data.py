"""Batch assembly and the step monitor on the GPU (csrc/data.hip, jatsr_amd.data.LatentStore): `jat_latent_gather` has the
bits of the composed path stack -> .float() -> channel_affine for every alignment case, repeats short clips by the golden
index map, writes nothing outside its outputs, and a store that keeps most files in pinned host memory returns the same bits
as a fully resident one; `jat_train_monitor` is within the fp64 summation bound of numpy and repeats bit for bit."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import jatsr_amd.io as jio  # noqa: E402
from jatsr_amd import _lib as L  # noqa: E402
from jatsr_amd.data import LatentStore  # noqa: E402
from jatsr_amd.sampler import channel_affine  # noqa: E402
from jatsr_amd.train import monitor_figures, train_monitor  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 64            # floats of canary either side of an output tensor (keeps it 256-byte aligned)
CANARY = -1234.5


def bits(x):
    return x.contiguous().view(torch.int32)


def make_src(C_, length, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(C_, length, generator=g) * 3).to(torch.float16)
    flat = x.view(-1)
    special = torch.tensor([0.0, -0.0, 6e-8, -6e-8, 65504.0, -65504.0, 1.0, 6.1e-5], dtype=torch.float16)   # +-0, subnormals, max
    flat[:min(8, flat.numel())] = special[:min(8, flat.numel())]
    return x


def make_stats(C_, seed=7):
    g = torch.Generator().manual_seed(seed)
    return {"hr_mean": torch.randn(C_, generator=g).cuda(), "hr_std": (torch.rand(C_, generator=g) * 2 + 0.3).cuda(),
            "lr_mean": torch.randn(C_, generator=g).cuda(), "lr_std": (torch.rand(C_, generator=g) * 2 + 0.3).cuda()}


def guarded_pair(B, C_, T):
    n = B * C_ * T
    n_al = (n + 3) // 4 * 4
    flat = torch.full((PAD + n_al + PAD + n_al + PAD,), CANARY, dtype=torch.float32, device="cuda")
    hr = flat[PAD:PAD + n].view(B, C_, T)
    lr = flat[2 * PAD + n_al:2 * PAD + n_al + n].view(B, C_, T)
    guards = [flat[:PAD], flat[PAD + n:2 * PAD + n_al], flat[2 * PAD + n_al + n:]]
    return flat, hr, lr, guards


def gather(hr_src, lr_src, starts, T, stats, out=None):
    """jat_latent_gather through ctypes on device tensors hr_src[b] / lr_src[b] (fp16 [C, len_b])."""
    B, C_ = len(hr_src), hr_src[0].shape[0]
    table = torch.tensor([[x.data_ptr() for x in hr_src], [x.data_ptr() for x in lr_src],
                          [x.shape[1] for x in hr_src], list(starts)], dtype=torch.int64).cuda()
    if out is None:
        out = (torch.empty(B, C_, T, device="cuda"), torch.empty(B, C_, T, device="cuda"))
    vec = [stats[k] if stats is not None else None for k in ("hr_mean", "hr_std", "lr_mean", "lr_std")]
    L.check(L.lib().jat_latent_gather(L.ptr(table[0]), L.ptr(table[1]), L.ptr(table[2]), L.ptr(table[3]), *[L.ptr(v) for v in vec],
                                      L.ptr(out[0]), L.ptr(out[1]), B, C_, T, L.stream_ptr()))
    torch.cuda.synchronize()
    return out


def composed(srcs, starts, T, mean, std):
    x = torch.stack([s[:, a:a + T] for s, a in zip(srcs, starts)]).float()
    return channel_affine(x, mean, std) if mean is not None else x


def batch_layout(B, T):
    """lengths and starts of B samples: even / odd lengths, even / odd starts, start 0, start = len - T, len == T"""
    lengths, starts = [], []
    for b in range(B):
        length = T + (0, 1, 2, 37, 300, 301)[b % 6] + 2 * (b // 6)
        if b % 7 == 3:
            length = T
        room = length - T
        start = (0, room, room // 2, max(room - 1, 0), min(1, room), min(3, room), room // 3)[b % 7]
        lengths.append(length), starts.append(start)
    return lengths, starts


@pytest.mark.parametrize("T,B,C_", [(1378, 28, 1024), (1378, 1, 32), (512, 28, 32), (512, 1, 1024), (37, 28, 32), (37, 1, 1024),
                                    (37, 5, 32)])
def test_gather_bit_identical_to_composed_path(T, B, C_):
    stats = make_stats(C_)
    variants = [batch_layout(B, T)] if B > 1 else [([T + d], [s]) for d, s in ((0, 0), (1, 1), (8, 3), (9, 9), (301, 150), (300, 300 - 1))]
    for lengths, starts in variants:
        assert all(0 <= s <= n - T for s, n in zip(starts, lengths))
        hr_src = [make_src(C_, n, 100 + i).cuda() for i, n in enumerate(lengths)]
        lr_src = [make_src(C_, n, 500 + i).cuda() for i, n in enumerate(lengths)]
        flat, hr, lr, guards = guarded_pair(B, C_, T)
        gather(hr_src, lr_src, starts, T, stats, (hr, lr))
        assert torch.equal(bits(hr), bits(composed(hr_src, starts, T, stats["hr_mean"], stats["hr_std"])))
        assert torch.equal(bits(lr), bits(composed(lr_src, starts, T, stats["lr_mean"], stats["lr_std"])))
        assert all(bool((g == CANARY).all()) for g in guards), "wrote outside the output tensors"
        first = flat.clone()
        gather(hr_src, lr_src, starts, T, stats, (hr, lr))
        assert torch.equal(bits(flat), bits(first))                                  # two calls, identical bits
        gather(hr_src, lr_src, starts, T, None, (hr, lr))                            # null statistics: the plain conversion
        assert torch.equal(bits(hr), bits(composed(hr_src, starts, T, None, None)))
        assert torch.equal(bits(lr), bits(composed(lr_src, starts, T, None, None)))
        assert all(bool((g == CANARY).all()) for g in guards)


def test_gather_source_alignment_inside_a_larger_buffer():
    """sources that start on every 2-byte offset of a 16-byte line (views into one allocation)"""
    T, C_ = 37, 32
    stats = make_stats(C_)
    big = make_src(1, C_ * 64 * 9 + 64, 3).cuda().view(-1)
    hr_src = [big[off:off + C_ * (T + off)].view(C_, T + off) for off in range(9)]
    starts = [off % 3 for off in range(9)]
    hr, lr = gather(hr_src, hr_src, starts, T, stats)
    assert torch.equal(bits(hr), bits(composed(hr_src, starts, T, stats["hr_mean"], stats["hr_std"])))
    assert torch.equal(bits(lr), bits(composed(hr_src, starts, T, stats["lr_mean"], stats["lr_std"])))


@pytest.mark.parametrize("T", [1378, 512, 37])
def test_short_clips_follow_the_golden_index_map(T, golden_dir):
    z = np.load(os.path.join(golden_dir, "fit_crops.npz"))
    lengths = [int(n) for n, f in z["short_cases"].tolist() if f == T]
    assert {1, 5, T - 1} <= set(lengths) and (T == 37 or 500 in lengths)
    C_ = 32
    stats = make_stats(C_)
    lengths = lengths + [T + 5]                                   # a long clip in the same batch
    hr_src = [make_src(C_, n, 40 + n).cuda() for n in lengths]
    lr_src = [make_src(C_, n, 90 + n).cuda() for n in lengths]
    starts = [0] * (len(lengths) - 1) + [5]
    flat, hr, lr, guards = guarded_pair(len(lengths), C_, T)
    gather(hr_src, lr_src, starts, T, stats, (hr, lr))
    for b, n in enumerate(lengths[:-1]):
        idx = torch.from_numpy(z[f"short_map_{T}_{n}"].astype(np.int64)).cuda()
        for got, src, m, s in ((hr, hr_src, "hr_mean", "hr_std"), (lr, lr_src, "lr_mean", "lr_std")):
            want = channel_affine(src[b][:, idx].float().unsqueeze(0), stats[m], stats[s])
            assert torch.equal(bits(got[b:b + 1]), bits(want)), (T, n)
    assert torch.equal(bits(hr[-1:]), bits(composed(hr_src[-1:], [5], T, stats["hr_mean"], stats["hr_std"])))
    assert all(bool((g == CANARY).all()) for g in guards)


def test_gather_rejects_bad_arguments():
    x = make_src(32, 50, 1).cuda()
    out = torch.empty(1, 32, 40, device="cuda")
    with pytest.raises(ValueError, match="all given or all null"):
        gather([x], [x], [0], 40, {"hr_mean": torch.zeros(32).cuda(), "hr_std": None, "lr_mean": None, "lr_std": None}, (out, out.clone()))
    with pytest.raises(ValueError, match="above"):
        gather([x], [x], [0], 9000, None, (out, out.clone()))


@pytest.fixture(scope="module")
def data_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("latents")
    os.makedirs(d / "train")
    for i, n in enumerate([300, 257, 40, 512, 301, 256, 399]):          # one shorter than frames = 256 ... and one equal
        jio.save_latent_file(str(d / "train" / f"clip_{i:02d}.pt"), hr_latent=make_src(32, n, 10 + i), lr_latent=make_src(32, n, 20 + i),
                             metadata={"name": f"clip_{i:02d}"})
    return str(d)


def test_store_host_resident_files_give_the_same_bits(data_dir):
    T, C_ = 256, 32
    stats = make_stats(C_)
    full = LatentStore(data_dir, "train", T, "cuda")
    tiny = LatentStore(data_dir, "train", T, "cuda", max_resident_bytes=2 * 2 * 32 * 300)   # room for the first file only
    assert len(full) == len(tiny) == 7 and full.lengths == [300, 257, 40, 512, 301, 256, 399]
    assert all(full.is_resident(i) for i in range(7)) and full.stage_guards() is None
    assert [tiny.is_resident(i) for i in range(7)] == [True, False, True, False, False, False, False]   # the short clip stays on the device
    plans = [([0, 1, 2, 3], [44, 1, 0, 255]), ([4, 5, 6, 1], [45, 0, 143, 0]), ([3, 3, 2, 6], [0, 256, 0, 1]), ([0, 2, 0, 2], [0, 0, 43, 0]),
             ([6, 5, 4, 3], [142, 0, 44, 101])]
    want = [tuple(t.clone() for t in full.batch(f, s, stats)) for f, s in plans]
    for b, (f, s) in enumerate(plans):                       # against the composed path on the files themselves
        srcs = [torch.load(full.files[i], weights_only=False) for i in f]
        idx = [(torch.arange(T) + a) % full.lengths[i] for i, a in zip(f, s)]
        hr = torch.stack([d["hr_latent"][:, j] for d, j in zip(srcs, idx)]).cuda().float()
        assert torch.equal(bits(want[b][0]), bits(channel_affine(hr, stats["hr_mean"], stats["hr_std"])))
    for use_prefetch in (False, True):
        for b, (f, s) in enumerate(plans):
            if use_prefetch and b == 0:
                tiny.prefetch(f, s)
            hr, lr = tiny.batch(f, s, stats)
            if use_prefetch and b + 1 < len(plans):
                tiny.prefetch(*plans[b + 1])                # one batch ahead, while this one is still being read
            assert torch.equal(bits(hr), bits(want[b][0])) and torch.equal(bits(lr), bits(want[b][1])), (use_prefetch, b)
    torch.cuda.synchronize()
    before, after = tiny.stage_guards()
    assert bool((before == 0x7C01).all()) and bool((after == 0x7C01).all()), "wrote outside the staging buffer"
    raw_hr, raw_lr = tiny.batch(*plans[0])                   # no statistics: the fp16 values as they are
    assert torch.equal(bits(raw_hr), bits(full.batch(*plans[0])[0]))
    with pytest.raises(ValueError, match="crop start"):
        full.batch([0], [45], stats)
    with pytest.raises(ValueError, match="No .pt files"):
        LatentStore(data_dir, "val", T, "cuda")


def both_builds_outputs():
    """what the child on libjat_hip_fp16.so and this process both compute: one gathered batch of the ragged layout (every
    alignment case of `batch_layout`, the special values of `make_src`) and one monitor call"""
    T, B, C_ = 37, 7, 32
    lengths, starts = batch_layout(B, T)
    hr_src = [make_src(C_, n, 100 + i).cuda() for i, n in enumerate(lengths)]
    lr_src = [make_src(C_, n, 500 + i).cuda() for i, n in enumerate(lengths)]
    hr, lr = gather(hr_src, lr_src, starts, T, make_stats(C_))
    g = torch.Generator().manual_seed(11)
    target = torch.randn((3, 5, 1031), generator=g) * 1.1 + 0.05
    pred = target + torch.randn((3, 5, 1031), generator=g) * 0.3 - 0.02
    cond = torch.randn((3, 5, 1031), generator=g) * 1.3 + 0.1
    sums = train_monitor(pred.cuda(), target.cuda(), cond.cuda())
    return {k: v.cpu().numpy() for k, v in dict(hr=hr, lr=lr, sums=sums).items()}


def test_fp16_library_gives_the_same_bits(tmp_path):
    """data.hip is fp32 in both builds (csrc/Makefile): libjat_hip_fp16.so, in a child process, computes the bits this process
    computes"""
    code = ("import sys, numpy as np\n"
            "sys.path.insert(0, 'tests')\n"
            "import jatsr_amd._lib as L\n"
            "from test_gpu_data import both_builds_outputs\n"
            "assert L.operand_dtype() == 'fp16'\n"
            "np.savez(sys.argv[1], **both_builds_outputs())\n")
    env = dict(os.environ, JAT_OPERAND_DTYPE="fp16")
    env.pop("JAT_LIB_PATH", None)
    path = str(tmp_path / "fp16.npz")
    out = subprocess.run([sys.executable, "-c", code, path], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
    got, mine = dict(np.load(path)), both_builds_outputs()
    assert sorted(got) == sorted(mine) == ["hr", "lr", "sums"]
    for k, v in mine.items():
        assert v.dtype == got[k].dtype and np.isfinite(v).all() and np.abs(v).max() > 0, k
        assert np.array_equal(v, got[k]) and v.tobytes() == got[k].tobytes(), k
    assert mine["hr"].shape == (7, 32, 37) and mine["sums"].shape == (6,) and mine["sums"].dtype == np.float64


def np_sums(p, h, l):
    p, h = p.double().cpu().numpy().ravel(), h.double().cpu().numpy().ravel()
    terms = [p, p * p, h * h, (p - h) ** 2]
    if l is not None:
        l = l.double().cpu().numpy().ravel()
        terms += [l, l * l]
    return [float(t.sum()) for t in terms], [float(np.abs(t).sum()) for t in terms]


@pytest.mark.parametrize("shape,cond_scale", [((28, 1024, 1378), 1.3), ((3, 5, 7), 3.0), ((1, 2, 2), 0.1)])
def test_train_monitor(shape, cond_scale):
    g = torch.Generator(device="cuda").manual_seed(11)
    target = torch.randn(shape, device="cuda", generator=g) * 1.1 + 0.05
    pred = target + torch.randn(shape, device="cuda", generator=g) * 0.3 - 0.02
    cond = torch.randn(shape, device="cuda", generator=g) * cond_scale + 0.1
    n = pred.numel()
    got = train_monitor(pred, target, cond)
    assert got.dtype == torch.float64 and torch.equal(got.view(torch.int64), train_monitor(pred, target, cond).view(torch.int64))
    ref, mag = np_sums(pred, target, cond)
    # worst-case error of an fp64 sum of n = 3.95e7 terms: n 2^-53 = 4.4e-9 of sum |terms|; twice that
    for q, (a, b, m) in enumerate(zip(got.tolist(), ref, mag)):
        print(f"sum {q}: {a!r} vs {b!r}, |diff| / sum|terms| = {abs(a - b) / m:.3e}")
        assert abs(a - b) <= 1e-8 * m, q
    no_cond = train_monitor(pred, target).tolist()
    assert no_cond[:4] == got.tolist()[:4] and no_cond[4:] == [0.0, 0.0]
    # the derived figures against the reference's formulas (train_ddp_v3mod2.py:902-919) in fp64
    p, h, l = (x.double().cpu().numpy().ravel() for x in (pred, target, cond))
    want = dict(pred_mean=p.mean(), pred_std=p.std(ddof=1),
                snr_db=10 * math.log10((h ** 2).mean() / (((p - h) ** 2).mean() + 1e-8)),
                cond_noise_std=0.05 * min(max(l.std(ddof=1), 0.5), 2.0))
    fig = monitor_figures(got.tolist(), n, 0.05, True)
    for k, v in want.items():
        print(f"{k}: {fig[k]!r} vs {v!r}")
        assert abs(fig[k] - v) <= 1e-9 * abs(v), k
    assert monitor_figures(got.tolist(), n, 0.05, False)["cond_noise_std"] == 0.05
    if cond_scale == 3.0:
        assert fig["cond_noise_std"] == 0.05 * 2.0
    if cond_scale == 0.1:
        assert fig["cond_noise_std"] == 0.05 * 0.5
