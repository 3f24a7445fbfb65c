"""Caller-owned workspaces: exactly the reported size, stale, between guard bands.

For every entry below the workspace is `need` bytes, `need` being what the entry's `*_workspace_bytes` function or its documented
formula gives, cut out of a larger allocation with GUARD bytes of the pattern 0xA5 on either side (the guard keeps the 256-byte
alignment of the allocation).  The entry runs on input A, which leaves legal stale state of the same shape behind, then on a
different input B in the same workspace; B's outputs must have the bits of B run in a fresh zero-filled workspace, and the guards
around the workspace and around every output must be intact after both runs.  With `need - 1` and `need - 16` bytes the entry
must refuse with its documented error and write nothing: outputs, workspace and guards stay as they were.

The only contents a workspace ever holds here are zeros and what a real run of the same entry left: the model's workspace may
hold counters a kernel waits on, so no test writes arbitrary bytes into one.

Left out because their own tests already pass an exact-size workspace between guards: the loss kernels (tests/test_gpu_loss_paths.py,
tests/test_gpu_mod3_loss.py), the training-step kernels (tests/test_gpu_train_kernels.py) and the two entries of the probabilistic
pitch tracker (their own GPU test file); `jat_yin` takes no workspace."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import jatsr_amd._lib as L  # noqa: E402
import jatsr_amd.recipe as recipe  # noqa: E402
from stream_check import bits_equal  # noqa: E402
from test_gpu_streams import _audio, cuda, gen, micro, vp  # noqa: E402

GUARD, PATTERN, SENTINEL = 4096, 0xA5, 0x5A


class Guarded:
    """`nbytes` bytes (filled with `fill`) between two bands of GUARD pattern bytes"""

    def __init__(self, nbytes, fill=0):
        self.n = int(nbytes)
        self.buf = torch.full((2 * GUARD + self.n,), PATTERN, dtype=torch.uint8, device="cuda")
        self.mid = self.buf[GUARD:GUARD + self.n]
        self.mid.fill_(fill)

    @property
    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + GUARD)

    def intact(self):
        return bool((self.buf[:GUARD] == PATTERN).all()) and bool((self.buf[GUARD + self.n:] == PATTERN).all())

    def view(self, shape, dtype):
        t = self.mid.view(torch.float32).view(torch.complex64) if dtype == torch.complex64 else self.mid.view(dtype)
        return t.view(shape)


def out_buffers(spec, fill=SENTINEL):
    """spec {name: (shape, dtype)} -> {name: (Guarded, view)}"""
    outs = {}
    for k, (shape, dtype) in spec.items():
        esize = 8 if dtype == torch.complex64 else torch.empty(0, dtype=dtype).element_size()
        g = Guarded(int(np.prod(shape)) * esize, fill)
        outs[k] = (g, g.view(shape, dtype))
    return outs


def exercise(name, need, run, spec, A, B, error, out_fill=SENTINEL):
    """run(inputs, workspace pointer, workspace bytes, {name: output view}) -> return code"""
    need = int(need)
    assert need > 16, (name, need)

    def go(inputs, ws, nbytes):
        outs = out_buffers(spec, out_fill)
        rc = run(inputs, ws.ptr, nbytes, {k: v for k, (_, v) in outs.items()})
        torch.cuda.synchronize()
        return rc, outs

    def intact(ws, outs):
        return ws.intact() and all(g.intact() for g, _ in outs.values())

    fresh = Guarded(need)
    rc, want = go(B, fresh, need)
    assert rc == 0 and intact(fresh, want), (name, rc, L.lib().jat_last_error())
    ws = Guarded(need)
    rc, first = go(A, ws, need)
    assert rc == 0 and intact(ws, first), (name, "run A", rc)
    rc, second = go(B, ws, need)
    assert rc == 0 and intact(ws, second), (name, "run B in the stale workspace", rc)
    assert any(not bits_equal(first[k][1], second[k][1]) for k in spec), (name, "A and B give the same outputs: the case checks nothing")
    bad = [k for k in spec if not bits_equal(second[k][1], want[k][1])]
    assert not bad, f"{name}: outputs {bad} depend on what the workspace held before the call"
    before = ws.mid.clone()
    for short in (need - 1, need - 16):
        rc, outs = go(B, ws, short)
        assert rc == error, (name, short, rc)
        assert intact(ws, outs) and torch.equal(ws.mid, before), (name, short, "a refused call wrote to the workspace or past it")
        for k, (g, _) in outs.items():
            assert bool((g.mid == out_fill).all()), (name, short, k, "a refused call wrote an output")


# ---- the model forward family ----------------------------------------------------------------------------------------------
def model_need(h, B, T):
    need = C.c_size_t()
    L.check(L.lib().jat_model_workspace_bytes(h.ptr, B, T, C.byref(need)))
    return need.value


def test_forward_model():
    h = micro()._get_handle()
    B, T = 2, 22

    def inputs(salt):
        x_t, x_c = recipe.make_latents(B, 32, T, salt=salt)
        return {"x_t": cuda(x_t), "x_cond": cuda(x_c), "t": cuda(np.array([0.02 + 0.001 * salt, 0.98], np.float32))}

    def run(i, ws, n, o):
        return L.lib().jat_forward(h.ptr, vp(i["x_t"]), vp(i["t"]), vp(i["x_cond"]), vp(o["y"]), B, T, ws, n, L.stream_ptr())
    exercise("jat_forward", model_need(h, B, T), run, {"y": ((B, 32, T), torch.float32)}, inputs(100), inputs(101), L.JAT_E_STATE)


def test_block_forward_model():
    h = micro()._get_handle()
    B, N, D = 2, 10, 256

    def run(i, ws, n, o):
        return L.lib().jat_block_forward(h.ptr, 1, vp(i["x"]), vp(i["t_emb"]), vp(o["y"]), B, N, ws, n, L.stream_ptr())
    A, Bi = ({"x": gen((B, N, D), s), "t_emb": gen((B, D), s + 1)} for s in (1, 3))
    exercise("jat_block_forward", model_need(h, B, 4 * N), run, {"y": ((B, N, D), torch.float32)}, A, Bi, L.JAT_E_STATE)


def test_attn_forward_model():
    h = micro()._get_handle()
    B, N, D = 2, 37, 256

    def run(i, ws, n, o):
        return L.lib().jat_attn_forward(h.ptr, 1, vp(i["x"]), vp(o["y"]), B, N, ws, n, L.stream_ptr())
    exercise("jat_attn_forward", model_need(h, B, 4 * N), run, {"y": ((B, N, D), torch.float32)}, {"x": gen((B, N, D), 5)},
             {"x": gen((B, N, D), 6)}, L.JAT_E_STATE)


def test_time_embed_model():
    h = micro()._get_handle()
    B, D = 5, 256

    def run(i, ws, n, o):
        return L.lib().jat_time_embed(h.ptr, vp(i["t"]), vp(o["y"]), B, ws, n, L.stream_ptr())
    exercise("jat_time_embed", model_need(h, B, 4), run, {"y": ((B, D), torch.float32)},
             {"t": cuda(np.array([0.0, 0.02, 0.5, 0.98, 1.0], np.float32))}, {"t": cuda(np.array([0.1, 0.3, 0.7, 0.9, 0.4], np.float32))},
             L.JAT_E_STATE)


# ---- audio -----------------------------------------------------------------------------------------------------------------
N_FFT, HOP, LEN, ROWS = 512, 128, 1301, 2
BINS, FRAMES = 1 + N_FFT // 2, 1 + LEN // HOP


def metrics_handle(n_mels=0):
    from jatsr_amd.metrics import _handle
    return _handle(44100, N_FFT, HOP, n_mels, torch.device("cuda", torch.cuda.current_device()))


def test_audio_metrics_run():
    h = metrics_handle(40)
    need = C.c_size_t()
    L.check(L.lib().jat_audio_metrics_workspace_bytes(h.ptr, ROWS, LEN, C.byref(need)))

    def run(i, ws, n, o):
        return L.lib().jat_audio_metrics_run(h.ptr, vp(i["pred"]), vp(i["gt"]), ROWS, LEN, 1, vp(o["out"]), vp(o["lsd"]), vp(o["pdb"]),
                                             vp(o["gdb"]), ws, n, L.stream_ptr())
    spec = {"out": ((ROWS, 3), torch.float64), "lsd": ((ROWS, FRAMES), torch.float32), "pdb": ((ROWS, 40, FRAMES), torch.float32),
            "gdb": ((ROWS, 40, FRAMES), torch.float32)}
    A, B = ({"pred": _audio(ROWS, LEN, s), "gt": _audio(ROWS, LEN, s + 1)} for s in (5, 25))
    exercise("jat_audio_metrics_run", need.value, run, spec, A, B, L.JAT_E_STATE)


def test_istft():
    h = metrics_handle()
    need = C.c_size_t()
    L.check(L.lib().jat_istft_workspace_bytes(N_FFT, HOP, ROWS, LEN, C.byref(need)))

    def run(i, ws, n, o):
        return L.lib().jat_istft(h.ptr, vp(i["X"]), ROWS, LEN, vp(o["y"]), ws, n, L.stream_ptr())
    A, B = ({"X": torch.view_as_complex(gen((ROWS, BINS, FRAMES, 2), s))} for s in (9, 29))
    exercise("jat_istft", need.value, run, {"y": ((ROWS, LEN), torch.float32)}, A, B, L.JAT_E_STATE)


def test_ltas():
    h = metrics_handle()

    def run(i, ws, n, o):
        return L.lib().jat_ltas(h.ptr, vp(i["x"]), ROWS, LEN, vp(o["P"]), ws, n, L.stream_ptr())
    exercise("jat_ltas", ROWS * L.LTAS_SLICES * BINS * 8, run, {"P": ((ROWS, BINS), torch.float64)}, {"x": _audio(ROWS, LEN, 10)},
             {"x": _audio(ROWS, LEN, 30) * 0.5}, L.JAT_E_STATE)


def test_band_splice():
    from jatsr_amd.splice import band_gain
    h = metrics_handle()
    gain = band_gain(44100, N_FFT, 8000.0, 2000.0).cuda()
    need = C.c_size_t()
    L.check(L.lib().jat_band_splice_workspace_bytes(N_FFT, HOP, ROWS, LEN, LEN + 7, C.byref(need)))

    def run(i, ws, n, o):
        return L.lib().jat_band_splice(h.ptr, vp(i["g"]), vp(i["s"]), ROWS, LEN, LEN + 7, vp(gain), vp(o["y"]), ws, n, L.stream_ptr())
    A, B = ({"g": _audio(ROWS, LEN, s), "s": _audio(ROWS, LEN + 7, s + 1)} for s in (11, 31))
    exercise("jat_band_splice", need.value, run, {"y": ((ROWS, LEN), torch.float32)}, A, B, L.JAT_E_STATE)


def test_channel_stats():
    Bn, Cc, T = 2, 32, 37

    def run(i, ws, n, o):
        return L.lib().jat_channel_stats(vp(i["z"]), Bn, Cc, T, vp(o["sum"]), vp(o["sq"]), ws, n, L.stream_ptr())
    # the caller owns and zeroes the two running totals: the outputs start as zeros here, not as the sentinel
    exercise("jat_channel_stats", Cc * 16 * 16, run, {"sum": ((Cc,), torch.float64), "sq": ((Cc,), torch.float64)},
             {"z": gen((Bn, Cc, T), 2)}, {"z": gen((Bn, Cc, T), 22)}, L.JAT_E_STATE, out_fill=0)


def test_train_monitor():
    shape = (3, 5, 7)

    def run(i, ws, n, o):
        return L.lib().jat_train_monitor(vp(i["p"]), vp(i["h"]), vp(i["l"]), 105, vp(o["out"]), ws, n, L.stream_ptr())
    A, B = ({"p": gen(shape, s), "h": gen(shape, s + 1), "l": gen(shape, s + 2)} for s in (140, 150))
    exercise("jat_train_monitor", L.MONITOR_WORK_BYTES, run, {"out": ((6,), torch.float64)}, A, B, L.JAT_E_STATE)


# ---- bank searches ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bank():
    """5000 rows: two slabs of JAT_BANK_SLAB key rows, the second ragged"""
    from jatsr_amd.retrieval import LatentBank
    b = LatentBank(32, 5000, key="hr")
    b.load_rows(gen((5000, 32), 160, dtype=torch.float16))
    torch.cuda.synchronize()
    assert len(b) == 5000 > L.BANK_SLAB
    return b


QB, QT = 2, 37


def test_bank_search(bank):
    need = C.c_size_t()
    L.check(L.lib().jat_bank_search_workspace_bytes(bank._h, QB * QT, C.byref(need)))
    mean, std = gen((32,), 161, 0.1), gen((32,), 162).abs() + 0.5

    def run(i, ws, n, o):
        return L.lib().jat_bank_search(bank._h, vp(i["x"]), vp(mean), vp(std), QB, QT, vp(o["idx"]), vp(o["d2"]), ws, n, L.stream_ptr())
    exercise("jat_bank_search", need.value, run, {"idx": ((QB, QT), torch.int32), "d2": ((QB, QT), torch.float32)},
             {"x": gen((QB, 32, QT), 163)}, {"x": gen((QB, 32, QT), 164)}, L.JAT_E_INVALID)


def test_bank_search_topk(bank):
    k = 3
    need = C.c_size_t()
    L.check(L.lib().jat_bank_topk_workspace_bytes(bank._h, QB * QT, k, C.byref(need)))

    def run(i, ws, n, o):
        return L.lib().jat_bank_search_topk(bank._h, vp(i["x"]), None, None, QB, QT, k, vp(o["idx"]), vp(o["d2"]), ws, n,
                                            L.stream_ptr())
    exercise("jat_bank_search_topk", need.value, run, {"idx": ((QB, QT, k), torch.int32), "d2": ((QB, QT, k), torch.float32)},
             {"x": gen((QB, 32, QT), 165)}, {"x": gen((QB, 32, QT), 166)}, L.JAT_E_INVALID)
