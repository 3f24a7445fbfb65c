"""What `jat_trainer_create` accepts as a parameter table, without a GPU.  `jat_model_create` describes the model's
parameters (csrc/jat_params.cpp) and `jat_trainer_create` checks the caller's table against that description before its first
HIP call, so a host array as the flat buffers and a null stream are enough: a rejected table returns its code and text, and a
valid one gets as far as creating the weight-gradient stream (JAT_E_HIP here, not asserted)."""
import ctypes as C
import os

import numpy as np
import pytest

import jatsr_amd._lib as L
import jatsr_amd.recipe as recipe
from jatsr_amd.model import JaT_AudioSR_V2, JaT_AudioSR_V3, _Handle
from jatsr_amd.train import flat_layout

MODELS = {"rms": (JaT_AudioSR_V3, 35, 2465536), "ln": (JaT_AudioSR_V2, 30, 2464256)}   # class, tensors, floats of the micro config


@pytest.fixture(scope="module", autouse=True)
def built_lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.lib()


@pytest.fixture(scope="module", params=["rms", "ln"])
def table(request):
    """(norm, model handle, [(name, offset, numel)], flat buffer) of the micro model."""
    cls, n_tensors, n_floats = MODELS[request.param]
    model = cls(**recipe.CONFIGS["micro"])
    layout, total = flat_layout([(k, p.shape) for k, p in model.named_parameters()])
    assert (len(layout), total) == (n_tensors, n_floats)
    return request.param, _Handle(*model._handle_cfg()), [(k, off, n) for k, off, n, _ in layout], np.zeros(total, np.float32)


def create(table, entries, B=2, T=24):
    """jat_trainer_create over `entries` [(name, offset, numel)] -> (code, error text)."""
    _, h, _, flat = table
    refs = (L.JatTensorRef * len(entries))()
    for i, (k, off, n) in enumerate(entries):
        refs[i] = L.JatTensorRef(k.encode(), flat.ctypes.data + 4 * off, n)
    base, tr = C.c_void_p(flat.ctypes.data), C.c_void_p()
    rc = L.lib().jat_trainer_create(h.ptr, refs, len(entries), base, base, base, base, flat.size, B, T, None, C.byref(tr))
    assert (rc == 0) == bool(tr)
    if tr:
        L.lib().jat_trainer_destroy(tr)
    return rc, L.lib().jat_last_error().decode()


def swap_offsets(entries, a, b):
    """The entries with the offsets of those named a[i] and b[i] exchanged."""
    off = {k: o for k, o, _ in entries}
    to = dict(zip(a, b), **dict(zip(b, a)))
    return [(k, off[to.get(k, k)], n) for k, _, n in entries]


@pytest.mark.parametrize("drop", ["last", "blocks.1.mlp.0.bias"])
def test_a_missing_tensor_is_named(table, drop):
    entries = table[2]
    name = entries[-1][0] if drop == "last" else drop
    rc, msg = create(table, [e for e in entries if e[0] != name])
    assert rc == L.JAT_E_STATE and f"missing parameter '{name}'" in msg


def test_a_tensor_the_model_does_not_have_is_counted(table):
    entries = table[2]
    n = len(entries)
    for extra in (("blocks.0.attn.rope.inv_freq", 0, 32), entries[3]):      # an unknown name; one entry twice
        rc, msg = create(table, entries + [extra])
        assert rc == L.JAT_E_INVALID and f"{n + 1} parameters given, {n} belong to this model" in msg


def test_a_slice_outside_the_flat_buffer_or_off_alignment_is_rejected(table):
    _, _, entries, flat = table
    k, off, n = entries[5]
    for bad in ((k, off + 1, n), (k, flat.size, n)):
        rc, msg = create(table, entries[:5] + [bad] + entries[6:])
        assert rc == L.JAT_E_INVALID and f"parameter '{k}' is not a 16-byte aligned slice of the flat buffer" in msg


def test_blocks_out_of_order_are_rejected(table):
    entries = table[2]
    b0 = [k for k, _, _ in entries if k.startswith("blocks.0.")]
    rc, msg = create(table, swap_offsets(entries, b0, [k.replace("blocks.0.", "blocks.1.") for k in b0]))
    assert rc == L.JAT_E_INVALID and "parameters of block 0 are not laid out before those of block 1" in msg


def test_the_head_must_precede_the_blocks(table):
    """t_embedder.3.bias exchanged with a tensor of block 0 of its size (hidden_size floats)."""
    other = "blocks.0.norm1.weight" if table[0] == "rms" else "blocks.0.mlp.3.bias"
    rc, msg = create(table, swap_offsets(table[2], ["t_embedder.3.bias"], [other]))
    assert rc == L.JAT_E_INVALID and "must precede the blocks in the flat buffer" in msg


def test_batch_and_length_limits(table):
    rc, msg = create(table, table[2], B=33)
    assert rc == L.JAT_E_INVALID and "per-rank batch 33 > 32" in msg
    rc, msg = create(table, table[2], T=4 * 2048 + 1)
    assert rc == L.JAT_E_SEQLEN and "Sequence length 2049 exceeds max_len 2048" in msg


def test_a_tensor_of_the_wrong_size_is_rejected(table):
    """Half of blocks.0.mlp.3.weight is still an aligned slice of the flat buffer; the re-pack would cast the full count from it."""
    entries = table[2]
    name = "blocks.0.mlp.3.weight"
    full = {k: n for k, _, n in entries}[name]
    rc, msg = create(table, [(k, off, n // 2 if k == name else n) for k, off, n in entries])
    assert rc == L.JAT_E_INVALID and f"parameter '{name}' has {full // 2} elements, expected {full}" in msg
