"""Host side of gradient accumulation (Trainer(grad_accum_steps=k), fit --grad-accum-steps K), no GPU: the
parser, the argument check that comes before the GPU is required, the mask seeds of the micro-batches, the steps-per-epoch
arithmetic and the declarations of the C ABI."""
import os
import re

import pytest

import jatsr_amd._lib as L
from jatsr_amd import fit as F
from jatsr_amd.train import Trainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = 2 ** 64 - 1


def test_parser_default_and_rejection(capsys):
    assert F.build_parser().parse_args([]).grad_accum_steps == 1
    assert F.build_parser().parse_args(["--grad-accum-steps", "4"]).grad_accum_steps == 4
    for bad in ("0", "-2", "1.5", "two"):
        with pytest.raises(SystemExit):
            F.build_parser().parse_args(["--grad-accum-steps", bad])
    assert "--grad-accum-steps" in capsys.readouterr().err


@pytest.mark.parametrize("bad", [0, -1, 1.5])
def test_trainer_rejects_the_count_before_the_gpu_is_required(bad, monkeypatch):
    """The check sits with the other argument checks at the top of __init__: neither the GPU nor the model is looked at."""
    def no_gpu():
        raise AssertionError("require_gpu was reached")
    monkeypatch.setattr(L, "require_gpu", no_gpu)
    with pytest.raises(ValueError, match="grad_accum_steps"):
        Trainer(None, batch_size=2, frames=24, grad_accum_steps=bad)


def seed_formula(mask_seed, step, rank):
    """The step seed as it was before micro-batches existed: splitmix64 of mask_seed + golden * (step * 4096 + rank + 1)."""
    x = (mask_seed + 0x9E3779B97F4A7C15 * (step * 4096 + rank + 1)) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def bare_trainer(mask_seed, global_step=0):
    tr = Trainer.__new__(Trainer)
    tr.mask_seed, tr.global_step, tr.distributed, tr.group = mask_seed, global_step, False, None
    return tr


def test_step_seed_of_micro_batch_zero_is_the_old_seed():
    for mask_seed in (0x9E3779B97F4A7C15, 7, 2 ** 63 + 12345):
        tr = bare_trainer(mask_seed, global_step=11)
        assert tr.step_seed() == tr.step_seed(micro=0) == seed_formula(mask_seed, 11, 0)
        for step in (0, 1, 5, 123456, 2 ** 31):
            assert tr.step_seed(step) == tr.step_seed(step, 0) == seed_formula(mask_seed, step, 0)
            for rank in (0, 1, 63):
                assert tr._step_seed(step, 0, rank) == seed_formula(mask_seed, step, rank)
        assert tr.step_seed(3, 1) != tr.step_seed(3, 0)


def test_step_seeds_do_not_collide_over_steps_micro_batches_and_ranks():
    tr = bare_trainer(0x9E3779B97F4A7C15)
    seeds = {tr._step_seed(step, micro, rank) for step in range(8) for micro in range(64) for rank in range(64)}
    assert len(seeds) == 8 * 64 * 64
    # neighbouring steps do not run into each other at the edges of their counter ranges
    assert tr._step_seed(0, 63, 63) != tr._step_seed(1, 0, 0)


@pytest.mark.parametrize("n,k,steps,left", [(4, 1, 4, 0), (4, 2, 2, 0), (5, 2, 2, 1), (5, 4, 1, 1), (3, 4, 0, 3), (0, 1, 0, 0),
                                            (345, 4, 86, 1)])
def test_steps_per_epoch(n, k, steps, left):
    assert F.steps_per_epoch(n, k) == (steps, left)


def test_steps_per_epoch_rejects_a_count_below_one():
    for bad in (0, -3):
        with pytest.raises(ValueError, match="grad_accum_steps"):
            F.steps_per_epoch(10, bad)


def test_header_declares_the_accumulation_entry_points():
    header = open(os.path.join(ROOT, "include", "jat_hip.h")).read()
    assert re.search(r"#define\s+JAT_FB_ACCUMULATE\s+1\b", header) and re.search(r"#define\s+JAT_FB_NO_HOOK\s+2\b", header)
    assert (L.FB_ACCUMULATE, L.FB_NO_HOOK) == (1, 2)
    fb = re.search(r"int\s+jat_trainer_fwd_bwd_ex\s*\(([^;]*)\)\s*;", header)
    plain = re.search(r"int\s+jat_trainer_fwd_bwd\s*\(([^;]*)\)\s*;", header)
    norm = lambda s: re.sub(r"\s+", " ", s).strip()
    # the plain call's arguments, then the flags in front of the stream
    assert norm(fb.group(1)) == norm(plain.group(1)).replace(", void* stream", ", int32_t flags, void* stream")
    wg = re.search(r"int\s+jat_k_weight_grad_ex\s*\(([^;]*)\)\s*;", header)
    wg0 = re.search(r"int\s+jat_k_weight_grad\s*\(([^;]*)\)\s*;", header)
    assert norm(wg.group(1)) == norm(wg0.group(1)).replace(", void* stream", ", int32_t accumulate, void* stream")
    for name, plain_name in (("jat_trainer_fwd_bwd_ex", "jat_trainer_fwd_bwd"), ("jat_k_weight_grad_ex", "jat_k_weight_grad")):
        res, args = L.SIGNATURES[name]
        res0, args0 = L.SIGNATURES[plain_name]
        assert res is res0 and list(args) == list(args0[:-1]) + [L._I32, args0[-1]]
