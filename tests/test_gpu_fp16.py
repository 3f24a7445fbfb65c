"""The fp16-operand build (libjat_hip_fp16.so, csrc/jat_dtype.h): `torch.amp.autocast('cuda')` of the v3mod2 trainer is
fp16 with a dynamic loss scale (train_ddp_v3mod2.py:745,854).  The operand dtype is a process-level choice
(JAT_OPERAND_DTYPE=fp16), so this module re-runs the per-kernel, model, sampler and training parity tests in child processes
against that library: the same reference goldens and the same gates (fp16 rounds operands with 3 more mantissa bits than
bf16), plus the fp16-specific behaviour — operand overflow (> 65504) must surface as a skipped step and a halved scale.
What runs is the table of tests/fp16_matrix.py: one child per selection, one after another."""
import os
import re
import subprocess
import sys
import time

import pytest

from fp16_matrix import children

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _child(args, extra_env=None, timeout=900):
    env = dict(os.environ, JAT_OPERAND_DTYPE="fp16", **(extra_env or {}))
    env.pop("JAT_LIB_PATH", None)
    out = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider"] + args, cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=timeout)
    tail = (out.stdout + out.stderr)[-3000:]
    assert out.returncode == 0, tail
    passed = re.search(r"\b(\d+) passed\b", tail)            # a -k expression that matches nothing must not pass silently
    assert passed and int(passed.group(1)) >= 1, tail
    return tail


def test_fp16_library_is_what_the_env_selects():
    code = "import jatsr_amd._lib as L; print(L.operand_dtype(), L.LIB_PATH)"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, JAT_OPERAND_DTYPE="fp16"),
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-1000:]
    assert out.stdout.split()[0] == "fp16" and out.stdout.split()[1].endswith("libjat_hip_fp16.so")


@pytest.mark.parametrize("args", [a for _, a in children()], ids=[i for i, _ in children()])
def test_fp16_child(args):
    t0 = time.perf_counter()
    tail = _child(args)
    print(f"fp16 child {' '.join(args)}: {tail.strip().splitlines()[-1].strip()} (wall {time.perf_counter() - t0:.1f} s)")
