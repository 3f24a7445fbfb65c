"""`python bench.py --gpus N` must start its own ranks: the parent spawns a torch.distributed.run
child before touching any GPU and relays rank 0's JSON line.  Rehearsed on CPU with --dry-run (gloo, world_size 2): the
launcher, the rendezvous on 127.0.0.1, the barrier / max-over-ranks timing contract and both scaling modes."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dry-run", "--steps", "3", "--warmup", "1"] + extra,
                         capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout           # ONE JSON line, from rank 0
    return json.loads(lines[0])


@pytest.mark.parametrize("scaling", ["weak", "strong"])
def test_bench_starts_its_own_ranks_world2(scaling):
    r = _run(["--gpus", "2", "--scaling", scaling])
    assert r["n_gpus"] == 2 and r["ranks_seen"] == 2 and r["dry_run"] is True
    assert r["steps"] == 3 and r["warmup"] == 1 and r["scaling"] == scaling and r["value"] > 0
    assert r["config"]["B_local"] == (14 if scaling == "strong" else 28)      # 28 -> 14,14 (jatsr_amd.dist.shard_range)


def test_bench_dry_run_single_rank():
    r = _run(["--gpus", "1"])
    assert r["n_gpus"] == 1 and r["ranks_seen"] == 1


def test_bench_full_option_keeps_the_contract():
    """--full (the extra legs after the headline, GPU path only) is accepted and leaves the one-line timing contract as it is."""
    r = _run(["--gpus", "2", "--full"])
    assert r["n_gpus"] == 2 and r["ranks_seen"] == 2 and r["steps"] == 3 and r["warmup"] == 1 and r["value"] > 0


@pytest.mark.parametrize("mode", ["train", "long"])
def test_bench_launcher_other_modes_world2(mode):
    """`--mode train` (configs[3]: the gradient exchange of jatsr_amd.dist.exchange_sum_, slice by slice, summed right on both
    ranks) and `--mode long` (configs[4]: the chunk plan sharded round-robin, one object gather per file) through the same
    self-launch + 127.0.0.1 rendezvous + barrier / max-over-ranks contract, world_size 2 on gloo."""
    r = _run(["--gpus", "2", "--mode", mode])
    assert r["n_gpus"] == 2 and r["ranks_seen"] == 2 and r["dry_run"] is True and r["config"]["mode"] == mode
    assert r["steps"] == 3 and r["value"] > 0 and ("training" in r["metric"] if mode == "train" else "long-sequence" in r["metric"])


def test_bench_dump_outputs_dry_run(tmp_path):
    """--dump-outputs DIR: rank 0 writes what the last timed step returned as DIR/<name>.npy, the same on every run with the
    same arguments (the GPU modes write the sampler / trainer outputs through the same function)."""
    import numpy as np
    got = []
    for d in ("a", "b"):
        r = _run(["--gpus", "2", "--dump-outputs", str(tmp_path / d)])
        assert r["steps"] == 3 and r["ms_per_step"] > 0
        assert sorted(os.listdir(tmp_path / d)) == ["out.npy"]
        got.append(np.load(tmp_path / d / "out.npy"))
    assert got[0].dtype == np.float64 and np.array_equal(got[0], got[1])


def test_dump_outputs_cap_and_seeded_sample(tmp_path):
    """Above 64 MB in all, large arrays are cut to a fixed, seeded sample of their elements (sorted positions, written 1-D);
    small arrays and the dtypes (float64 kept, everything else float32) are left as they are."""
    import numpy as np
    import bench
    big = np.arange(10_000_000, dtype=np.float64)                  # 80 MB: its values are its positions
    small = np.arange(6, dtype=np.int32).reshape(2, 3)
    out = {}
    for d in ("a", "b"):
        w = bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small, "loss": np.float64(0.25)})
        assert w["small"] == (6, 6) and w["loss"] == (1, 1) and 0 < w["big"][0] < w["big"][1]
        assert sum(os.path.getsize(tmp_path / d / f) for f in os.listdir(tmp_path / d)) <= bench.DUMP_LIMIT_BYTES
        out[d] = {k: np.load(tmp_path / d / (k + ".npy")) for k in ("big", "small", "loss")}
    a, b = out["a"], out["b"]
    assert np.array_equal(a["big"], b["big"]) and a["big"].dtype == np.float64 and a["big"].ndim == 1
    assert np.all(np.diff(a["big"]) >= 0) and a["big"].min() >= 0 and a["big"].max() < big.size
    assert a["small"].dtype == np.float32 and np.array_equal(a["small"], small) and a["loss"] == 0.25
