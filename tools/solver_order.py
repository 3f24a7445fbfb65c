"""Discretisation error of the sampler's solvers on the fp64 oracle (CPU only).

    python tools/solver_order.py [--configs micro tiny] [--fine 128]

For each configuration (recipe weights, B = 2, T = 64, CFG 3) the sampling ODE is solved with Euler, midpoint and Heun on
linspace grids by the fp64 twin of the solvers (tests/solver_ref.py over oracle.jat_oracle.OracleModel), and each result is
compared (rel-L2) with a fine Euler solve of the same ODE, which carries a discretisation error of its own (about 1e-2 at 128
steps: compare it with the 256-step solve via --fine 256).  Prints the markdown table of DESIGN.md 15.

The weights are synthetic: the table says how the error of the integration rule falls with the number of model evaluations on this
ODE, nothing about trained weights or audio quality.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import jatsr_amd.recipe as recipe  # noqa: E402
from oracle import jat_oracle as O  # noqa: E402

import solver_ref as R  # noqa: E402

RUNS = [("euler", 8), ("euler", 16), ("midpoint", 8), ("midpoint", 16), ("heun", 8)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", nargs="+", default=["micro", "tiny"], choices=sorted(recipe.CONFIGS))
    ap.add_argument("--fine", type=int, default=128, help="Euler steps of the reference solve")
    ap.add_argument("--B", type=int, default=2)
    ap.add_argument("--T", type=int, default=64)
    ap.add_argument("--cfg-scale", type=float, default=3.0)
    args = ap.parse_args()
    heads = [f"{s} {n} ({len(R.plan(O.linspace_f32(0.0, 1.0, n + 1), s)[0])} evals)" for s, n in RUNS]
    print("| config | " + " | ".join(heads) + " |")
    print("|---|" + "---|" * len(RUNS))
    for name in args.configs:
        cfg = recipe.CONFIGS[name]
        model = O.OracleModel(cfg, recipe.make_state_dict(cfg), "rms", np.float64)
        lr = recipe.gaussian("lr_latent", (args.B, cfg["input_channels"], args.T), 900)
        z0 = recipe.gaussian("z0", (args.B, cfg["input_channels"], args.T), 901)
        fine = R.flow_matching_sample(model, lr, z0, None, "euler", args.cfg_scale, num_steps=args.fine)
        row = []
        for solver, n in RUNS:
            z = R.flow_matching_sample(model, lr, z0, None, solver, args.cfg_scale, num_steps=n)
            row.append(float(np.linalg.norm(z - fine) / np.linalg.norm(fine)))
        print(f"| {name} | " + " | ".join(f"{v:.3f}" for v in row) + " |", flush=True)


if __name__ == "__main__":
    main()
