"""The gate of the kernels against the fp64 twin (tests/forward_ref.py), shared by tests/test_gpu_forward_paths.py and
tests/test_gpu_widths.py — test infrastructure.

`exact` = the twin with rnd = identity, `rounded` = the twin rounding to the library's operand dtype.  E0 = error(rounded vs
exact) on the same inputs is a property of the reference alone; a correct kernel rounds at the twin's points and differs only in
fp32 accumulation order and isolated last-bit flips, so its error has E0's statistics:

    error(kernel vs exact) <= F * E0,  F = 1.5, one F for every shape of every section of both files
"""
import torch

F = 1.5


def check(tag, got, base, ref64, ref_r):
    """The section's checks on one output: finite; the error of `got - base` against the exact twin within F * E0 — whole
    tensor, every sample alone, max-abs — where E0 is the rounded twin's error on the same rows.  Returns the worst ratio."""
    assert bool(torch.isfinite(got).all()), tag
    g, e, r = got.double() - base, ref64 - base, ref_r - base
    B = g.shape[0]
    err, e0 = float((g - e).norm() / e.norm()), float((r - e).norm() / e.norm())
    flat = lambda t: t.reshape(B, -1)   # noqa: E731
    err_b = (flat(g - e).norm(dim=1) / flat(e).norm(dim=1)).cpu()
    e0_b = (flat(r - e).norm(dim=1) / flat(e).norm(dim=1)).cpu()
    ma, ma0 = float((g - e).abs().max()), float((r - e).abs().max())
    worst_b = int((err_b / e0_b).argmax())
    near = float((g - r).norm() / e.norm())      # printed only: how far the kernel is from the ROUNDED twin (flips, summation order)
    print(f"{tag}: error {err:.3e} / E0 {e0:.3e} = {err / e0:.3f}; worst sample {worst_b}: {float(err_b[worst_b]):.3e} / "
          f"{float(e0_b[worst_b]):.3e} = {float((err_b / e0_b).max()):.3f}; max-abs {ma:.3e} / {ma0:.3e} = {ma / ma0:.3f}; "
          f"vs the rounded twin {near:.3e}")
    assert err <= F * e0, tag
    assert bool((err_b <= F * e0_b).all()), (tag, worst_b)
    assert ma <= F * ma0, tag
    return max(err / e0, float((err_b / e0_b).max()), ma / ma0)
