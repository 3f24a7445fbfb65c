"""The V3-MOD3 trainer on the GPU (train_ddp_v3mod3.py: reconstruction_weight * Charbonnier + latent_loss_weight * latent perceptual
loss, the Charbonnier term inside the latent loss kernels): `Trainer(loss="charbonnier_latent")`, `jat_trainer_set_loss_ex`,
`validate`, accumulation, the fp16 library, and `python -m jatsr_amd.fit --loss charbonnier_latent`.

Step fixtures: tests/golden/train_{micro,tiny}_mod3{,fw0}_T*.npz (tools/gen_golden_mod3.py: the reference's model and loss functions
under fp64 autograd).  Gates are those tests/test_gpu_train.py applies to the train_*_mod2* cases: the fw = 0 twins against the
reference's gradients directly, the fw = 0.5 cases against the fp64 oracle backward driven by the twin's d loss / d pred at the HIP
prediction (the log-magnitude gradient is ill-conditioned in the prediction, see test_v3mod2_step_vs_reference_golden)."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import jatsr_amd._lib as L  # noqa: E402
import jatsr_amd.io as jio  # noqa: E402
import jatsr_amd.recipe as recipe  # noqa: E402
import mod3_loss_ref as M3  # noqa: E402
from helpers import load_golden, rel_l2  # noqa: E402
from jatsr_amd import fit as F  # noqa: E402
from jatsr_amd.model import JaT_AudioSR_V2  # noqa: E402
from jatsr_amd.prepare import final_stats  # noqa: E402
from jatsr_amd.train import Trainer  # noqa: E402
from oracle import jat_oracle_train as OT  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP16 = L.OPERAND_DTYPE == "fp16"
FP16_TEST_SCALE = 4096.0
GRAD_TOL, GRAD_TOL_SMALL = 3e-2, 8e-2          # tests/test_gpu_train.py
LOSS_TOL, GNORM_TOL = 2e-3, 1e-2
TERMS = ("total", "mse", "freq", "ms", "consistency", "latent")


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def gsub(a, meta):
    s = meta["strides"]
    a = np.asarray(a)
    if a.size <= meta["full_limit"] or a.ndim != 2:
        return a if a.size <= meta["full_limit"] else a.reshape(-1)[::(meta.get("stride1d") or s[0] * s[1])]
    return a[::s[0], ::s[1]]


def loss_kw(meta):
    return dict(loss="charbonnier_latent", charbonnier_eps=meta["eps"], reconstruction_weight=meta["rw"],
                latent_loss_weight=meta["lw"], freq_loss_weight=meta["fw"], ms_loss_weight=meta["mw"], consistency_weight=meta["cw"])


def twin_kw(meta):
    return dict(recon_eps=meta["eps"], recon_weight=meta["rw"], latent_weight=meta["lw"], freq_weight=meta["fw"],
                ms_weight=meta["mw"], consistency_weight=meta["cw"])


def make_trainer(meta, **kw):
    L.require_gpu()
    cfg = recipe.CONFIGS[meta["cfg"]]
    m = JaT_AudioSR_V2(**cfg, dropout=0.0, drop_path_rate=0.0)
    sd = {k: torch.from_numpy(v) for k, v in recipe.make_state_dict(cfg, "ln", meta["salt"]).items()}
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all(".rope." in k for k in missing)
    kw = dict(dict(use_grad_scaler=False, condition_noise_ratio=0.0, lr=5e-5, weight_decay=0.1, grad_clip=1.0), **kw)
    tr = Trainer(m.to("cuda"), batch_size=meta["B"], frames=meta["T"], **kw)
    if FP16 and not kw["use_grad_scaler"]:
        tr.scaler.scale = FP16_TEST_SCALE      # gradients of 1e-6 sit in fp16's denormal range: a fixed loss scale, divided out below
    return m, tr


def step_tensors(meta):
    cfg = recipe.CONFIGS[meta["cfg"]]
    C, B, T, salt = cfg["input_channels"], meta["B"], meta["T"], meta["salt"]
    hr = cuda(recipe.gaussian("train_hr", (B, C, T), salt + 300))
    lr = cuda(recipe.gaussian("train_lr", (B, C, T), salt + 301))
    noise = cuda(recipe.gaussian("train_noise", (B, C, T), salt + 302))
    cn = cuda((meta["cond_noise_ratio"] * recipe.gaussian("train_cnoise", (B, C, T), salt + 303)).astype(np.float32))
    t = cuda(np.asarray(meta["t"], np.float32))
    return hr, lr, noise, cn, t


def run_step(meta, **kw):
    m, tr = make_trainer(meta, **dict(loss_kw(meta), **kw))
    hr, lr, noise, cn, t = step_tensors(meta)
    z_t, t2, _ = tr.prepare(hr, lr, noise=noise, cfg_mask=torch.zeros(meta["B"], dtype=torch.bool), t=t)
    cond_in = lr + cn
    pred = tr.forward_backward(z_t, t2, cond_in, hr, cond_clean=lr, want_pred=True)
    return tr, (z_t, t2, cond_in, hr, lr), pred


@pytest.mark.parametrize("name", ["train_micro_mod3_T24", "train_tiny_mod3_T128"])
def test_step_fixture_reference_settings(name):
    """fw = 0.5: the loss and its parts against the reference, the gradients and the clip norm against the fp64 oracle backward
    driven by the twin's d loss / d pred evaluated at the HIP prediction."""
    z, meta = load_golden(name)
    tr, (z_t, t2, cond_in, hr, lr), pred = run_step(meta)
    terms = tr.loss_terms()
    assert abs(terms["total"] - float(z["loss64"])) <= LOSS_TOL * float(z["loss64"]), (terms, float(z["loss64"]))
    assert abs(terms["mse"] - float(z["recon"])) <= LOSS_TOL * float(z["recon"]) and terms["reconstruction"] == terms["mse"]
    assert abs(terms["latent"] - float(z["latent"])) <= 5e-3 * float(z["latent"])
    cfg = recipe.CONFIGS[meta["cfg"]]
    orc = OT.TrainOracle(cfg, recipe.make_state_dict(cfg, "ln", meta["salt"]), "ln")
    orc.forward(z_t.cpu().numpy(), t2.cpu().numpy(), cond_in.cpu().numpy())
    _, dp_hip = M3.mod3_loss(pred.cpu().numpy(), hr.cpu().numpy(), lr.cpu().numpy(), **twin_kw(meta))
    grads = orc.backward(dp_hip)
    gn = math.sqrt(sum(float((g * g).sum()) for g in grads.values()))
    worst, sq = ("", 0.0), 0.0
    for k in meta["names"]:
        g = (tr.grad(k) / tr.scaler.scale).cpu().numpy()
        sq += float((g.astype(np.float64) ** 2).sum())
        r = rel_l2(g, grads[k])
        tol = GRAD_TOL if np.linalg.norm(grads[k]) >= 1e-3 * gn else GRAD_TOL_SMALL
        if r / tol > worst[1]:
            worst = (k, r / tol)
        assert r <= tol, f"{k}: grad rel-L2 {r:.3e}"
    print(f"{name}: {terms}; gnorm {sq ** 0.5:.5f} (oracle {gn:.5f}); worst tensor {worst[0]} at {worst[1]:.2f} of tolerance")
    assert abs(sq ** 0.5 - gn) <= GNORM_TOL * gn
    loss, clip_norm = tr.optimizer_step()
    assert loss == terms["total"] and abs(clip_norm - sq ** 0.5) <= 1e-4 * clip_norm


@pytest.mark.parametrize("name", ["train_micro_mod3fw0_T24", "train_tiny_mod3fw0_T128"])
def test_step_fixture_vs_reference_autograd_conditioned(name):
    """fw = 0: loss, every parameter gradient and the clip norm against the REFERENCE's own autograd, at the gates of
    test_v3mod2_step_gradients_vs_reference_autograd_conditioned (per tensor 2 x the MSE-only tolerance: 6e-2, small tensors 1.6e-1;
    clip norm 2e-2).  Before that, the backward chain alone: every tensor against the fp64 oracle backward driven by the twin's
    d loss / d pred at the HIP prediction, at the plain per-tensor tolerance.

    Conditioning.  With eps = 1e-6 the Charbonnier gradient e / sqrt(e^2 + eps) / n is +-1/n for |e| >> 1e-3, a sign function: the
    bf16 forward moves the prediction by rel-L2 4.5e-3 / 4.8e-3, sign(pred - target) flips on 0.07 % of the elements, each changing by
    2/n, and d loss / d pred differs by rel-L2 0.038 / 0.040 between the HIP and the fp64 prediction (printed below).  The parameter
    gradients therefore sit at 3-5e-2 from the reference's, noise-like, ten times what an MSE step shows (tools/mod3_conditioning.py
    reproduces this in fp64), and the comparison needs a sample of each large matrix that can carry a rel-L2: the fixtures store
    >= 2000 (micro) / >= 400 (tiny) strided values per matrix.  MEASURED, bf16 library: worst tensor against the reference 5.3e-2
    (micro, blocks.1.attn.q_proj.weight) and 4.9e-2 (tiny, blocks.6.attn.v_proj.weight), gate 6e-2; on whole tensors against the
    oracle backward at the fp64 prediction 5.1e-2 and 4.0e-2; against the oracle backward at the HIP prediction 0.36 / 0.38 of the
    tolerance.  (With the 25-value samples that strides (61, 53) leave of a tiny matrix, five attn.out_proj.weight tensors whose
    whole-tensor deviation is 2.5-2.8e-2 read 7e-2 to 1.3e-1.)  The fp16 library: 1.6e-3."""
    z, meta = load_golden(name)
    assert meta["fw"] == 0.0
    tr, (z_t, t2, cond_in, hr, lr), pred = run_step(meta)
    terms = tr.loss_terms()
    assert abs(terms["total"] - float(z["loss64"])) <= LOSS_TOL * float(z["loss64"]), (terms, float(z["loss64"]))
    assert abs(terms["mse"] - float(z["recon"])) <= LOSS_TOL * float(z["recon"])
    cfg = recipe.CONFIGS[meta["cfg"]]
    orc = OT.TrainOracle(cfg, recipe.make_state_dict(cfg, "ln", meta["salt"]), "ln")
    opred = orc.forward(z_t.cpu().numpy(), t2.cpu().numpy(), cond_in.cpu().numpy())
    hp, hh, hl = pred.cpu().numpy(), hr.cpu().numpy(), lr.cpu().numpy()
    _, dp_hip = M3.mod3_loss(hp, hh, hl, **twin_kw(meta))
    _, dp_ref = M3.mod3_loss(opred, hh, hl, **twin_kw(meta))
    flips = float(np.mean(np.sign(hp.astype(np.float64) - hh) != np.sign(opred - hh)))
    print(f"{name}: pred rel-L2 {rel_l2(hp, opred):.2e} -> d loss/d pred changes by rel-L2 {rel_l2(dp_hip, dp_ref):.3f}, "
          f"sign(pred - target) flips on {flips:.2%} of the elements")
    ograds = orc.backward(dp_hip)
    gn_ref = math.sqrt(sum(float(z["gl2_" + k]) ** 2 for k in meta["names"]))
    worst_o, worst, sq, rs = ("", 0.0), ("", 0.0, 0.0), 0.0, {}
    for k in meta["names"]:
        g = (tr.grad(k).detach() / tr.scaler.scale).cpu().numpy()
        sq += float((g.astype(np.float64) ** 2).sum())
        ref_l2 = float(z["gl2_" + k])
        tol = GRAD_TOL if ref_l2 >= 1e-3 * gn_ref else GRAD_TOL_SMALL
        ro = rel_l2(g, ograds[k])
        if ro / tol > worst_o[1]:
            worst_o = (k, ro / tol)
        assert ro <= tol, f"{k}: grad rel-L2 {ro:.3e} vs the oracle backward"
        rs[k] = (rel_l2(gsub(g, meta), z["g_" + k]), 2 * tol, ref_l2)
        if rs[k][0] / rs[k][1] > worst[1]:
            worst = (k, rs[k][0] / rs[k][1], rs[k][0])
    over = {k: f"{v[0]:.3e}" for k, v in rs.items() if v[0] > v[1]}
    # the same comparison on WHOLE tensors: the oracle backward at the fp64 prediction is the reference's gradient (pinned to 5e-4 by
    # tests/test_mod3_cpu.py), where the fixture keeps a strided sample of the large matrices (25 values of a tiny-preset weight)
    full_ref = orc.backward(dp_ref)
    full = {k: rel_l2((tr.grad(k).detach() / tr.scaler.scale).cpu().numpy(), full_ref[k]) for k in meta["names"]}
    print(f"{name}: whole tensors vs the oracle backward at the fp64 prediction: worst {max(full, key=full.get)} {max(full.values()):.3e}; "
          f"the tensors over their gate above: { {k: f'{full[k]:.3e}' for k in over} }")
    print(f"{name}: {terms}; gnorm {sq ** 0.5:.5f} (ref {gn_ref:.5f}); vs the oracle backward: worst tensor {worst_o[0]} at "
          f"{worst_o[1]:.2f} of tolerance; vs reference autograd: worst tensor {worst[0]} rel-L2 {worst[2]:.3e} at {worst[1]:.2f} of "
          f"tolerance, {len(over)} of {len(rs)} tensors over their gate: {over}")
    assert abs(sq ** 0.5 - gn_ref) <= 2 * GNORM_TOL * gn_ref
    _, clip_norm = tr.optimizer_step()
    assert abs(clip_norm - gn_ref) <= 2 * GNORM_TOL * gn_ref
    for k, (r, tol, ref_l2) in rs.items():
        assert r <= tol, f"{k}: grad rel-L2 {r:.3e} vs reference autograd (ref norm {ref_l2:.3e})"


def test_validate_returns_the_twins_loss_and_the_five_metrics():
    """validate(): the training loss, reconstruction weight included (train_ddp_v3mod3.py:1138-1159), through jat_k_latent_loss_ex;
    tolerances of test_validate_and_checkpoint_roundtrip."""
    z, meta = load_golden("train_micro_mod3_T24")
    meta = dict(meta, rw=0.5)
    m, tr = make_trainer(meta, **loss_kw(meta))
    cfg = recipe.CONFIGS[meta["cfg"]]
    C, B = cfg["input_channels"], meta["B"]
    hr, lr, noise, _, t = step_tensors(meta)
    mean, std = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    avg, sd_, metrics = tr.validate([(hr, lr), (lr, hr)], mean, std, mean, std, t=[t, t], noise=[noise, noise])
    orc = OT.TrainOracle(cfg, recipe.make_state_dict(cfg, "ln", meta["salt"]), "ln")
    ref = []
    for a, b_ in ((hr, lr), (lr, hr)):
        an, bn, nz, tn = (x.cpu().numpy().astype(np.float64) for x in (a, b_, noise, t))
        tv = tn.reshape(B, 1, 1)
        ref.append(M3.mod3_loss(orc.forward(tv * an + (1 - tv) * nz, tn, bn), an, bn, **twin_kw(meta))[0])
    assert sorted(metrics) == sorted(("mse_loss", "freq_loss", "ms_loss", "consistency_loss", "total_latent_loss"))
    assert abs(avg - np.mean([r["total"] for r in ref])) <= 3e-3 * avg
    assert abs(metrics["mse_loss"] - np.mean([r["mse"] for r in ref])) <= 3e-3 * metrics["mse_loss"]      # un-weighted Charbonnier mean
    assert abs(metrics["consistency_loss"] - np.mean([r["consistency"] for r in ref])) <= 1e-2 * metrics["consistency_loss"]
    assert abs(avg - (0.5 * metrics["mse_loss"] + meta["lw"] * metrics["total_latent_loss"])) <= 1e-6 * avg
    assert sd_ == pytest.approx(float(np.std([r["total"] for r in ref], ddof=1)), rel=0.05)


def test_set_loss_ex_validates_first_and_the_old_setters_keep_rejecting_each_other():
    z, meta = load_golden("train_micro_mod3_T24")
    tr, x, _ = run_step(meta)
    lib = L.lib()
    before, terms_before = tr.grads.clone(), tr.loss_terms()
    cuts = (0.3, 0.30, 0.36)
    # after jat_trainer_set_loss_ex stored Charbonnier AND a latent weight, each old setter still refuses what it always refused
    assert lib.jat_trainer_set_charbonnier(tr.ptr, 1e-6) == L.JAT_E_STATE
    assert lib.jat_trainer_set_latent_loss(tr.ptr, 0.3, 0.5, 0.5, 0.1, *cuts) == L.JAT_E_STATE
    for bad in ((-1e-6, 1.0, 0.3, 0.5, 0.5, 0.1) + cuts, (float("nan"), 1.0, 0.3, 0.5, 0.5, 0.1) + cuts,
                (1e-6, float("nan"), 0.3, 0.5, 0.5, 0.1) + cuts, (1e-6, 1.0, float("inf"), 0.5, 0.5, 0.1) + cuts,
                (1e-6, 1.0, 0.3, 0.5, float("nan"), 0.1) + cuts, (1e-6, 1.0, 0.3, 0.5, 0.5, 0.1, 0.3, 0.36, 0.30),
                (1e-6, 1.0, 0.3, 0.5, 0.5, 0.1, 1.25, 0.30, 0.36)):
        assert lib.jat_trainer_set_loss_ex(tr.ptr, *bad) == L.JAT_E_INVALID, bad
    # nothing was stored by the rejected calls: the same step gives the same bits
    z_t, t2, cond_in, hr, lr = x
    tr.forward_backward(z_t, t2, cond_in, hr, cond_clean=lr)
    assert torch.equal(tr.grads, before) and tr.loss_terms() == terms_before
    # a reconstruction weight of 0 is legal: the total is lw * latent, slot 1 still the Charbonnier mean
    L.check(lib.jat_trainer_set_loss_ex(tr.ptr, meta["eps"], 0.0, meta["lw"], meta["fw"], meta["mw"], meta["cw"], *cuts))
    tr.forward_backward(z_t, t2, cond_in, hr, cond_clean=lr)
    t0 = tr.loss_terms()
    assert t0["mse"] == terms_before["mse"] and t0["latent"] == terms_before["latent"]
    assert abs(t0["total"] - float(np.float32(meta["lw"])) * t0["latent"]) <= 2.0 ** -23 * t0["total"]
    # back on MSE with weight 1 the old setters work again
    L.check(lib.jat_trainer_set_loss_ex(tr.ptr, 0.0, 1.0, 0.0, 0.5, 0.5, 0.1, *cuts))
    assert lib.jat_trainer_set_charbonnier(tr.ptr, 1e-6) == L.JAT_OK


def test_two_equal_micro_batches_step_like_one():
    """k = 2 times the same micro-batch: the gradient sums and the loss cells double exactly and the 1 / (scale * k) is a power of
    two, so the step, the loss and the six terms are those of the plain step, bit for bit."""
    z, meta = load_golden("train_micro_mod3_T24")
    kw = dict(loss_kw(meta), lr=1e-4)
    hr, lr, noise, cn, t = step_tensors(meta)
    m0, tr0 = make_trainer(meta, **kw)
    z_t, t2, _ = tr0.prepare(hr, lr, noise=noise, cfg_mask=torch.zeros(meta["B"], dtype=torch.bool), t=t)
    x = (z_t, t2, lr + cn, hr)
    tr0.forward_backward(*x, cond_clean=lr)
    terms0 = tr0.loss_terms()
    loss0, norm0 = tr0.optimizer_step(lr=1e-3)
    m1, tr1 = make_trainer(meta, grad_accum_steps=2, **kw)
    for _ in range(2):
        tr1.forward_backward(*x, cond_clean=lr, mask_seed=tr1.step_seed())
    terms1 = tr1.loss_terms()
    loss1, norm1 = tr1.optimizer_step(lr=1e-3)
    torch.cuda.synchronize()
    assert (loss1, norm1) == (loss0, norm0) and math.isfinite(norm0) and norm0 > 0
    assert terms1 == terms0 and tr1.loss_terms() == terms0 and loss0 == terms0["total"]
    assert torch.equal(tr1.params, tr0.params) and torch.equal(tr1.exp_avg, tr0.exp_avg) and torch.equal(tr1.exp_avg_sq, tr0.exp_avg_sq)


def test_fp16_library_runs_the_mod3_step():
    """The fp16-operand library (the v3mod3 trainer's autocast dtype) is a process-level choice: a child process runs the micro
    fw = 0 step fixture against it at loss scale 4096, same gates."""
    env = dict(os.environ, JAT_OPERAND_DTYPE="fp16")
    env.pop("JAT_LIB_PATH", None)
    out = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-s", "-p", "no:cacheprovider", "-m", "gpu",
                          "tests/test_gpu_mod3_train.py", "-k", "conditioned and micro_mod3fw0"], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=300)
    tail = (out.stdout + out.stderr)[-3000:]
    print(tail)
    assert out.returncode == 0 and "1 passed" in out.stdout, tail


# ---- python -m jatsr_amd.fit --loss charbonnier_latent -------------------------------------------------------------------------
C_, FRAMES, BATCH = 32, 40, 2


def write_folder(root):
    g = torch.Generator().manual_seed(4321)
    s, q, count = torch.zeros(2 * C_, dtype=torch.float64), torch.zeros(2 * C_, dtype=torch.float64), 0
    scale = torch.linspace(0.5, 2.0, C_).view(-1, 1)
    for split, lengths in (("train", [64, 41, 90, 58]), ("val", [50, 44])):
        os.makedirs(os.path.join(root, split))
        for i, n in enumerate(lengths):
            hr = (torch.randn(C_, n, generator=g) * scale + 0.3).to(torch.float16)
            lr = (hr.float() * 0.7 + torch.randn(C_, n, generator=g) * 0.2 - 0.1).to(torch.float16)
            jio.save_latent_file(os.path.join(root, split, f"clip_{i:03d}.pt"), hr_latent=hr, lr_latent=lr, metadata={"name": str(i)})
            if split == "train":
                both = torch.cat([hr, lr]).double()
                s += both.sum(1)
                q += (both ** 2).sum(1)
                count += n
    with open(os.path.join(root, "global_stats_separated.json"), "w") as f:
        json.dump(final_stats(s, q, count, C_), f)
    return root


def fit_args(data_dir, base, *more):
    argv = ["--data-dir", data_dir, "--save-dir-base", base, "--preset", "micro", "--model", "v2", "--frames", str(FRAMES),
            "--batch-size", str(BATCH), "--epochs", "2", "--samples-per-epoch-multiplier", "1", "--log-interval", "1",
            "--warmup-steps", "3", "--lr", "1e-3", "--seed", "7", "--loss", "charbonnier_latent"]
    return F.build_parser().parse_args(argv + list(more))


def read_log(folder):
    with open(os.path.join(folder, "train_log.jsonl")) as f:
        return [json.loads(line) for line in f]


def test_fit_runs_the_mod3_trainer(tmp_path):
    data_dir = write_folder(str(tmp_path / "prepared"))
    base = str(tmp_path / "ck")
    first = F.run(fit_args(data_dir, base, "--max-steps", "3"))
    assert first["global_step"] == 3 and first["trainer"].loss == "charbonnier_latent"
    steps = [r for r in read_log(first["save_dir"]) if "Train/Loss" in r]
    assert [r["step"] for r in steps] == [0, 1, 2]
    lw32 = float(np.float32(0.3))
    for r in steps:
        assert "Train/Charbonnier_Loss" in r and "Train/MSE_Loss" not in r and "Train/LatentPerc_TotalLoss" in r
        total = r["Train/Charbonnier_Loss"] + lw32 * r["Train/LatentPerc_TotalLoss"]        # rw = 1, the reference's default
        assert abs(r["Train/Loss"] - total) <= 3 * 2.0 ** -24 * total and r["Train/Charbonnier_Loss"] > 0
    vals = [r for r in read_log(first["save_dir"]) if "Val/Loss" in r]
    assert len(vals) == 1 and "Val/MSE_Loss" in vals[0] and "Val/LatentPerc_TotalLoss" in vals[0]      # the validation tags stay
    # --resume continues from last.pt (written after epoch 0: two steps), with the loss the flags select
    del first["trainer"]
    second = F.run(fit_args(data_dir, base, "--resume"))
    assert second["save_dir"] == first["save_dir"] and second["global_step"] == 4
    resumed = [r for r in read_log(second["save_dir"]) if "Train/Loss" in r][3:]
    assert [r["step"] for r in resumed] == [2, 3] and resumed[0] == steps[2]               # step 2 again, bit for bit
    assert all("Train/Charbonnier_Loss" in r and "Train/MSE_Loss" not in r for r in resumed)
    # --reconstruction-weight 0.5: the same first step (same weights, draws and masks), the total lower by half the Charbonnier term
    half = F.run(fit_args(data_dir, str(tmp_path / "ck_half"), "--max-steps", "1", "--reconstruction-weight", "0.5"))
    h = [r for r in read_log(half["save_dir"]) if "Train/Loss" in r][0]
    a = steps[0]
    assert h["Train/Charbonnier_Loss"] == a["Train/Charbonnier_Loss"] and h["Train/LatentPerc_TotalLoss"] == a["Train/LatentPerc_TotalLoss"]
    # each total is one fp32 rounding of its fp64 sum, the logged term one rounding of its fp64 value
    assert abs((a["Train/Loss"] - h["Train/Loss"]) - 0.5 * a["Train/Charbonnier_Loss"]) <= 3 * 2.0 ** -24 * a["Train/Loss"]
    assert h["Train/Loss"] < a["Train/Loss"]
