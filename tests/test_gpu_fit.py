"""The training-run driver on the GPU (jatsr_amd.fit) at micro dimensions on a synthetic prepared folder: the files a run
leaves, the log's tags, checkpoints that load, per-step losses equal to hand-written loops (through `step_normalised` and
through the existing `train_step` on raw fp32 crops), a resumed run that continues bit for bit, a validation set too small
for one batch, and a mistyped --loss that fails before any device memory is taken."""
import json
import os
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

import jatsr_amd  # noqa: E402
import jatsr_amd.io as jio  # noqa: E402
from jatsr_amd import fit as F  # noqa: E402
from jatsr_amd.data import LatentStore, epoch_batches, train_batch_plan  # noqa: E402
from jatsr_amd.model import JaT_AudioSR_V3  # noqa: E402
from jatsr_amd.prepare import final_stats  # noqa: E402

C_, FRAMES, BATCH = 32, 40, 2
TRAIN_LENGTHS = [64, 41, 25, 90, 40, 77, 58, 120]       # one shorter than FRAMES, one equal, odd and even
VAL_LENGTHS = [50, 44, 95, 61]
TRAIN_TAGS = ["Train/Loss", "Train/LR", "Train/GradNorm", "Train/SNR_dB", "Train/PredictionMean", "Train/PredictionStd",
              "Train/CondNoiseStd", "Train/MSE_Loss", "Train/LatentPerc_FreqLoss", "Train/LatentPerc_MSLoss",
              "Train/LatentPerc_ConsistencyLoss", "Train/LatentPerc_TotalLoss"]


def write_folder(root, train_lengths, val_lengths):
    g = torch.Generator().manual_seed(1234)
    s = torch.zeros(2 * C_, dtype=torch.float64)
    q = torch.zeros(2 * C_, dtype=torch.float64)
    count = 0
    scale = torch.linspace(0.5, 2.0, C_).view(-1, 1)
    for split, lengths in (("train", train_lengths), ("val", val_lengths)):
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
    argv = ["--data-dir", data_dir, "--save-dir-base", base, "--preset", "micro", "--model", "v3", "--frames", str(FRAMES),
            "--batch-size", str(BATCH), "--epochs", "2", "--samples-per-epoch-multiplier", "1", "--save-interval-steps", "2",
            "--log-interval", "1", "--warmup-steps", "3", "--lr", "1e-3", "--seed", "7"]
    return F.build_parser().parse_args(argv + list(more))


def read_log(folder):
    with open(os.path.join(folder, "train_log.jsonl")) as f:
        return [json.loads(line) for line in f]


@pytest.fixture(scope="module")
def data_dir(tmp_path_factory):
    return write_folder(str(tmp_path_factory.mktemp("prepared")), TRAIN_LENGTHS, VAL_LENGTHS)


@pytest.fixture(scope="module")
def full_run(data_dir, tmp_path_factory):
    base = str(tmp_path_factory.mktemp("ck_full"))
    args = fit_args(data_dir, base)
    return args, F.run(args)


def test_run_writes_checkpoints_and_log(full_run):
    args, res = full_run
    base = args.save_dir_base
    assert [d for d in os.listdir(base)] == [os.path.basename(res["save_dir"])] and re.fullmatch(r"\d{8}", os.listdir(base)[0])
    names = sorted(os.listdir(res["save_dir"]))
    per_epoch = len(TRAIN_LENGTHS) // BATCH
    assert res["global_step"] == 2 * per_epoch == 8
    assert {"last.pt", "best.pt", "train_log.jsonl", "interval_step_2.pt", "interval_step_4.pt", "interval_step_6.pt"} <= set(names)
    log = read_log(res["save_dir"])
    steps = [r for r in log if "Train/Loss" in r]
    vals = [r for r in log if "Val/Loss" in r]
    assert [r["step"] for r in steps] == list(range(8)) and [r["epoch"] for r in vals] == [0, 1]
    for r in steps:
        assert all(k in r and isinstance(r[k], float) and r[k] == r[k] for k in TRAIN_TAGS), r
        assert r["Train/LR"] == jatsr_amd.get_lr(r["step"], 8, 3, 1e-3)
    for r in vals:
        assert r["Val/Loss"] > 0 and "Val/Loss_Std" in r and "Val/MSE_Loss" in r and "Val/LatentPerc_TotalLoss" in r
    assert res["best_val_loss"] == min(r["Val/Loss"] for r in vals)
    assert 0.05 * 0.5 <= steps[0]["Train/CondNoiseStd"] <= 0.05 * 2.0
    # the checkpoints load: the inference loader, and a fresh trainer
    last = os.path.join(res["save_dir"], "last.pt")
    ck = torch.load(last, map_location="cpu", weights_only=False)
    assert ck["epoch"] == 1 and ck["global_step"] == 8 and ck["fit_args"]["frames"] == FRAMES and "trainer_generator" in ck["rng_state"]
    model = jatsr_amd.load_model(last, cls=JaT_AudioSR_V3)
    tr = res["trainer"]
    for k, p in model.named_parameters():
        assert torch.equal(p.data, dict(tr.model.named_parameters())[k].data), k
    fresh = F.build_trainer(args, F.build_model(args, "cuda"), 8)
    assert fresh.load_checkpoint(last) == 1
    assert (fresh.global_step, fresh.opt_step, fresh.scaler.scale) == (tr.global_step, tr.opt_step, tr.scaler.scale)
    assert torch.equal(fresh.params, tr.params) and torch.equal(fresh.exp_avg, tr.exp_avg) and torch.equal(fresh.exp_avg_sq, tr.exp_avg_sq)


def hand_loop(args, data_dir, raw):
    """The driver's loop written out: raw=False through store.batch + step_normalised, raw=True through the existing
    train_step on the same crops as raw fp32 tensors."""
    store = LatentStore(data_dir, "train", FRAMES, "cuda")
    stats = jio.load_stats(os.path.join(data_dir, "global_stats_separated.json"), channels=C_, device="cuda")
    per_epoch = len(epoch_batches(len(store), 1, BATCH, 0, 0, 1, True, args.seed))
    trainer = F.build_trainer(args, F.build_model(args, "cuda"), per_epoch * args.epochs)
    files_cpu = [torch.load(p, weights_only=False) for p in store.files]
    losses = []
    for epoch in range(args.epochs):
        for batch in epoch_batches(len(store), 1, BATCH, epoch, 0, 1, True, args.seed):
            files, starts = train_batch_plan(store.lengths, FRAMES, batch, args.seed, epoch)
            if raw:
                idx = [(torch.arange(FRAMES) + s) % store.lengths[f] for f, s in zip(files, starts)]
                hr = torch.stack([files_cpu[f]["hr_latent"][:, j] for f, j in zip(files, idx)]).float()
                lr = torch.stack([files_cpu[f]["lr_latent"][:, j] for f, j in zip(files, idx)]).float()
                out = trainer.train_step(hr, lr, stats["hr_mean"], stats["hr_std"], stats["lr_mean"], stats["lr_std"])
            else:
                out = trainer.step_normalised(*store.batch(files, starts, stats))
            losses.append(out["loss"])
    return losses, trainer


@pytest.mark.parametrize("raw", [False, True])
def test_losses_equal_hand_written_loop(full_run, data_dir, raw):
    args, res = full_run
    logged = [r["Train/Loss"] for r in read_log(res["save_dir"]) if "Train/Loss" in r]
    losses, trainer = hand_loop(args, data_dir, raw)
    assert losses == logged                                   # floats compared exactly: bit for bit
    assert torch.equal(trainer.params, res["trainer"].params)


def test_resume_continues_bit_for_bit(full_run, data_dir, tmp_path):
    args, res = full_run
    base = str(tmp_path / "ck_resume")
    first = F.run(fit_args(data_dir, base, "--max-steps", "4"))
    assert first["global_step"] == 4 and os.path.exists(os.path.join(first["save_dir"], "last.pt"))
    assert [r["step"] for r in read_log(first["save_dir"]) if "Train/Loss" in r] == [0, 1, 2, 3]
    del first["trainer"]
    second = F.run(fit_args(data_dir, base, "--resume"))
    assert second["save_dir"] == first["save_dir"] and second["global_step"] == 8 and len(os.listdir(base)) == 1
    a, b = res["trainer"], second["trainer"]
    assert torch.equal(a.params, b.params) and torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq)
    assert (a.opt_step, a.scaler.scale) == (b.opt_step, b.scaler.scale)
    full_log, resumed_log = read_log(res["save_dir"]), read_log(second["save_dir"])
    assert [r for r in resumed_log if "Train/Loss" in r] == [r for r in full_log if "Train/Loss" in r]
    assert [r for r in resumed_log if "Val/Loss" in r] == [r for r in full_log if "Val/Loss" in r]
    # --resume PATH resumes into that file's folder
    third = F.run(fit_args(data_dir, base, "--resume", os.path.join(first["save_dir"], "last.pt")))
    assert third["save_dir"] == first["save_dir"] and third["global_step"] == 8      # both epochs were done: nothing left to run


def test_validation_set_too_small_for_a_batch(tmp_path, capsys):
    d = write_folder(str(tmp_path / "prepared"), TRAIN_LENGTHS[:4], VAL_LENGTHS[:1])
    res = F.run(fit_args(d, str(tmp_path / "ck"), "--epochs", "1"))
    assert res["global_step"] == 2 and res["best_val_loss"] == float("inf")
    names = os.listdir(res["save_dir"])
    assert "last.pt" in names and "best.pt" not in names
    log = read_log(res["save_dir"])
    assert any("Val/Skipped" in r for r in log) and not any("Val/Loss" in r for r in log)
    assert "validation skipped" in capsys.readouterr().out


def test_bad_loss_fails_before_any_workspace(data_dir, tmp_path):
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with pytest.raises(ValueError, match="loss must be"):
        F.run(fit_args(data_dir, str(tmp_path / "ck"), "--loss", "charbonier"))
    assert torch.cuda.memory_allocated() == before and not os.path.exists(str(tmp_path / "ck"))
    model = F.build_model(fit_args(data_dir, str(tmp_path / "ck")), "cuda")
    before = torch.cuda.memory_allocated()
    with pytest.raises(ValueError, match="loss must be"):
        jatsr_amd.Trainer(model, BATCH, FRAMES, loss="charbonier")
    with pytest.raises(ValueError, match="latent"):
        jatsr_amd.Trainer(model, BATCH, FRAMES, loss="charbonnier", latent_loss_weight=0.3)
    assert torch.cuda.memory_allocated() == before
