"""Training run on MI355X — one rank of reference `train_ddp_v3mod2.py:main` (:603-1018), or of `train_ddp_v3m2.py` /
`train_ddp_v3m2mod1.py` by flag (`--model v3 --latent-loss-weight 0 [--loss charbonnier]`), or of `train_ddp_v3mod3.py`
(`--loss charbonnier_latent`: Charbonnier + latent perceptual loss with configurable weights).

    python -m jatsr_amd.fit --data-dir data_processed_v13_final --save-dir-base checkpoints/v3mod2_full_run
    python -m jatsr_amd.fit --data-dir ... --resume                 # newest run folder; --resume PATH for a given file
    torchrun --nproc_per_node=8 -m jatsr_amd.fit --data-dir ...     # RANK / WORLD_SIZE in the environment: one rank each

The prepared folder (`python -m jatsr_amd.prepare`) is held in HBM as fp16 (`jatsr_amd.data.LatentStore`); each step's batch
is cropped, converted and normalised by one kernel and goes through `Trainer.step_normalised`.  The host code here is the
bookkeeping: epoch order and rank shard, learning rate, log lines, validation, checkpoint rotation, resume.  TensorBoard is
replaced by `train_log.jsonl` in the run folder, one JSON object per logged step / epoch under the reference's tag names.
"""
from __future__ import annotations

import argparse
import glob
import json
import os
import sys
import time
from datetime import datetime

# TrainConfig of train_ddp_v3mod2.py:327-386
DEFAULTS = dict(seed=42, data_dir="data_processed_v13_final", stats_file="global_stats_separated.json", target_duration=16.0,
                batch_size=28, lr=5e-5, weight_decay=0.1, warmup_steps=1000, epochs=300, grad_clip=1.0,
                condition_noise_ratio=0.05, latent_loss_weight=0.3, dropout=0.1, drop_path_rate=0.05,
                save_dir_base="checkpoints/v3mod2_full_run", save_interval_steps=1000, samples_per_epoch_multiplier=6,
                log_interval=10,
                # train_ddp_v3mod3.py:408-422
                reconstruction_weight=1.0, charbonnier_eps=1e-6, freq_loss_weight=0.5, ms_loss_weight=0.5, consistency_weight=0.1)
MODEL_DIMS = ("input_channels", "patch_len", "hidden_size", "depth", "num_q_heads", "num_kv_heads", "bottleneck_dim", "mlp_ratio")
CHARBONNIER_TAG = "Train/Charbonnier_Loss"      # in place of Train/MSE_Loss with a Charbonnier loss (train_ddp_v3mod3.py:1030-1032)
TRAIN_TAGS = {"mse": "Train/MSE_Loss", "freq": "Train/LatentPerc_FreqLoss", "ms": "Train/LatentPerc_MSLoss",
              "consistency": "Train/LatentPerc_ConsistencyLoss", "latent": "Train/LatentPerc_TotalLoss"}
EMA_VAL_TAGS = {"mse_loss": "Val/EMA_MSE_Loss", "freq_loss": "Val/EMA_LatentPerc_FreqLoss", "ms_loss": "Val/EMA_LatentPerc_MSLoss",
                "consistency_loss": "Val/EMA_LatentPerc_ConsistencyLoss", "total_latent_loss": "Val/EMA_LatentPerc_TotalLoss"}
VAL_TAGS = {"mse_loss": "Val/MSE_Loss", "freq_loss": "Val/LatentPerc_FreqLoss", "ms_loss": "Val/LatentPerc_MSLoss",
            "consistency_loss": "Val/LatentPerc_ConsistencyLoss", "total_latent_loss": "Val/LatentPerc_TotalLoss"}


def _accum_steps(text):
    k = int(text)
    if k < 1:
        raise argparse.ArgumentTypeError(f"must be >= 1, got {k}")
    return k


def steps_per_epoch(n_batches, grad_accum_steps):
    """(optimiser steps, batches left over) of an epoch whose plan has n_batches batches: a step consumes grad_accum_steps
    consecutive batches, and what does not fill a step is dropped."""
    k = int(grad_accum_steps)
    if k < 1:
        raise ValueError(f"grad_accum_steps must be >= 1, got {grad_accum_steps!r}")
    return n_batches // k, n_batches % k


def build_parser():
    from .io import frames_for_seconds
    d = DEFAULTS
    p = argparse.ArgumentParser(prog="python -m jatsr_amd.fit", description="JaT-AudioSR training run on MI355X (one rank)")
    p.add_argument("--data-dir", default=d["data_dir"], help="folder with train/*.pt, val/*.pt and the statistics file")
    p.add_argument("--stats-file", default=d["stats_file"], help="normalisation statistics, relative to --data-dir unless absolute")
    p.add_argument("--frames", type=int, default=frames_for_seconds(d["target_duration"]), help="latent frames per sample (16 s = 1378)")
    p.add_argument("--batch-size", type=int, default=d["batch_size"], help="samples per rank and step")
    p.add_argument("--model", choices=["v3", "v2"], default="v2", help="v2: LayerNorm model of train_ddp_v3mod2.py; v3: RMSNorm")
    p.add_argument("--preset", choices=["v3mod2", "tiny", "micro"], default="v3mod2", help="model dimensions (recipe.CONFIGS)")
    for k in MODEL_DIMS:
        p.add_argument("--" + k.replace("_", "-"), type=float if k == "mlp_ratio" else int, default=None, help="overrides the preset")
    p.add_argument("--dropout", type=float, default=d["dropout"])
    p.add_argument("--drop-path-rate", type=float, default=d["drop_path_rate"])
    p.add_argument("--init-checkpoint", default=None, help="start from this checkpoint's weights (optimiser state is not taken)")
    p.add_argument("--epochs", type=int, default=d["epochs"])
    p.add_argument("--lr", type=float, default=d["lr"])
    p.add_argument("--weight-decay", type=float, default=d["weight_decay"])
    p.add_argument("--warmup-steps", type=int, default=d["warmup_steps"])
    p.add_argument("--grad-clip", type=float, default=d["grad_clip"])
    p.add_argument("--cfg-dropout-prob", type=float, default=0.0, help="train_ddp_v3mod2.py has none; train_ddp_v3m2.py uses 0.1")
    p.add_argument("--condition-noise-ratio", type=float, default=d["condition_noise_ratio"])
    p.add_argument("--no-adaptive-noise", dest="use_adaptive_noise", action="store_false")
    p.add_argument("--latent-loss-weight", type=float, default=d["latent_loss_weight"], help="0: MSE only (train_ddp_v3m2.py)")
    p.add_argument("--loss", default="mse",
                   help="mse, charbonnier (train_ddp_v3m2mod1.py; needs --latent-loss-weight 0) or charbonnier_latent "
                        "(train_ddp_v3mod3.py: Charbonnier + latent perceptual loss)")
    p.add_argument("--reconstruction-weight", type=float, default=d["reconstruction_weight"],
                   help="weight of the MSE / Charbonnier term (train_ddp_v3mod3.py:416)")
    p.add_argument("--charbonnier-eps", type=float, default=d["charbonnier_eps"], help="added to the squared difference (:409)")
    p.add_argument("--freq-loss-weight", type=float, default=d["freq_loss_weight"], help="inside the latent perceptual loss (:420)")
    p.add_argument("--ms-loss-weight", type=float, default=d["ms_loss_weight"], help="inside the latent perceptual loss (:421)")
    p.add_argument("--consistency-weight", type=float, default=d["consistency_weight"], help="inside the latent perceptual loss (:422)")
    p.add_argument("--ema-decay", type=float, default=None,
                   help="keep an exponential moving average of the weights with this decay (e.g. 0.9999): validated beside the "
                        "raw weights, stored in every checkpoint (infer --ema samples from it); default: none")
    p.add_argument("--no-ema-warmup", dest="ema_warmup", action="store_false",
                   help="with --ema-decay: the constant decay from the first step instead of min(decay, (1 + n) / (10 + n))")
    p.add_argument("--grad-accum-steps", type=_accum_steps, default=1,
                   help="micro-batches per optimiser step (effective batch = this x --batch-size per rank); steps, --max-steps, "
                        "--log-interval and --save-interval-steps count optimiser steps; default 1: none")
    p.add_argument("--amp-dtype", default=None, choices=["bf16", "fp16"], help="must match the loaded library (JAT_OPERAND_DTYPE)")
    p.add_argument("--samples-per-epoch-multiplier", type=int, default=d["samples_per_epoch_multiplier"])
    p.add_argument("--max-resident-gb", type=float, default=None, help="device memory for the data set; default half of what is free")
    p.add_argument("--save-dir-base", default=d["save_dir_base"])
    p.add_argument("--save-interval-steps", type=int, default=d["save_interval_steps"])
    p.add_argument("--log-interval", type=int, default=d["log_interval"])
    p.add_argument("--resume", nargs="?", const="auto", default=None, help="no value: newest run folder; or a checkpoint path")
    p.add_argument("--seed", type=int, default=d["seed"])
    p.add_argument("--max-steps", type=int, default=None, help="stop once this many steps have run (tests, smoke runs)")
    p.add_argument("--device", default="cuda", help="an AMD GPU; there is no CPU path")
    return p


def find_latest_checkpoint_dir(base_dir):
    """== find_latest_checkpoint_dir (train_ddp_v3mod2.py:397-424): the newest 8-digit sub-folder of base_dir and its
    last.pt -> (folder, checkpoint); (folder, None) when that folder holds no last.pt; (None, None) without such a folder."""
    if not os.path.exists(base_dir):
        return None, None
    subdirs = sorted((d for d in os.listdir(base_dir)
                      if os.path.isdir(os.path.join(base_dir, d)) and d.isdigit() and len(d) == 8), reverse=True)
    if not subdirs:
        return None, None
    latest = os.path.join(base_dir, subdirs[0])
    ck = os.path.join(latest, "last.pt")
    return latest, (ck if os.path.exists(ck) else None)


def resolve_run_dir(save_dir_base, resume, now=None):
    """-> (run folder, checkpoint to resume from or None), as train_ddp_v3mod2.py:622-660: a new `MMDDHHMM` folder; with
    resume == "auto" the newest run folder when it holds last.pt (else a new run); with a path, that file's folder."""
    stamp = (now or datetime.now()).strftime("%m%d%H%M")
    if resume is None:
        return os.path.join(save_dir_base, stamp), None
    if resume == "auto":
        latest, ck = find_latest_checkpoint_dir(save_dir_base)
        if ck:
            return latest, ck
        return os.path.join(save_dir_base, stamp), None
    if not os.path.exists(resume):
        raise FileNotFoundError(f"Checkpoint not found: {resume}")
    return os.path.dirname(os.path.abspath(resume)), resume


def model_config(args):
    from . import recipe
    cfg = dict(recipe.CONFIGS[args.preset])
    for k in MODEL_DIMS:
        if getattr(args, k) is not None:
            cfg[k] = getattr(args, k)
    cfg["cond_channels"] = cfg["input_channels"]
    return dict(cfg, dropout=args.dropout, drop_path_rate=args.drop_path_rate)


def build_model(args, device):
    """The model of a run: seeded construction, then --init-checkpoint's weights."""
    import torch

    from .model import JaT_AudioSR_V2, JaT_AudioSR_V3
    torch.manual_seed(args.seed)
    model = (JaT_AudioSR_V2 if args.model == "v2" else JaT_AudioSR_V3)(**model_config(args))
    if args.init_checkpoint:
        ck = torch.load(args.init_checkpoint, map_location="cpu", weights_only=False)
        sd = {k.replace("_orig_mod.", "").replace("module.", ""): torch.as_tensor(v).float()
              for k, v in ck["model_state_dict"].items()}
        model.load_state_dict(sd, strict=False)
    return model.to(device)


def build_trainer(args, model, total_steps, process_group=None, rank=0, distributed=False):
    from .train import Trainer
    return Trainer(model, batch_size=args.batch_size, frames=args.frames, lr=args.lr, weight_decay=args.weight_decay,
                   grad_clip=args.grad_clip, cfg_dropout_prob=args.cfg_dropout_prob,
                   condition_noise_ratio=args.condition_noise_ratio, use_adaptive_noise=args.use_adaptive_noise,
                   warmup_steps=args.warmup_steps, total_steps=total_steps, process_group=process_group,
                   seed=args.seed + rank, latent_loss_weight=args.latent_loss_weight, distributed=distributed,
                   amp_dtype=args.amp_dtype, loss=args.loss, ema_decay=args.ema_decay, ema_warmup=args.ema_warmup,
                   grad_accum_steps=getattr(args, "grad_accum_steps", 1), **_loss_keywords(args))


def _loss_keywords(args):
    """The loss flags a namespace carries as Trainer keywords (one written before the flags existed: Trainer's defaults)."""
    names = ("reconstruction_weight", "charbonnier_eps", "freq_loss_weight", "ms_loss_weight", "consistency_weight")
    return {k: getattr(args, k) for k in names if hasattr(args, k)}


def loop_step(trainer, store, plans, i, stats, lr, monitor):
    """The data path and the step of batch i of an epoch's plans [(files, starts)]: gather, staging of the next batch's
    host-resident crops, one optimisation step."""
    hr_norm, lr_norm = store.batch(*plans[i], stats)
    if i + 1 < len(plans):
        store.prefetch(*plans[i + 1])
    return trainer.step_normalised(hr_norm, lr_norm, monitor=monitor, lr=lr)


def loop_micro(trainer, store, plans, i, stats):
    """The same data path for a batch that is not the last micro-batch of its optimiser step (--grad-accum-steps): its
    gradients are added up, nothing steps and the host does not wait."""
    hr_norm, lr_norm = store.batch(*plans[i], stats)
    if i + 1 < len(plans):
        store.prefetch(*plans[i + 1])
    trainer.accumulate_normalised(hr_norm, lr_norm)


class _ValDraws:
    """t and noise of validation batch i, drawn in order from a generator of their own: the same draws every epoch, and the
    training generator is not touched, so a resumed run continues bit for bit."""

    def __init__(self, seed, B, C, T, device, what, rank=0):
        import torch
        self.gen = torch.Generator(device=device)
        self.gen.manual_seed(((int(seed) * 1000003 + int(rank)) * 2 + (1 if what == "noise" else 0)) & (2 ** 63 - 1))   # per rank: each shard its own draws
        self.shape, self.device, self.what, self.next = (B, C, T), device, what, 0

    def __getitem__(self, i):
        import torch
        assert i == self.next, "validation draws are made in batch order"
        self.next += 1
        if self.what == "t":
            return torch.rand(self.shape[0], device=self.device, generator=self.gen)
        return torch.randn(self.shape, device=self.device, generator=self.gen)


def _dist_setup():
    """(rank, world, local_rank); initialises the process group when RANK / WORLD_SIZE are set (torchrun)."""
    if "RANK" not in os.environ or "WORLD_SIZE" not in os.environ:
        return 0, 1, None
    import torch
    import torch.distributed as dist
    rank, world, local = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), int(os.environ.get("LOCAL_RANK", 0))
    torch.cuda.set_device(local)
    if not dist.is_initialized():
        dist.init_process_group(backend="nccl", init_method="env://", world_size=world, rank=rank)
    return rank, world, local


def run(args):
    import torch

    from . import _lib as L
    from . import io as jio
    from .data import LatentStore, epoch_batches, train_batch_plan, val_batch_plan
    from .train import check_loss_arguments, get_lr
    kw = _loss_keywords(args)                         # before any device memory is taken; Trainer checks again
    check_loss_arguments(args.loss, args.latent_loss_weight, kw.get("reconstruction_weight", 1.0), kw.get("charbonnier_eps", 1e-6),
                         tuple(kw.get(k, 0.0) for k in ("freq_loss_weight", "ms_loss_weight", "consistency_weight")))
    accum = int(getattr(args, "grad_accum_steps", 1))
    steps_per_epoch(0, accum)                         # rejects a count below 1
    L.require_gpu()
    rank, world, local = _dist_setup()
    master = rank == 0
    device = torch.device("cuda", local if local is not None else torch.cuda.current_device()) if args.device == "cuda" \
        else torch.device(args.device)
    save_dir, resume_path = resolve_run_dir(args.save_dir_base, args.resume)
    if master:
        os.makedirs(save_dir, exist_ok=True)
        print(f"run folder {save_dir}" + (f", resuming from {resume_path}" if resume_path else ""))
    log_path = os.path.join(save_dir, "train_log.jsonl")

    def log(record):
        if master:
            with open(log_path, "a") as f:
                f.write(json.dumps(record) + "\n")

    cfg = model_config(args)
    C, T, B, mult = cfg["input_channels"], args.frames, args.batch_size, args.samples_per_epoch_multiplier
    budget = None if args.max_resident_gb is None else int(args.max_resident_gb * 2 ** 30)
    train_store = LatentStore(args.data_dir, "train", T, device, budget)
    # an empty or missing val/ folder means no validation (the reference's ValidationDataset accepts it, :544); anything
    # wrong with a validation file is an error
    has_val = bool(glob.glob(os.path.join(args.data_dir, "val", "*.pt")))
    val_store = LatentStore(args.data_dir, "val", T, device, budget) if has_val else None
    stats_path = args.stats_file if os.path.isabs(args.stats_file) else os.path.join(args.data_dir, args.stats_file)
    stats = jio.load_stats(stats_path, channels=C, device=device)
    per_epoch, dropped = steps_per_epoch(len(epoch_batches(len(train_store), mult, B, 0, rank, world, True, args.seed)), accum)
    if per_epoch == 0:
        raise ValueError(f"{len(train_store)} files x {mult} over {world} rank(s) give no batch of {B}" +
                         (f" x {accum} micro-batches" if accum > 1 else ""))
    if dropped and master:
        print(f"{dropped} batch(es) per epoch do not fill an optimiser step of {accum} micro-batches and are dropped")
    total_steps = per_epoch * args.epochs
    model = build_model(args, device)
    trainer = build_trainer(args, model, total_steps, rank=rank, distributed=world > 1)
    start_epoch, best_val = 0, float("inf")
    if resume_path:
        ck = torch.load(resume_path, map_location="cpu", weights_only=False)
        start_epoch = trainer.load_checkpoint(ck) + 1
        best_val = ck.get("best_val_loss", float("inf"))
        # last.pt is written before its epoch's validation (:981-985), so it can be one validation behind: the run folder's
        # best.pt knows the best loss so far, and a worse model must not replace it
        best_path = os.path.join(save_dir, "best.pt")
        if os.path.exists(best_path):
            best_val = min(best_val, torch.load(best_path, map_location="cpu", weights_only=False).get("best_val_loss", float("inf")))
        state = (ck.get("rng_state") or {}).get("trainer_generator")
        if state is not None:
            trainer.gen.set_state(state.cpu())
        if master:
            print(f"resumed at epoch {start_epoch}, step {trainer.global_step}" +
                  (f", moving average after {trainer.ema_updates} updates" if trainer.ema is not None else ""))
    flags = {k: v for k, v in vars(args).items() if isinstance(v, (int, float, str, bool, type(None)))}

    def save(name, epoch):
        if master:
            trainer.save_checkpoint(os.path.join(save_dir, name), epoch=epoch, best_val_loss=best_val,
                                    extra=dict(rng_state=dict(trainer_generator=trainer.gen.get_state()), fit_args=flags,
                                               model_class=args.model))

    if master:
        print(f"{len(train_store)} train files ({train_store.resident_bytes / 2**20:.0f} MiB in HBM, "
              f"{train_store.host_bytes / 2**20:.0f} MiB pinned), {per_epoch} steps per epoch, {args.epochs} epochs, "
              f"{world} rank(s)")
    done = False
    for epoch in range(start_epoch, args.epochs):
        if args.max_steps is not None and trainer.global_step >= args.max_steps:
            break
        batches = epoch_batches(len(train_store), mult, B, epoch, rank, world, True, args.seed)
        plans = [train_batch_plan(train_store.lengths, T, b, args.seed, epoch) for b in batches]
        plans = plans[:per_epoch * accum]       # an optimiser step consumes `accum` consecutive batches of the plan
        t0, epoch_loss = time.time(), 0.0
        for i in range(accum - 1, len(plans), accum):     # i: the step's last micro-batch
            g = trainer.global_step
            if args.max_steps is not None and g >= args.max_steps:
                done = True          # inside an epoch: no last.pt for it; resume restarts from the last finished epoch
                break
            lr_now = get_lr(g, total_steps, args.warmup_steps, args.lr)
            logging = g % args.log_interval == 0
            for j in range(i - accum + 1, i):
                loop_micro(trainer, train_store, plans, j, stats)
            out = loop_step(trainer, train_store, plans, i, stats, lr_now, logging)
            epoch_loss += out["loss"]
            if logging:
                rec = {"step": g, "epoch": epoch, "Train/Loss": out["loss"], "Train/LR": lr_now,
                       "Train/GradNorm": out["grad_norm"], "Train/SNR_dB": out["snr_db"],
                       "Train/PredictionMean": out["pred_mean"], "Train/PredictionStd": out["pred_std"]}
                if args.condition_noise_ratio > 0:
                    rec["Train/CondNoiseStd"] = out["cond_noise_std"]
                if args.latent_loss_weight != 0.0:
                    terms = trainer.loss_terms()
                    rec.update({tag: terms[k] for k, tag in TRAIN_TAGS.items()})
                    if args.loss != "mse":
                        rec[CHARBONNIER_TAG] = rec.pop(TRAIN_TAGS["mse"])
                log(rec)
                if master:
                    print(f"epoch {epoch} step {g}: loss {out['loss']:.5f} lr {lr_now:.2e} grad norm {out['grad_norm']:.3f}")
            # named after the step that has just run, as the reference's (:966-970); the file holds the state AFTER that step
            # (global_step = g + 1).  Resume is by epoch: resuming from an interval file starts at the next epoch and skips
            # the rest of the one it was written in
            if g > 0 and g % args.save_interval_steps == 0:
                save(f"interval_step_{g}.pt", epoch)
        if done:
            break
        if master:
            print(f"epoch {epoch} done in {time.time() - t0:.1f} s, average loss {epoch_loss / per_epoch:.5f}")
        save("last.pt", epoch)
        vbatches = [] if val_store is None else epoch_batches(len(val_store), mult, B, 0, rank, world, False)
        if not vbatches:
            if master:
                print(f"validation skipped: the validation set gives no full batch of {B}")
            log({"epoch": epoch, "Val/Skipped": f"no full batch of {B}"})
        else:
            def val_iter():
                for vb in vbatches:
                    yield val_store.batch(*val_batch_plan(val_store.lengths, T, vb, mult), stats)
            def validate():
                return trainer.validate(val_iter(), normalised=True, t=_ValDraws(args.seed, B, C, T, device, "t", rank),
                                        noise=_ValDraws(args.seed, B, C, T, device, "noise", rank))
            val_loss, val_std, metrics = validate()
            rec = {"epoch": epoch, "Val/Loss": val_loss, "Val/Loss_Std": val_std}
            rec.update({VAL_TAGS[k]: v for k, v in metrics.items() if k in VAL_TAGS})
            if trainer.ema is not None:
                # the same batches, t and noise on the moving average: a paired comparison.  best.pt stays chosen by the raw loss
                with trainer.ema_weights():
                    ema_loss, ema_std, ema_metrics = validate()
                rec.update({"Val/EMA_Loss": ema_loss, "Val/EMA_Loss_Std": ema_std})
                rec.update({EMA_VAL_TAGS[k]: v for k, v in ema_metrics.items() if k in EMA_VAL_TAGS})
            log(rec)
            if master:
                print(f"validation loss {val_loss:.5f} +- {val_std:.5f} (best {best_val:.5f})" +
                      (f", on the moving average {ema_loss:.5f} +- {ema_std:.5f}" if trainer.ema is not None else ""))
            if val_loss < best_val:
                best_val = val_loss
                save("best.pt", epoch)
        if world > 1:
            torch.distributed.barrier()      # wait for rank 0's files (train_ddp_v3mod2.py:1018)
    return dict(save_dir=save_dir, global_step=trainer.global_step, best_val_loss=best_val, trainer=trainer)


def main(argv=None):
    run(build_parser().parse_args(argv))
    return 0


if __name__ == "__main__":
    sys.exit(main())
