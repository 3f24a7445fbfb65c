#!/usr/bin/env python3
"""Fixtures of the DAC 44.1 kHz encoder + quantizer (CPU only): transformers' DacModel(DacConfig(sampling_rate=44100)) in
fp64, its encoder and quantizer filled with the recipe weights (jatsr_amd.recipe.make_dac_encoder_state_dict), encodes
recipe audio (recipe.make_dac_audio).  Writes tests/golden/dac44k_enc_B2_T24.npz and dac44k_enc_B1_T37.npz:
  audio fp32 [B, 1, T*512]; hidden and z fp64 [B, 1024, T]; codes int64 [B, 9, T]; latents fp64 [B, 72, T];
  margin fp64 [B, 9, T] (top-1 minus top-2 score <normalize(e), normalize(c_j)> of each decision); meta (JSON).
No weights ship.
    python tools/gen_dac_encoder_golden.py [--out tests/golden] [--check]   (--check: compare with the committed files)"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CASES = [(2, 24), (1, 37)]
SALT = 0
KEYS = ("audio", "hidden", "z", "codes", "latents", "margin")


def fixture(B, T):
    import torch
    import torch.nn.functional as F
    import transformers
    from transformers.models.dac.modeling_dac import DacConfig, DacModel

    import jatsr_amd.recipe as recipe
    cfg = DacConfig(sampling_rate=44100)
    model = DacModel(cfg).double().eval()
    for m in model.modules():   # fold transformers' weight norm so that the plain recipe weights load
        if hasattr(m, "parametrizations"):
            torch.nn.utils.parametrize.remove_parametrizations(m, "weight")
    sd = recipe.make_dac_encoder_state_dict(salt=SALT)
    full = model.state_dict()
    missing = [k for k in full if not k.startswith("decoder.") and k not in sd]
    assert not missing and all(tuple(full[k].shape) == v.shape for k, v in sd.items()), missing
    model.load_state_dict({k: torch.from_numpy(v).double() for k, v in sd.items()}, strict=False)
    audio_salt = 2000 + 7 * B + T
    audio = recipe.make_dac_audio(B, T * 512, audio_salt)
    with torch.no_grad():
        x = torch.from_numpy(audio).double()
        hidden = model.encoder(x)
        z, codes, latents, _, _ = model.quantizer(hidden)
        margin = []
        for i, q in enumerate(model.quantizer.quantizers):   # the scores of each decision on its own residual
            e = latents[:, 8 * i:8 * i + 8].permute(0, 2, 1)
            sc = F.normalize(e, dim=-1) @ F.normalize(q.codebook.weight, dim=-1).t()
            s = sc.sort(-1).values
            margin.append(s[..., -1] - s[..., -2])
        margin = torch.stack(margin, 1)
    meta = {"B": B, "T": T, "salt": SALT, "audio_salt": audio_salt, "hidden_size": cfg.hidden_size,
            "encoder_hidden_size": cfg.encoder_hidden_size, "downsampling_ratios": list(cfg.downsampling_ratios),
            "n_codebooks": cfg.n_codebooks, "sampling_rate": cfg.sampling_rate, "transformers": transformers.__version__,
            "dtypes": "audio fp32, hidden / z / latents / margin fp64, codes int64"}
    return {"audio": audio, "hidden": hidden.numpy(), "z": z.numpy(), "codes": codes.numpy(), "latents": latents.numpy(),
            "margin": margin.numpy()}, meta


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    for B, T in CASES:
        arrs, meta = fixture(B, T)
        path = os.path.join(a.out, f"dac44k_enc_B{B}_T{T}.npz")
        if a.check:
            g = np.load(path)
            ok = all(np.array_equal(g[k], arrs[k]) for k in KEYS)
            print(f"{path}: {'identical' if ok else 'DIFFERS'}")
            if not ok:
                sys.exit(1)
            continue
        np.savez_compressed(path, meta=json.dumps(meta), **arrs)
        distinct = [len(np.unique(arrs["codes"][:, i])) for i in range(arrs["codes"].shape[1])]
        print(f"{path}: hidden std {arrs['hidden'].std():.3f}, distinct codes per codebook {distinct}, "
              f"median margin {np.median(arrs['margin']):.2e}, min margin {arrs['margin'].min():.2e}")


if __name__ == "__main__":
    main()
