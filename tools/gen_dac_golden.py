#!/usr/bin/env python3
"""Fixtures of the DAC 44.1 kHz decoder (CPU only): transformers' DacDecoder(DacConfig(sampling_rate=44100)) in fp64,
filled with the recipe weights (jatsr_amd.recipe.make_dac_state_dict), decodes recipe latents.  Writes
tests/golden/dac44k_B2_T24.npz and dac44k_B1_T37.npz: input z (fp32), fp64 audio and metadata.  No weights ship.
    python tools/gen_dac_golden.py [--out tests/golden] [--check]   (--check: compare with the committed files)"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CASES = [(2, 24), (1, 37)]
SALT = 0


def fixture(B, T):
    import torch
    import transformers
    from transformers.models.dac.modeling_dac import DacConfig, DacDecoder

    import jatsr_amd.recipe as recipe
    cfg = DacConfig(sampling_rate=44100)
    dec = DacDecoder(cfg).double().eval()
    sd = recipe.make_dac_state_dict(salt=SALT)
    missing, unexpected = dec.load_state_dict({k: torch.from_numpy(v).double() for k, v in sd.items()}, strict=True)
    z = recipe.gaussian("dac_z", (B, cfg.hidden_size, T), 1000 + 7 * B + T)
    with torch.no_grad():
        audio = dec(torch.from_numpy(z).double()).numpy()
    meta = {"B": B, "T": T, "salt": SALT, "z_salt": 1000 + 7 * B + T, "hidden_size": cfg.hidden_size,
            "decoder_hidden_size": cfg.decoder_hidden_size, "upsampling_ratios": list(cfg.upsampling_ratios),
            "sampling_rate": cfg.sampling_rate, "transformers": transformers.__version__}
    return z, audio, meta


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    for B, T in CASES:
        z, audio, meta = fixture(B, T)
        path = os.path.join(a.out, f"dac44k_B{B}_T{T}.npz")
        if a.check:
            g = np.load(path)
            ok = np.array_equal(g["z"], z) and np.array_equal(g["audio"], audio)
            print(f"{path}: {'identical' if ok else 'DIFFERS'}")
            if not ok:
                sys.exit(1)
            continue
        np.savez_compressed(path, z=z, audio=audio, meta=json.dumps(meta))
        print(f"{path}: z {z.shape} audio {audio.shape} std {audio.std():.4f} |y|>0.99 {np.mean(np.abs(audio) > 0.99):.4f}")


if __name__ == "__main__":
    main()
