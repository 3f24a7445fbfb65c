"""CPU tests of the DAC decoder's host side: the fp64 restatement (tests/dac_ref.py) against the fixtures, the weight-file
formats and weight-norm folding of jatsr_amd.dac, the float WAV writer, and the recipe weights."""
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

import dac_ref
import jatsr_amd.dac as D
import jatsr_amd.io as jio
import jatsr_amd.recipe as recipe
from helpers import load_golden, rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sd():
    return recipe.make_dac_state_dict()


@pytest.mark.parametrize("name", ["dac44k_B2_T24", "dac44k_B1_T37"])
def test_dac_ref_matches_golden(name, sd):
    g, meta = load_golden(name)
    assert g["z"].shape == (meta["B"], 1024, meta["T"])
    np.testing.assert_array_equal(g["z"], recipe.gaussian("dac_z", g["z"].shape, meta["z_salt"]))
    y = dac_ref.decode(g["z"], sd)
    assert y.shape == (meta["B"], 1, meta["T"] * 512)
    assert rel_l2(y, g["audio"]) <= 1e-9


def test_recipe_weights_do_not_saturate(sd):
    g, _ = load_golden("dac44k_B2_T24")
    assert np.mean(np.abs(g["audio"]) > 0.99) < 0.01 and g["audio"].std() > 0.05
    a = [v for k, v in sd.items() if k.endswith(".alpha")]
    lo, hi = min(float(x.min()) for x in a), max(float(x.max()) for x in a)
    assert 0.5 <= lo < 0.6 and 2.9 < hi <= 3.0


def _weight_norm_parts(w):
    v = w.double() * 1.7
    g = w.double().reshape(w.shape[0], -1).norm(dim=1).reshape([-1] + [1] * (w.dim() - 1))
    return g.float(), v.float()


def _to_dac_pkg(name):
    """inverse of the dac package key map (module layout of dac.model.dac.Decoder)"""
    if name.startswith("conv1."):
        return "decoder.model.0." + name[6:]
    if name.startswith("snake1."):
        return "decoder.model.5." + name[7:]
    if name.startswith("conv2."):
        return "decoder.model.6." + name[6:]
    parts = name.split(".")
    i, sub = int(parts[1]), parts[2]
    pre = f"decoder.model.{i + 1}.block."
    if sub == "snake1":
        return pre + "0." + ".".join(parts[3:])
    if sub == "conv_t1":
        return pre + "1." + ".".join(parts[3:])
    u = int(sub[-1])
    j = ("snake1", "conv1", "snake2", "conv2").index(parts[3])
    return f"{pre}{u + 1}.block.{j}." + ".".join(parts[4:])


def _write_safetensors(path, tensors):
    header, blobs, off = {}, [], 0
    for k, v in tensors.items():
        b = v.contiguous().numpy().astype("<f4").tobytes()
        header[k] = {"dtype": "F32", "shape": list(v.shape), "data_offsets": [off, off + len(b)]}
        blobs.append(b)
        off += len(b)
    h = json.dumps(header).encode()
    with open(path, "wb") as f:
        f.write(len(h).to_bytes(8, "little") + h + b"".join(blobs))


def test_weight_file_layouts_load_the_same(sd, tmp_path):
    plain = {k: torch.from_numpy(v) for k, v in sd.items()}
    hf_plain = {"decoder." + k: v for k, v in plain.items()}
    hf_plain["encoder.block.0.conv1.weight"] = torch.zeros(3)          # ignored
    hf_gv, hf_par, pkg = {}, {}, {}
    for k, v in plain.items():
        if k.endswith(".weight"):
            g, vv = _weight_norm_parts(v)
            b = k[:-len(".weight")]
            hf_gv["decoder." + b + ".weight_g"], hf_gv["decoder." + b + ".weight_v"] = g, vv
            hf_par["decoder." + b + ".parametrizations.weight.original0"] = g
            hf_par["decoder." + b + ".parametrizations.weight.original1"] = vv
            pb = _to_dac_pkg(k)[:-len(".weight")]
            pkg[pb + ".weight_g"], pkg[pb + ".weight_v"] = g, vv
        else:
            hf_gv["decoder." + k] = hf_par["decoder." + k] = v
            pkg[_to_dac_pkg(k)] = v
    pkg["quantizer.quantizers.0.codebook.weight"] = torch.zeros(4, 8)
    torch.save(hf_plain, tmp_path / "plain.bin")
    _write_safetensors(tmp_path / "gv.safetensors", hf_gv)
    torch.save(hf_par, tmp_path / "par.pt")
    torch.save({"state_dict": pkg, "metadata": {"kwargs": {"sample_rate": 44100}}}, tmp_path / "weights.pth")
    ref = D.load_decoder_file(tmp_path / "plain.bin")
    assert list(ref.keys()) == list(sd.keys())
    for k in sd:
        np.testing.assert_array_equal(ref[k].numpy(), sd[k])
    for f in ("gv.safetensors", "par.pt", "weights.pth"):
        got = D.load_decoder_file(tmp_path / f)
        for k in sd:
            assert rel_l2(got[k].numpy(), sd[k]) <= 1e-6, (f, k)

    bad = dict(hf_plain)
    del bad["decoder.block.2.res_unit3.conv1.weight"]
    with pytest.raises(KeyError, match="block.2.res_unit3.conv1.weight"):
        D.decoder_state_dict(bad)
    bad = dict(hf_plain)
    bad["decoder.block.1.snake1.alpha"] = torch.ones(1, 767, 1)
    with pytest.raises(ValueError, match="block.1.snake1.alpha"):
        D.decoder_state_dict(bad)


def test_decoder_module_uses_transformers_names(sd):
    m = D.DacDecoder()
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert got == {k: tuple(v.shape) for k, v in sd.items()}
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    with pytest.raises(ValueError):
        D.DacDecoder(precision="fp8")


def test_wav_float32_roundtrip(tmp_path):
    x = np.sin(np.arange(1000) * 0.05).astype(np.float32) * 0.7
    x[3] = -1.0
    p = tmp_path / "a.wav"
    jio.write_wav_float32(p, torch.from_numpy(x)[None], 44100)
    raw = p.read_bytes()
    assert raw[:4] == b"RIFF" and raw[8:12] == b"WAVE" and struct.unpack("<I", raw[4:8])[0] == len(raw) - 8
    pos, chunks = 12, {}
    while pos < len(raw):
        cid, n = struct.unpack("<4sI", raw[pos:pos + 8])
        chunks[cid] = raw[pos + 8:pos + 8 + n]
        pos += 8 + n
    tag, ch, sr, bps, align, bits = struct.unpack("<HHIIHH", chunks[b"fmt "][:16])
    assert (tag, ch, sr, bps, align, bits) == (3, 1, 44100, 44100 * 4, 4, 32)
    np.testing.assert_array_equal(np.frombuffer(chunks[b"data"], "<f4"), x)


def test_cli_flags():
    from jatsr_amd.infer import build_parser
    a = build_parser().parse_args(["--dac-weights", "w.pth", "--dac-precision", "bf16"])
    assert a.dac_weights == "w.pth" and a.dac_precision == "bf16"
    d = build_parser().parse_args([])
    assert d.dac_weights is None and d.dac_precision == "bf16x3"


def test_package_does_not_import_transformers():
    code = "import sys, jatsr_amd.dac, jatsr_amd.infer; print('transformers' in sys.modules)"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.strip() == "False"


def test_generator_reproduces_fixtures():
    pytest.importorskip("transformers.models.dac.modeling_dac")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_dac_golden.py"), "--check"], cwd=ROOT,
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
