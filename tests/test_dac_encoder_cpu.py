"""CPU tests of the DAC encoder's host side: the fp64 restatement (tests/dac_enc_ref.py) against the transformers fixtures,
the generator, the recipe's non-degeneracy, the weight-file layouts, the WAV reader and the inference CLI flags."""
import os
import struct
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

import dac_enc_ref as R
import jatsr_amd.dac as D
import jatsr_amd.io as jio
import jatsr_amd.recipe as recipe
from helpers import load_golden, rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["dac44k_enc_B2_T24", "dac44k_enc_B1_T37"]


@pytest.fixture(scope="module")
def sd():
    return recipe.make_dac_encoder_state_dict()


@pytest.mark.parametrize("name", NAMES)
def test_ref_matches_golden(name, sd):
    g, meta = load_golden(name)
    B, T = meta["B"], meta["T"]
    np.testing.assert_array_equal(g["audio"], recipe.make_dac_audio(B, T * 512, meta["audio_salt"]))
    h = R.encode_hidden(g["audio"], sd)
    assert h.shape == (B, 1024, T) and rel_l2(h, g["hidden"]) <= 1e-12
    q = R.quantize(g["hidden"], sd)
    np.testing.assert_array_equal(q["codes"], g["codes"])
    assert rel_l2(q["z"], g["z"]) <= 1e-12 and rel_l2(q["latents"], g["latents"]) <= 1e-12
    np.testing.assert_allclose(R.margins(q["scores"]), g["margin"], rtol=0, atol=1e-12)


def test_recipe_is_not_degenerate():
    for name in NAMES:
        g, _ = load_golden(name)
        std = float(g["hidden"].std())
        distinct = [len(np.unique(g["codes"][:, i])) for i in range(g["codes"].shape[1])]
        print(f"{name}: hidden std {std:.3f}, distinct codes {distinct}, median margin {np.median(g['margin']):.3e}, "
              f"min margin {g['margin'].min():.3e}")
        assert 0.1 <= std <= 10
        assert min(distinct) >= 16
        assert np.abs(g["audio"]).max() == pytest.approx(0.5, abs=1e-6)


def test_flops_and_sizes():
    assert abs(recipe.dac_encoder_flops(1, n_quantizers=0) / 1e9 - 0.711) < 1e-3
    assert abs((recipe.dac_encoder_flops(1) - recipe.dac_encoder_flops(1, n_quantizers=0)) / 1e6 - 0.44) < 0.01
    shapes = recipe.dac_encoder_param_shapes()
    n_enc = sum(int(np.prod(s)) for k, s in shapes.items() if k.startswith("encoder."))
    n_q = sum(int(np.prod(s)) for k, s in shapes.items() if k.startswith("quantizer."))
    assert abs(n_enc / 1e6 - 22.3) < 0.05 and abs(n_q / 1e6 - 0.23) < 0.01


def test_pack_kind2_is_the_strided_conv():
    rng = np.random.default_rng(0)
    for s in (2, 4, 8):
        cin, cout, B, T = 3, 5, 2, 6
        w = rng.standard_normal((cout, cin, 2 * s)).astype(np.float32)
        x = rng.standard_normal((B, cin, T * s))
        ref = torch.nn.functional.conv1d(torch.tensor(x), torch.tensor(w, dtype=torch.float64), stride=s,
                                         padding=s // 2).numpy()
        P = D.pack_weight(2, w, cin, cout, s)
        assert P.shape == (cout, 3, s * cin)
        A = np.pad(x.transpose(0, 2, 1).reshape(B, T, s * cin), ((0, 0), (1, 1), (0, 0)))   # super-rows, zero outside
        out = np.einsum("btjk,njk->bnt", np.stack([A[:, j:j + T] for j in range(3)], 2), P)
        np.testing.assert_allclose(out, ref, rtol=0, atol=1e-12)


def _weight_norm_parts(w):
    v = w.double() * 1.7
    g = w.double().reshape(w.shape[0], -1).norm(dim=1).reshape([-1] + [1] * (w.dim() - 1))
    return g.float(), v.float()


def _to_dac_pkg(name):
    """inverse of the dac package encoder key map (module layout of dac.model.dac.Encoder)"""
    if not name.startswith("encoder."):
        return name
    p = name.split(".")
    if p[1] in ("conv1", "snake1", "conv2"):
        return f"encoder.block.{ {'conv1': 0, 'snake1': 5, 'conv2': 6}[p[1]] }." + ".".join(p[2:])
    i, sub = int(p[2]), p[3]
    pre = f"encoder.block.{i + 1}.block."
    if sub == "snake1":
        return pre + "3." + ".".join(p[4:])
    if sub == "conv1":
        return pre + "4." + ".".join(p[4:])
    j = ("snake1", "conv1", "snake2", "conv2").index(p[4])
    return f"{pre}{int(sub[-1]) - 1}.block.{j}." + ".".join(p[5:])


def test_weight_file_layouts_load_the_same(sd, tmp_path):
    plain = {k: torch.from_numpy(v) for k, v in sd.items()}
    hf_plain = dict(plain)
    hf_plain["decoder.conv1.bias"] = torch.zeros(3)                      # ignored
    hf_gv, hf_par, pkg = {}, {}, {}
    for k, v in plain.items():
        if k.endswith(".weight") and not k.endswith("codebook.weight"):
            g, vv = _weight_norm_parts(v)
            b = k[:-len(".weight")]
            hf_gv[b + ".weight_g"], hf_gv[b + ".weight_v"] = g, vv
            hf_par[b + ".parametrizations.weight.original0"] = g
            hf_par[b + ".parametrizations.weight.original1"] = vv
            pb = _to_dac_pkg(k)[:-len(".weight")]
            pkg[pb + ".weight_g"], pkg[pb + ".weight_v"] = g, vv
        else:
            hf_gv[k] = hf_par[k] = v
            pkg[_to_dac_pkg(k)] = v
    pkg["decoder.model.0.bias"] = torch.zeros(4)
    ref = D.encoder_state_dict(hf_plain)
    assert list(ref.keys()) == list(sd.keys())
    for k in sd:
        np.testing.assert_array_equal(ref[k].numpy(), sd[k])
    torch.save(hf_par, tmp_path / "par.pt")
    torch.save({"state_dict": pkg, "metadata": {"kwargs": {"sample_rate": 44100}}}, tmp_path / "weights.pth")
    for got in (D.encoder_state_dict(hf_gv), D.load_encoder_file(tmp_path / "par.pt"),
                D.load_encoder_file(tmp_path / "weights.pth")):
        assert list(got.keys()) == list(sd.keys())
        for k in sd:
            assert rel_l2(got[k].numpy(), sd[k]) <= 1e-6, k
    bad = dict(hf_plain)
    del bad["encoder.block.1.res_unit2.conv1.weight"]
    with pytest.raises(KeyError, match="encoder.block.1.res_unit2.conv1.weight"):
        D.encoder_state_dict(bad)
    bad = dict(hf_plain)
    bad["quantizer.quantizers.3.in_proj.bias"] = torch.ones(9)
    with pytest.raises(ValueError, match="quantizer.quantizers.3.in_proj.bias"):
        D.encoder_state_dict(bad)


def test_encoder_module_uses_transformers_names(sd):
    m = D.DacEncoder()
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()}
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    with pytest.raises(ValueError):
        D.DacEncoder(precision="fp8")


def test_decoder_only_file_still_loads(tmp_path, monkeypatch):
    dsd = recipe.make_dac_state_dict()
    torch.save({"decoder." + k: torch.from_numpy(v) for k, v in dsd.items()}, tmp_path / "dec.pt")
    monkeypatch.setattr(torch.nn.Module, "to", lambda self, *a, **k: self)   # no GPU here: keep the modules on the CPU
    codec = D.load_dac_codec(tmp_path / "dec.pt", device="cpu")
    assert codec.encoder is None
    for k, v in dsd.items():
        np.testing.assert_array_equal(codec.decoder.state_dict()[k].numpy(), v)
    with pytest.raises(D.L.JatError, match="no encoder"):
        codec.encode(torch.zeros(1, 1, 512))
    full = {"decoder." + k: torch.from_numpy(v) for k, v in dsd.items()}
    full.update({k: torch.from_numpy(v) for k, v in recipe.make_dac_encoder_state_dict().items()})
    torch.save(full, tmp_path / "full.pt")
    assert D.load_dac_codec(tmp_path / "full.pt", device="cpu").encoder is not None


def test_wav_reader_roundtrips_float32(tmp_path):
    x = (np.sin(np.arange(1001) * 0.05) * 0.7).astype(np.float32)
    jio.write_wav_float32(tmp_path / "a.wav", torch.from_numpy(x)[None], 44100)
    y, sr = jio.read_wav(tmp_path / "a.wav")
    assert sr == 44100 and y.dtype == np.float32
    np.testing.assert_array_equal(y, x)


def test_wav_reader_pcm16_stereo_and_pcm24(tmp_path):
    rng = np.random.default_rng(1)
    pcm = rng.integers(-32768, 32767, size=(500, 2), dtype=np.int16)
    with wave.open(str(tmp_path / "s.wav"), "wb") as w:
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(22050)
        w.writeframes(pcm.astype("<i2").tobytes())
    y, sr = jio.read_wav(tmp_path / "s.wav")
    assert sr == 22050 and y.shape == (500,)
    np.testing.assert_allclose(y, pcm.astype(np.float64).mean(1) / 32768, rtol=0, atol=1e-7)
    v = rng.integers(-2 ** 23, 2 ** 23, size=300)
    b = (v & 0xFFFFFF).astype(np.uint32)
    with wave.open(str(tmp_path / "p24.wav"), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(3)
        w.setframerate(44100)
        w.writeframes(np.stack([b & 255, (b >> 8) & 255, b >> 16], 1).astype(np.uint8).tobytes())
    y, sr = jio.read_wav(tmp_path / "p24.wav")
    np.testing.assert_allclose(y, v / 2.0 ** 23, rtol=0, atol=1e-7)
    v32 = rng.integers(-2 ** 31, 2 ** 31 - 1, size=200).astype("<i4")
    with wave.open(str(tmp_path / "p32.wav"), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(4)
        w.setframerate(44100)
        w.writeframes(v32.tobytes())
    np.testing.assert_allclose(jio.read_wav(tmp_path / "p32.wav")[0], v32 / 2.0 ** 31, rtol=0, atol=1e-7)


def test_wav_reader_rejects_malformed(tmp_path):
    good = tmp_path / "g.wav"
    jio.write_wav_float32(good, np.zeros(10, np.float32), 44100)
    raw = good.read_bytes()
    cases = {"riff": b"RIFX" + raw[4:], "short": raw[:10], "nofmt": raw[:12] + raw[raw.index(b"data"):],
             "trunc": raw[:-8],
             "align": raw.replace(struct.pack("<HH", 4, 32), struct.pack("<HH", 3, 32), 1),
             "tag": raw.replace(struct.pack("<HH", 3, 1), struct.pack("<HH", 2, 1), 1)}
    for name, data in cases.items():
        p = tmp_path / f"{name}.wav"
        p.write_bytes(data)
        with pytest.raises(ValueError):
            jio.read_wav(p)


def test_cli_flags():
    from jatsr_amd.infer import build_parser, run
    a = build_parser().parse_args(["--input-audio", "x.wav", "--dac-weights", "w.pth"])
    assert a.input_audio == "x.wav" and a.dac_weights == "w.pth"
    assert build_parser().parse_args([]).input_audio is None
    for argv in (["--input-audio", "x.wav"], ["--input-audio", "x.wav", "--dac-weights", "w.pth", "--input-file", "c.pt"]):
        with pytest.raises(SystemExit, match="--input-audio needs --dac-weights"):
            run(build_parser().parse_args(argv + ["--device", "cpu"]))


def test_generator_reproduces_fixtures():
    pytest.importorskip("transformers.models.dac.modeling_dac")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_dac_encoder_golden.py"), "--check"], cwd=ROOT,
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
    assert out.stdout.count("identical") == 2
