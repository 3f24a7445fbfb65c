"""DAC 44.1 kHz decoder on the GPU (csrc/dac.hip, jatsr_amd.dac): the transformers fp64 fixtures at full size, each
kernel against the fp64 restatement (tests/dac_ref.py), a 4096-frame decode, batch independence, determinism, argument
errors, the inference CLI's WAV output and the fp16-operand library."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import dac_ref  # noqa: E402
import jatsr_amd.dac as D  # noqa: E402
import jatsr_amd.io as jio  # noqa: E402
import jatsr_amd.recipe as recipe  # noqa: E402
from jatsr_amd import _lib as L  # noqa: E402
from helpers import load_golden, rel_l2  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# gates (rel-L2, max-abs) against the fp64 fixtures.  Measured on MI355X: bf16x3 4.5e-5 / 1.0e-4 (gates 2.2x / 3x above);
# bf16 2.3e-2, which is what a CPU emulation of the same rounding points gives with these recipe weights (2.28e-2; their
# alphas up to 3 and non-zero biases make the network more sensitive than transformers' init, 1.16e-2): gate 1.5x above
GATES = {"bf16x3": (1e-4, 3e-4), "bf16": (3.5e-2, None)}


@pytest.fixture(scope="module")
def sd():
    return recipe.make_dac_state_dict()


@pytest.fixture(scope="module")
def decoder(sd):
    m = D.DacDecoder()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.cuda()


@pytest.mark.parametrize("name", ["dac44k_B2_T24", "dac44k_B1_T37"])
@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
def test_golden(decoder, name, precision):
    g, meta = load_golden(name)
    y = decoder(torch.from_numpy(g["z"]).cuda(), precision=precision).cpu().numpy()
    assert y.shape == g["audio"].shape and np.isfinite(y).all()
    r, mx = rel_l2(y, g["audio"]), float(np.abs(y - g["audio"]).max())
    print(f"{name} {precision}: rel-L2 {r:.3e} max-abs {mx:.3e}")
    gate_r, gate_mx = GATES[precision]
    assert r <= gate_r
    if gate_mx is not None:
        assert mx <= gate_mx


def _rand(name, shape, salt, scale=1.0):
    return recipe.uniform(name, shape, salt) * np.float32(scale)


def _cl(x):   # [B, C, T] -> channels-last [B*T, C]
    return np.ascontiguousarray(np.transpose(x, (0, 2, 1)).reshape(-1, x.shape[1]))


def _check_rows(got, ref, B, T, tol):
    """per sample, and the 10 rows at each sample boundary on their own (a leak between samples shows there first)"""
    got, ref = got.reshape(B, T, -1), ref.reshape(B, T, -1)
    for b in range(B):
        assert rel_l2(got[b], ref[b]) <= tol, b
        assert rel_l2(got[b, :10], ref[b, :10]) <= tol and rel_l2(got[b, -10:], ref[b, -10:]) <= tol, b


@pytest.mark.parametrize("C", [96, 768])
@pytest.mark.parametrize("dil", [1, 3, 9])
def test_conv_k7_snake_epilogue(C, dil):
    B, T = 2, 37
    x = _rand("k7x", (B, C, T), C + dil)
    x[1] *= 50.0                                   # sample 1 large: any leak into sample 0 would stand out
    w = _rand("k7w", (C, C, 7), dil, 1.0 / np.sqrt(7 * C))
    b = _rand("k7b", (C,), dil, 0.1)
    alpha = 1.75 + _rand("k7a", (C,), dil, 1.25)
    ref = F.conv1d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), torch.from_numpy(b).double(),
                   padding=3 * dil, dilation=dil)
    ref_s = dac_ref.snake(ref, torch.from_numpy(alpha).double())
    ref, ref_s = _cl(ref.numpy()), _cl(ref_s.numpy())
    wp = D.pack_weight(0, w, C, C, 7)
    for prec, tol in (("bf16x3", 2e-5), ("bf16", 2e-2)):
        o32, planes = D.conv(torch.from_numpy(_cl(x)).cuda(), wp, torch.from_numpy(b).cuda(), B, T, C, C, C, 7, dil,
                             alpha=torch.from_numpy(alpha).cuda(), precision=prec)
        _check_rows(o32.cpu().numpy(), ref, B, T, tol)
        s = D.planes_to_float(planes[0], planes[1] if prec == "bf16x3" else None).cpu().numpy()
        _check_rows(s, ref_s, B, T, tol)


@pytest.mark.parametrize("s", [2, 4, 8])
def test_conv_transpose_polyphase(s):
    B, T, cin, cout = 2, 37, 192, 96
    x = _rand("ctx", (B, cin, T), s)
    x[1] *= 50.0
    w = _rand("ctw", (cin, cout, 2 * s), s, 1.0 / np.sqrt(2 * cin))
    b = _rand("ctb", (cout,), s, 0.1)
    alpha = 1.75 + _rand("cta", (cout,), s, 1.25)
    ref = F.conv_transpose1d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), torch.from_numpy(b).double(),
                             stride=s, padding=s // 2)
    assert ref.shape[-1] == T * s
    ref_s = _cl(dac_ref.snake(ref, torch.from_numpy(alpha).double()).numpy())
    ref = _cl(ref.numpy())
    wp = D.pack_weight(1, w, cin, cout, s)
    o32, planes = D.conv(torch.from_numpy(_cl(x)).cuda(), wp, torch.from_numpy(b).cuda(), B, T, cin, s * cout, cout, 3, 1,
                         alpha=torch.from_numpy(alpha).cuda())
    _check_rows(o32.cpu().numpy().reshape(-1, cout), ref, B, T * s, 2e-5)
    _check_rows(D.planes_to_float(*planes).cpu().numpy().reshape(-1, cout), ref_s, B, T * s, 2e-5)


@pytest.mark.parametrize("C", [96, 384])
def test_conv1x1_residual(C):
    B, T = 2, 41
    x = _rand("rx", (B, C, T), C)
    res = _rand("rr", (B, C, T), C, 3.0)
    w = _rand("rw", (C, C, 1), C, 1.0 / np.sqrt(C))
    b = _rand("rb", (C,), C, 0.1)
    ref = _cl(res + F.conv1d(torch.from_numpy(x).double(), torch.from_numpy(w).double(),
                             torch.from_numpy(b).double()).numpy())
    r = torch.from_numpy(_cl(res)).cuda()
    o32, _ = D.conv(torch.from_numpy(_cl(x)).cuda(), D.pack_weight(0, w, C, C, 1), torch.from_numpy(b).cuda(), B, T, C,
                    C, C, 1, 1, res=r)
    _check_rows(o32.cpu().numpy(), ref, B, T, 2e-6)


def test_long_input_windows(decoder, sd):
    T, margin = 4096, 16
    z = recipe.gaussian("dac_long", (1, 1024, T), 3)
    y = decoder(torch.from_numpy(z).cuda()).cpu().numpy()
    assert y.shape == (1, 1, T * 512) and np.isfinite(y).all()
    for a, b in ((0, 32), (2000, 2032), (T - 32, T)):
        wa, wb = max(0, a - margin), min(T, b + margin)
        ref = dac_ref.decode(z[:, :, wa:wb], sd)
        got = y[:, :, a * 512:b * 512]
        ref = ref[:, :, (a - wa) * 512:(b - wa) * 512]
        r = rel_l2(got, ref)
        print(f"frames [{a}, {b}): rel-L2 {r:.3e}")
        assert r <= 1e-4


def test_batch_independence_and_determinism(decoder):
    z = torch.from_numpy(recipe.gaussian("dac_batch", (3, 1024, 29), 4)).cuda()
    for prec in ("bf16x3", "bf16"):
        y3 = decoder(z, precision=prec)
        for b in range(3):
            assert torch.equal(decoder(z[b:b + 1], precision=prec)[0], y3[b]), (prec, b)
        assert torch.equal(decoder(z, precision=prec), y3), prec


def test_errors(sd):
    m = D.DacDecoder(max_B=2, max_T=32)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.cuda()
    ok = torch.zeros(2, 1024, 32, device="cuda")
    assert m(ok).shape == (2, 1, 32 * 512)
    for bad in (torch.zeros(1, 1024, 0, device="cuda"), torch.zeros(1, 1024, 33, device="cuda"),
                torch.zeros(3, 1024, 8, device="cuda"), torch.zeros(1, 1000, 8, device="cuda")):
        with pytest.raises(L.JatError):
            m(bad)
    # the C ABI rejects the same calls itself
    h = m._handle
    audio = torch.empty(4, 1, 40 * 512, device="cuda")
    for B, T, prec in ((1, 0, 0), (1, 33, 0), (3, 8, 0), (1, 8, 2)):
        with pytest.raises(L.JatError):
            D._check(L.lib().jat_dac_decode(h.ptr, L.ptr(ok), L.ptr(audio), B, T, prec, L.stream_ptr()))
    named = {k: torch.from_numpy(v) for k, v in sd.items()}
    del named["block.3.res_unit2.snake2.alpha"]
    with pytest.raises(L.JatError, match="block.3.res_unit2.snake2.alpha"):
        D._Handle(named, m.dims, 1, 8, torch.device("cuda"))
    with pytest.raises(L.JatError):
        D._check(L.lib().jat_k_dac_conv(None, None, None, None, None, None, None, None, None, None, 1, 8, 100, 96, 96, 7, 1,
                                        0, L.stream_ptr()))     # cin not a multiple of 32
    torch.cuda.synchronize()


def test_infer_cli_writes_wavs(tmp_path, sd, monkeypatch):
    from jatsr_amd.infer import main as infer_main
    cfg = recipe.CONFIGS["micro"]
    C, T = cfg["input_channels"], 200                      # one chunk (a file shorter than the 172-frame overlap has none)
    if C != 1024:
        cfg = dict(cfg, input_channels=1024, cond_channels=1024)
        C = 1024
    jsd = recipe.make_state_dict(cfg)
    torch.save({"model_state_dict": {k: torch.from_numpy(v) for k, v in jsd.items()}, "config": dict(cfg)},
               tmp_path / "last.pt")
    jio.save_latent_file(tmp_path / "clip.pt", hr_latent=torch.from_numpy(recipe.gaussian("dac_hr", (C, T), 1)),
                         lr_latent=torch.from_numpy(recipe.gaussian("dac_lr", (C, T), 2)))
    ones, zeros = [1.0] * C, [0.0] * C
    import json
    (tmp_path / "stats.json").write_text(json.dumps({"hr_mean": zeros, "hr_std": ones, "lr_mean": zeros, "lr_std": ones}))
    torch.save({"decoder." + k: torch.from_numpy(v) for k, v in sd.items()}, tmp_path / "dac.pt")
    base = ["--checkpoint", str(tmp_path / "last.pt"), "--input-file", str(tmp_path / "clip.pt"), "--stats-file",
            str(tmp_path / "stats.json"), "--steps", "2", "--cfg-scale", "2.0", "--seed", "3"]

    infer_main(base + ["--output-dir", str(tmp_path / "plain")])
    assert not [f for f in os.listdir(tmp_path / "plain") if f.endswith(".wav")]

    seen = []
    orig = D.DacCodec.decode
    monkeypatch.setattr(D.DacCodec, "decode", lambda self, z: seen.append(z.clone()) or orig(self, z))
    infer_main(base + ["--output-dir", str(tmp_path / "out"), "--dac-weights", str(tmp_path / "dac.pt")])
    names = sorted(f for f in os.listdir(tmp_path / "out") if f.endswith(".wav"))
    assert names == ["clip_generated_cfg2.0.wav", "clip_hr_gt.wav", "clip_lr_input.wav"]
    assert len(seen) == 3 and seen[0].dtype == torch.float32 and seen[0].shape == (1, C, T)
    codec = D.load_dac_codec(tmp_path / "dac.pt")
    for name, z in zip(["clip_generated_cfg2.0.wav", "clip_hr_gt.wav", "clip_lr_input.wav"], seen):
        raw = (tmp_path / "out" / name).read_bytes()
        assert int.from_bytes(raw[24:28], "little") == 44100
        data = np.frombuffer(raw[raw.index(b"data") + 8:], "<f4")
        assert data.size == T * 512
        np.testing.assert_array_equal(data, codec.decode(z)[0, 0].cpu().numpy())


_FP16_CHILD = """
import sys, numpy as np, torch
sys.path.insert(0, 'tests')
import jatsr_amd.dac as D, jatsr_amd.recipe as recipe
from jatsr_amd import _lib as L
from helpers import load_golden
assert L.operand_dtype() == 'fp16'
g, _ = load_golden('dac44k_B2_T24')
m = D.DacDecoder(); m.load_state_dict({k: torch.from_numpy(v) for k, v in recipe.make_dac_state_dict().items()})
np.save(sys.argv[1], m.cuda()(torch.from_numpy(g['z']).cuda()).cpu().numpy())
"""


def test_fp16_library_same_bits(decoder, tmp_path):
    out = tmp_path / "fp16.npy"
    env = dict(os.environ, JAT_OPERAND_DTYPE="fp16")
    env.pop("JAT_LIB_PATH", None)
    r = subprocess.run([sys.executable, "-c", _FP16_CHILD, str(out)], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    y16 = np.load(out)
    g, _ = load_golden("dac44k_B2_T24")
    assert rel_l2(y16, g["audio"]) <= GATES["bf16x3"][0]
    y = decoder(torch.from_numpy(g["z"]).cuda()).cpu().numpy()
    np.testing.assert_array_equal(y16, y)
