"""DAC 44.1 kHz encoder + residual vector quantizer on the GPU (csrc/dac_enc.hip, csrc/dac.hip, jatsr_amd.dac.DacEncoder):
the transformers fp64 fixtures in both precisions under the code-flip rule, each kernel against fp64 (tests/dac_enc_ref.py),
a 4096-frame encode, batch independence, determinism, argument errors, the inference CLI from a WAV and the fp16-operand
library.

Code-flip rule: the GPU's codes are compared with the fp64 argmax of a reference that follows the GPU's own codes
(teacher forcing), so one flip does not cascade.  A code may differ from that argmax only where its fp64 score is within
2 * |normalize(e_gpu) - normalize(e_ref)| + 1e-6 of the best (|c_j| = 1 bounds the score error the latent error causes),
and on at most FLIP_FRACTION of the decisions."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import dac_enc_ref as R  # noqa: E402
import dac_ref  # noqa: E402
import jatsr_amd.dac as D  # noqa: E402
import jatsr_amd.io as jio  # noqa: E402
import jatsr_amd.recipe as recipe  # noqa: E402
from jatsr_amd import _lib as L  # noqa: E402
from helpers import load_golden, rel_l2  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# rel-L2 gates on (hidden, latents, z) against fp64, z against the teacher-forced reference (it depends on the codes and the
# fp32 out_proj only).  Measured on MI355X, bf16x3: hidden 3.9e-5, latents 2.6e-5, z 8.0e-8 (gates 2.5x / 4x / 12x above).
# bf16 (one pass): hidden 2.1e-2, latents 1.4e-2 (gates 2.3x / 3.6x above).  Flips: bf16x3 none on the fixtures (cap 2 %); bf16 5.6 % on B2_T24, as expected from a
# latent error near 1e-2 against the recipe's median margin 2.3e-2 (cap 10 %).
GATES = {"bf16x3": (1e-4, 1e-4, 1e-6), "bf16": (5e-2, 5e-2, 1e-6)}
FLIP_FRACTION = {"bf16x3": 0.02, "bf16": 0.10}


@pytest.fixture(scope="module")
def sd():
    return recipe.make_dac_encoder_state_dict()


@pytest.fixture(scope="module")
def sd_t(sd):
    return {k: torch.from_numpy(v) for k, v in sd.items()}


@pytest.fixture(scope="module")
def encoder(sd_t):
    m = D.DacEncoder()
    m.load_state_dict(sd_t)
    return m.cuda()


def _unit(e):   # normalize over the codebook dim (axis 2 of [B, n_q, 8, T])
    return e / np.maximum(np.linalg.norm(e, axis=2, keepdims=True), 1e-12)


def _flip_check(hidden, sd, codes, latents, n_q, label, cap=FLIP_FRACTION["bf16x3"]):
    """teacher-forced fp64 quantizer on `hidden` following the GPU codes; checks the flip rule, returns the reference"""
    B, T = codes.shape[0], codes.shape[2]
    ref = R.quantize(hidden, sd, n_q, forced_codes=codes)
    sc = ref["scores"]                                                      # [B, n_q, T, K]
    best = sc.max(-1)
    own = np.take_along_axis(sc, codes[..., None].astype(np.int64), -1)[..., 0]
    flip = codes != sc.argmax(-1)
    err = np.linalg.norm(_unit(latents.reshape(B, n_q, 8, T).astype(np.float64))
                         - _unit(ref["latents"].reshape(B, n_q, 8, T)), axis=2)
    bound = 2 * err + 1e-6
    print(f"{label}: {int(flip.sum())} flips of {flip.size} decisions, worst score gap of a flip "
          f"{float((best - own)[flip].max()) if flip.any() else 0.0:.2e}")
    assert np.all((best - own)[flip] <= bound[flip]), label
    assert flip.mean() <= cap, label
    return ref


@pytest.mark.parametrize("name", ["dac44k_enc_B2_T24", "dac44k_enc_B1_T37"])
@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
def test_golden(encoder, sd, name, precision):
    g, meta = load_golden(name)
    z, codes, lat, hid = encoder(torch.from_numpy(g["audio"]).cuda(), precision=precision, return_hidden=True)
    z, codes, lat, hid = (t.cpu().numpy() for t in (z, codes, lat, hid))
    assert z.shape == g["z"].shape and codes.shape == g["codes"].shape and lat.shape == g["latents"].shape
    assert np.isfinite(z).all() and np.isfinite(hid).all()
    r_h = rel_l2(hid, g["hidden"])
    ref = _flip_check(g["hidden"], sd, codes, lat, 9, f"{name} {precision}", FLIP_FRACTION[precision])
    r_z, r_l = rel_l2(z, ref["z"]), rel_l2(lat, ref["latents"])
    print(f"{name} {precision}: hidden rel-L2 {r_h:.3e}, z {r_z:.3e}, latents {r_l:.3e}, codes equal to the fixture "
          f"{float(np.mean(codes == g['codes'])):.4f}")
    assert r_h <= GATES[precision][0] and r_l <= GATES[precision][1] and r_z <= GATES[precision][2]


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


def test_head_conv():
    B, n, C = 2, 1003, 64
    x = _rand("hx", (B, 1, n), 1, 0.5)
    x[1] *= 50.0                                    # sample 1 large: a leak into sample 0 would stand out
    w = _rand("hw", (C, 1, 7), 1, 0.5)
    b = _rand("hb", (C,), 1, 0.1)
    alpha = 1.75 + _rand("ha", (C,), 1, 1.25)
    ref = F.conv1d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), torch.from_numpy(b).double(), padding=3)
    ref_s = _cl(dac_ref.snake(ref, torch.from_numpy(alpha).double()).numpy())
    ref = _cl(ref.numpy())
    # fp32 sums of 7 products, measured 2.4e-6 on the small sample 0
    for prec, tol in (("bf16x3", 1e-5), ("bf16", 5e-3)):
        o32, planes = D.head(torch.from_numpy(x[:, 0]).cuda(), torch.from_numpy(w).cuda(), torch.from_numpy(b).cuda(),
                             torch.from_numpy(alpha).cuda(), precision=prec)
        _check_rows(o32.cpu().numpy(), ref, B, n, 1e-5)
        _check_rows(D.planes_to_float(*planes).cpu().numpy(), ref_s, B, n, tol)


@pytest.mark.parametrize("s,cin", [(2, 64), (4, 128), (8, 256), (8, 512)])
def test_strided_conv_superrows(s, cin):
    B, T, cout = 2, 19, 2 * cin
    x = _rand("sx", (B, cin, T * s), s + cin)
    x[1] *= 50.0
    w = _rand("sw", (cout, cin, 2 * s), s, 1.0 / np.sqrt(2 * s * cin))
    b = _rand("sb", (cout,), s, 0.1)
    alpha = 1.75 + _rand("sa", (cout,), s, 1.25)
    ref = F.conv1d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), torch.from_numpy(b).double(), stride=s,
                   padding=s // 2)
    assert ref.shape[-1] == T
    ref_s = _cl(dac_ref.snake(ref, torch.from_numpy(alpha).double()).numpy())
    ref = _cl(ref.numpy())
    wp = D.pack_weight(2, w, cin, cout, s)
    assert wp.shape == (cout, 3, s * cin)
    a = torch.from_numpy(_cl(x)).cuda()          # [B*T*s, cin] read by the kernel as [B*T, s*cin]
    for prec, tol in (("bf16x3", 2e-5), ("bf16", 2e-2)):
        o32, planes = D.conv(a, wp, torch.from_numpy(b).cuda(), B, T, s * cin, cout, cout, 3, 1,
                             alpha=torch.from_numpy(alpha).cuda(), precision=prec)
        _check_rows(o32.cpu().numpy(), ref, B, T, tol)
        _check_rows(D.planes_to_float(planes[0], planes[1] if prec == "bf16x3" else None).cpu().numpy(), ref_s, B, T, tol)


def _fp32_exact(x):   # round to fp32 so that kernel and fp64 reference see the same input
    return np.asarray(x, np.float32).astype(np.float64)


def test_rvq_kernel(sd, sd_t):
    B, T = 3, 45
    h = recipe.gaussian("rvq_h", (B, 1024, T), 5) * np.float32(1.5)
    h[2] *= 20.0
    hid_cl = torch.from_numpy(_cl(h)).cuda()
    dev = {k: v.cuda() for k, v in sd_t.items() if k.startswith("quantizer.")}
    z, codes, lat, hcm = (t.cpu().numpy() for t in D.rvq(hid_cl, dev, B, T, 9))
    np.testing.assert_array_equal(hcm, h)
    ref = _flip_check(_fp32_exact(h), sd, codes, lat, 9, "rvq kernel")
    _check_rows(_cl(z), _cl(ref["z"]), B, T, 1e-6)
    _check_rows(_cl(lat), _cl(ref["latents"]), B, T, 1e-6)
    for nq in (1, 4):
        z1, c1, l1, _ = (t.cpu().numpy() for t in D.rvq(hid_cl, dev, B, T, nq))
        np.testing.assert_array_equal(c1, codes[:, :nq])
        np.testing.assert_array_equal(l1, lat[:, :8 * nq])
        r1 = R.quantize(_fp32_exact(h), sd, nq, forced_codes=c1)
        assert rel_l2(z1, r1["z"]) <= 1e-6, nq


@pytest.mark.parametrize("nq", [1, 4, 9])
def test_n_quantizers(encoder, nq):
    g, _ = load_golden("dac44k_enc_B2_T24")
    a = torch.from_numpy(g["audio"]).cuda()
    z9, c9, l9 = encoder(a)
    z, c, lat, hid = encoder(a, n_quantizers=nq, return_hidden=True)
    assert c.shape == (2, nq, 24) and lat.shape == (2, 8 * nq, 24)
    assert torch.equal(c, c9[:, :nq]) and torch.equal(lat, l9[:, :8 * nq])
    # z of the first nq codebooks, summed in the kernel's order, from the 9-codebook run's own codes
    zz = torch.zeros_like(z9)
    sd = encoder.state_dict()
    for i in range(nq):
        p = f"quantizer.quantizers.{i}."
        rows = sd[p + "codebook.weight"][c9[:, i]]                           # [B, T, 8]
        q = torch.einsum("ck,btk->bct", sd[p + "out_proj.weight"][:, :, 0].double(), rows.double())
        zz += (q + sd[p + "out_proj.bias"].double()[None, :, None]).float()
    assert rel_l2(z.cpu().numpy(), zz.cpu().numpy()) <= 1e-6
    if nq == 9:
        assert torch.equal(z, z9)


def _receptive_field(strides=(2, 4, 8, 8)):
    """samples either side of a frame's own 512 samples that can reach it: conv1 (3), per block the three dilated k7
    convs (3 * (1 + 3 + 9) rows) and the strided conv (s / 2 rows before, 3 s / 2 - 1 after, s rows = 1 output row),
    conv2 (1 frame)."""
    reach, rate = 3, 1
    for s in strides:
        reach += 39 * rate + (3 * s // 2) * rate
        rate *= s
    return reach + rate


def test_long_input_windows(encoder, sd):
    T = 4096
    audio = recipe.make_dac_audio(1, T * 512, 77)
    z, codes, lat, hid = encoder(torch.from_numpy(audio).cuda(), return_hidden=True)
    assert z.shape == (1, 1024, T) and torch.isfinite(z).all()
    z, codes, hid = z.cpu().numpy(), codes.cpu().numpy(), hid.cpu().numpy()
    margin = -(-_receptive_field() // 512) + 1
    for a, b in ((0, 32), (2000, 2032), (T - 32, T)):
        wa, wb = max(0, a - margin), min(T, b + margin)
        zw, cw, _, hw = encoder(torch.from_numpy(audio[:, :, wa * 512:wb * 512]).cuda(), return_hidden=True)
        zw, cw, hw = (t.cpu().numpy()[:, :, a - wa:b - wa] for t in (zw, cw, hw))
        same = np.array_equal(zw, z[:, :, a:b]) and np.array_equal(hw, hid[:, :, a:b])
        print(f"frames [{a}, {b}) with {margin} frames of context: window re-encode bit-identical: {same}")
        np.testing.assert_array_equal(cw, codes[:, :, a:b])
        assert rel_l2(zw, z[:, :, a:b]) <= 1e-6 and rel_l2(hw, hid[:, :, a:b]) <= 1e-6
        ref = R.encode_hidden(audio[:, :, wa * 512:wb * 512], sd)[:, :, a - wa:b - wa]
        r = rel_l2(hid[:, :, a:b], ref)
        print(f"frames [{a}, {b}): hidden rel-L2 {r:.3e} vs fp64")
        assert r <= GATES["bf16x3"][0]


def test_batch_independence_and_determinism(encoder):
    audio = torch.from_numpy(recipe.make_dac_audio(3, 29 * 512, 9)).cuda()
    for prec in ("bf16x3", "bf16"):
        out3 = encoder(audio, precision=prec, return_hidden=True)
        for b in range(3):
            one = encoder(audio[b:b + 1], precision=prec, return_hidden=True)
            for x1, x3 in zip(one, out3):
                assert torch.equal(x1[0], x3[b]), (prec, b)
        for x, y in zip(encoder(audio, precision=prec, return_hidden=True), out3):
            assert torch.equal(x, y), prec


def test_errors(sd_t):
    m = D.DacEncoder(max_B=2, max_T=16)
    m.load_state_dict(sd_t)
    m = m.cuda()
    ok = torch.zeros(2, 1, 16 * 512, device="cuda")
    assert m(ok)[0].shape == (2, 1024, 16)
    for bad in (torch.zeros(1, 1, 0, device="cuda"), torch.zeros(1, 1, 17 * 512, device="cuda"),
                torch.zeros(3, 1, 512, device="cuda"), torch.zeros(1, 2, 512, device="cuda"),
                torch.zeros(1, 1, 700, device="cuda"), torch.zeros(1, 1, 512)):
        with pytest.raises(L.JatError):
            m(bad)
    for nq in (0, 10):
        with pytest.raises(L.JatError):
            m(ok, n_quantizers=nq)
    with pytest.raises(ValueError):
        m(ok, precision="fp8")
    # the C ABI rejects the same calls itself
    h = m._handle
    z = torch.empty(2, 1024, 16, device="cuda")
    for B, T, nq, prec in ((0, 8, 9, 0), (1, 0, 9, 0), (3, 8, 9, 0), (1, 17, 9, 0), (1, 8, 0, 0), (1, 8, 10, 0),
                           (1, 8, 9, 2)):
        with pytest.raises(L.JatError):
            D._check(L.lib().jat_dac_encode(h.ptr, L.ptr(ok), L.ptr(z), None, None, None, B, T, nq, prec, L.stream_ptr()))
    named = dict(sd_t)
    del named["encoder.block.2.res_unit3.snake2.alpha"]
    with pytest.raises(L.JatError, match="encoder.block.2.res_unit3.snake2.alpha"):
        D._EncHandle(named, m.dims, 1, 8, torch.device("cuda"))
    named = dict(sd_t)
    named["quantizer.quantizers.4.codebook.weight"] = torch.zeros(1024, 7)
    with pytest.raises(L.JatError, match="quantizer.quantizers.4.codebook.weight"):
        D._EncHandle(named, m.dims, 1, 8, torch.device("cuda"))
    with pytest.raises(L.JatError):
        D._EncHandle(sd_t, dict(m.dims, codebook_dim=16), 1, 8, torch.device("cuda"))
    with pytest.raises(L.JatError):
        D._check(L.lib().jat_k_dac_head(None, None, None, None, None, None, None, 1, 8, 48, L.stream_ptr()))
    with pytest.raises(L.JatError):
        D._check(L.lib().jat_k_dac_rvq(*([None] * 10), 1, 8, 512, 9, L.stream_ptr()))
    with pytest.raises(L.JatError):
        D._check(L.lib().jat_k_dac_rvq(*([None] * 10), 1, 8, 1024, 10, L.stream_ptr()))
    torch.cuda.synchronize()


def test_infer_cli_from_wav(tmp_path, sd_t):
    from jatsr_amd.infer import main as infer_main
    cfg = dict(recipe.CONFIGS["micro"], input_channels=1024, cond_channels=1024)
    T = 200                                               # one chunk
    jsd = recipe.make_state_dict(cfg)
    torch.save({"model_state_dict": {k: torch.from_numpy(v) for k, v in jsd.items()}, "config": dict(cfg)},
               tmp_path / "last.pt")
    import json
    ones, zeros = [1.0] * 1024, [0.0] * 1024
    (tmp_path / "stats.json").write_text(json.dumps({"hr_mean": zeros, "hr_std": ones, "lr_mean": zeros, "lr_std": ones}))
    full = {"decoder." + k: torch.from_numpy(v) for k, v in recipe.make_dac_state_dict().items()}
    full.update(sd_t)
    torch.save(full, tmp_path / "dac.pt")
    x = recipe.make_dac_audio(1, T * 512 - 100, 31)[0, 0]     # not a multiple of 512: encode pads to T frames
    jio.write_wav_float32(tmp_path / "clip.wav", x, 44100)
    base = ["--checkpoint", str(tmp_path / "last.pt"), "--stats-file", str(tmp_path / "stats.json"), "--steps", "2",
            "--seed", "3", "--input-audio", str(tmp_path / "clip.wav")]
    infer_main(base + ["--output-dir", str(tmp_path / "out"), "--dac-weights", str(tmp_path / "dac.pt")])
    out = torch.load(tmp_path / "out" / "clip_generated.pt", weights_only=False)
    assert "hr_latent" not in out and out["lr_latent"].shape == (1024, T)
    codec = D.load_dac_codec(tmp_path / "dac.pt")
    xr, sr = jio.read_wav(tmp_path / "clip.wav")
    assert sr == 44100
    z = codec.encode(torch.from_numpy(xr).cuda()[None, None])[0]
    torch.testing.assert_close(out["lr_latent"], z[0].cpu().half(), rtol=0, atol=0)
    names = sorted(f for f in os.listdir(tmp_path / "out") if f.endswith(".wav"))
    assert names == ["clip_generated.wav", "clip_lr_input.wav"]      # no HR latent, so no HR WAV
    for name in names:
        raw = (tmp_path / "out" / name).read_bytes()
        assert np.frombuffer(raw[raw.index(b"data") + 8:], "<f4").size == T * 512
    # a rate other than 44.1 kHz is refused
    jio.write_wav_float32(tmp_path / "r48.wav", x[:4800], 48000)
    with pytest.raises(SystemExit, match="resampling is not provided"):
        infer_main(base[:-1] + [str(tmp_path / "r48.wav"), "--output-dir", str(tmp_path / "o2"), "--dac-weights",
                                str(tmp_path / "dac.pt")])
    # a decoder-only file cannot encode
    torch.save({k: v for k, v in full.items() if k.startswith("decoder.")}, tmp_path / "dec.pt")
    with pytest.raises(L.JatError, match="no encoder"):
        D.load_dac_codec(tmp_path / "dec.pt").encode(torch.zeros(1, 1, 512, device="cuda"))


_FP16_CHILD = """
import sys, numpy as np, torch
sys.path.insert(0, 'tests')
import jatsr_amd.dac as D, jatsr_amd.recipe as recipe
from jatsr_amd import _lib as L
from helpers import load_golden
assert L.operand_dtype() == 'fp16'
g, _ = load_golden('dac44k_enc_B2_T24')
m = D.DacEncoder(); m.load_state_dict({k: torch.from_numpy(v) for k, v in recipe.make_dac_encoder_state_dict().items()})
m = m.cuda()
out = {}
for prec in ('bf16x3', 'bf16'):
    z, c, l, h = m(torch.from_numpy(g['audio']).cuda(), precision=prec, return_hidden=True)
    out.update({prec + '_z': z.cpu().numpy(), prec + '_c': c.cpu().numpy(), prec + '_l': l.cpu().numpy(),
                prec + '_h': h.cpu().numpy()})
np.savez(sys.argv[1], **out)
"""


def test_fp16_library_same_bits(encoder, tmp_path):
    out = tmp_path / "fp16.npz"
    env = dict(os.environ, JAT_OPERAND_DTYPE="fp16")
    env.pop("JAT_LIB_PATH", None)
    r = subprocess.run([sys.executable, "-c", _FP16_CHILD, str(out)], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    got = np.load(out)
    g, _ = load_golden("dac44k_enc_B2_T24")
    for prec in ("bf16x3", "bf16"):
        z, c, lat, h = encoder(torch.from_numpy(g["audio"]).cuda(), precision=prec, return_hidden=True)
        for key, x in (("_z", z), ("_c", c), ("_l", lat), ("_h", h)):
            np.testing.assert_array_equal(got[prec + key], x.cpu().numpy())
