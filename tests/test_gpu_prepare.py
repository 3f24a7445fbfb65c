"""Audio -> latent pairs on the GPU (jatsr_amd.prepare, jatsr_amd.infer --resample / --simulate-lr) with the recipe's
synthetic DAC weights: `prepare_audio` is the composition of `resample` and `codec.encode` in the reference's order and
nothing else (bit for bit), the audio entering the encoder follows the fp64 restatement of the chain, the statistics match
numpy on the saved fp16 tensors, and the command lines write what the trainer and the inference tool read."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import resample_ref as R  # noqa: E402
import jatsr_amd.dac as D  # noqa: E402
import jatsr_amd.io as jio  # noqa: E402
import jatsr_amd.recipe as recipe  # noqa: E402
from jatsr_amd.prepare import chunk_bounds, prepare_audio  # noqa: E402
from jatsr_amd.resample import resample, simulate_lr  # noqa: E402


@pytest.fixture(scope="module")
def dac_file(tmp_path_factory):
    full = {"decoder." + k: torch.from_numpy(v) for k, v in recipe.make_dac_state_dict().items()}
    full.update({k: torch.from_numpy(v) for k, v in recipe.make_dac_encoder_state_dict().items()})
    path = tmp_path_factory.mktemp("dac") / "dac.pt"
    torch.save(full, path)
    return str(path)


@pytest.fixture(scope="module")
def codec(dac_file):
    return D.load_dac_codec(dac_file)


def clip(seconds, sr, salt):
    return recipe.make_dac_audio(1, int(round(seconds * sr)), salt, sample_rate=sr)[0, 0]


def expected_frames(total, sr):
    """the reference's frame count for a file (prepare_dataset_v5.py:221-245) with the 44.1 kHz codec's hop of 512"""
    len48 = 8 * 48000
    frames = -(-R.out_length(len48, 48000, 44100) // 512)
    hop48 = len48 / frames
    trim, valid = int(int(0.5 * 48000) / hop48), int(int(7.0 * 48000) / hop48)
    return trim, valid, int(int(total / sr * 48000) / hop48)


@pytest.mark.parametrize("seconds,sr,salt", [(9.3, 22050, 41), (7.0, 48000, 42)])
def test_prepare_audio_is_the_composition(codec, seconds, sr, salt):
    x = clip(seconds, sr, salt)
    res = prepare_audio(x, sr, codec)
    trim, valid, frames = expected_frames(len(x), sr)
    assert (trim, valid) == (43, 603)
    assert res["hr_latent"].shape == res["lr_latent"].shape == (1024, frames) and res["count"] == frames
    assert res["metadata"]["trim_frames"] == trim and res["metadata"]["valid_frames"] == valid
    # by hand: chunks -> 48 kHz -> LR simulation -> 44.1 kHz -> encode -> trim -> concatenate -> cut
    xg = torch.from_numpy(x).cuda()
    chunks = torch.stack([torch.nn.functional.pad(xg[a:b], (pl, pr)) for a, b, pl, pr in R.chunk_bounds(len(x), sr)])
    assert chunks.shape == (int(np.ceil(seconds / 7.0)), 8 * sr)
    hr48 = resample(chunks, sr, 48000) if sr != 48000 else chunks
    lr48 = simulate_lr(hr48, 48000, 16000)
    assert hr48.shape == lr48.shape == (chunks.shape[0], 8 * 48000)
    hr44, lr44 = (resample(v, 48000, 44100, 24, 0.945) for v in (hr48, lr48))
    z_hr, z_lr = (codec.encode(v[:, None])[0] for v in (hr44, lr44))
    by_hand = [torch.cat(list(z[..., trim:trim + valid]), dim=-1)[..., :frames] for z in (z_hr, z_lr)]
    assert torch.equal(res["hr_latent"], by_hand[0]) and torch.equal(res["lr_latent"], by_hand[1])
    assert not torch.equal(res["hr_latent"], res["lr_latent"])
    # the 44.1 kHz audio entering the encoder against the fp64 chain (four resampling stages for LR): rel-L2 <= 4e-6
    c64 = chunks.cpu().numpy().astype(np.float64)
    r_hr48 = R.resample(c64, sr, 48000) if sr != 48000 else c64
    r_lr48 = R.simulate_lr(r_hr48)
    for name, got, ref48 in (("hr", hr44, r_hr48), ("lr", lr44, r_lr48)):
        ref = R.resample(ref48, 48000, 44100, 24, 0.945)
        g = got.cpu().numpy().astype(np.float64)
        rel = float(np.linalg.norm(g - ref) / np.linalg.norm(ref))
        print(f"{seconds} s at {sr} Hz, {name} audio at 44.1 kHz: rel-L2 {rel:.2e} (gate 4e-6)")   # measured: 1.4e-7 .. 1.9e-7
        assert g.shape == ref.shape and rel <= 4e-6
    # statistics of the fp16 tensors a latent file holds: HR channels first, then LR
    v = torch.cat([res["hr_latent"], res["lr_latent"]]).half().double().cpu().numpy()
    mag = np.abs(v).sum(axis=1)
    assert res["sum"].shape == res["sq_sum"].shape == (2048,) and res["sum"].dtype == torch.float64
    assert (np.abs(res["sum"].cpu().numpy() - v.sum(axis=1)) <= 1e-12 * mag).all()
    assert (np.abs(res["sq_sum"].cpu().numpy() - (v * v).sum(axis=1)) <= 1e-12 * (v * v).sum(axis=1)).all()
    # the batch size does not change a bit
    one = prepare_audio(x, sr, codec, batch=1)
    assert torch.equal(one["hr_latent"], res["hr_latent"]) and torch.equal(one["lr_latent"], res["lr_latent"])


def test_prepare_audio_peak_mono_and_short(codec):
    x = clip(2.0, 16000, 43)
    unit = (x / np.abs(x).max()).astype(np.float32)                               # peak exactly 1
    loud = prepare_audio(4.0 * unit, 16000, codec)                                # peak 4 -> divided by its peak, exactly
    ref = prepare_audio(unit, 16000, codec)
    assert loud["hr_latent"].shape == (1024, expected_frames(len(x), 16000)[2])
    assert torch.equal(loud["hr_latent"], ref["hr_latent"]) and torch.equal(loud["lr_latent"], ref["lr_latent"])
    quiet = prepare_audio(0.5 * unit, 16000, codec)                               # a peak below 1 is left alone
    assert not torch.equal(quiet["hr_latent"], ref["hr_latent"])
    stereo = prepare_audio(np.stack([x, x]), 16000, codec)
    assert torch.equal(stereo["hr_latent"], prepare_audio(x, 16000, codec)["hr_latent"])
    assert prepare_audio(x[:15999], 16000, codec) is None                         # shorter than 1 s
    with pytest.raises(ValueError):
        prepare_audio(x, 0, codec)


def _write_wavs(folder):
    os.makedirs(folder, exist_ok=True)
    for name, seconds, sr, salt in (("a", 2.5, 16000, 51), ("b", 8.2, 22050, 52), ("short", 0.5, 44100, 53)):
        jio.write_wav_float32(os.path.join(folder, f"{name}.wav"), clip(seconds, sr, salt), sr)


def test_prepare_cli_writes_what_the_trainer_reads(tmp_path, dac_file, capsys):
    import jatsr_amd
    from jatsr_amd.prepare import main as prepare_main
    _write_wavs(tmp_path / "wav")
    argv = ["--source-dir", str(tmp_path / "wav"), "--output-dir", str(tmp_path / "out"), "--dac-weights", dac_file,
            "--val-fraction", "0.34", "--seed", "1"]
    rep = prepare_main(argv)
    printed = capsys.readouterr().out
    assert len(rep["written"]) == 2 and [os.path.basename(p) for p in rep["skipped"]] == ["short.wav"]
    assert "skipped" in printed and "short.wav" in printed
    files = sorted(os.path.join(dp, f) for dp, _, fs in os.walk(tmp_path / "out") for f in fs if f.endswith(".pt")
                   and f != "running_stats.pt")
    assert sorted(os.path.basename(f) for f in files) == ["a.pt", "b.pt"]
    assert {os.path.basename(os.path.dirname(f)) for f in files} <= {"train", "val"}
    pairs = [jio.load_latent_file(f) for f in files]
    for (hr, lr), f in zip(pairs, files):
        meta = torch.load(f, weights_only=False)["metadata"]
        assert set(meta) == {"name", "path", "duration", "sr"} and meta["name"] in ("a", "b")
        assert hr.shape == lr.shape == (1024, expected_frames(int(round(meta["duration"] * meta["sr"])), meta["sr"])[2])
    stats = jio.load_stats(str(tmp_path / "out" / "global_stats_separated.json"))
    for i, key in enumerate(("hr", "lr")):
        v = torch.cat([p[i] for p in pairs], dim=1).double().numpy()
        mean = v.mean(axis=1)
        std = np.sqrt(np.maximum((v * v).mean(axis=1) - mean ** 2, 1e-6))
        assert np.allclose(stats[f"{key}_mean"].numpy(), mean, rtol=1e-5, atol=1e-7)
        assert np.allclose(stats[f"{key}_std"].numpy(), std, rtol=1e-5, atol=1e-7)
    running = torch.load(tmp_path / "out" / "running_stats.pt", weights_only=False)
    assert running["count"] == sum(p[0].shape[1] for p in pairs) and running["sum"].shape == (2048,)
    from_running = jio.load_stats(str(tmp_path / "out" / "running_stats.pt"))
    assert np.allclose(from_running["hr_mean"].numpy(), stats["hr_mean"].numpy(), rtol=1e-6, atol=1e-7)
    # a second run writes nothing and leaves the statistics alone
    before = {f: open(f, "rb").read() for f in files + [str(tmp_path / "out" / "global_stats_separated.json")]}
    rep2 = prepare_main(argv)
    assert rep2["written"] == [] and len(rep2["existing"]) == 2
    assert all(open(f, "rb").read() == b for f, b in before.items())
    again = torch.load(tmp_path / "out" / "running_stats.pt", weights_only=False)
    assert again["count"] == running["count"] and torch.equal(again["sum"], running["sum"])
    # a file added later is folded into the running totals
    jio.write_wav_float32(str(tmp_path / "wav" / "c.wav"), clip(1.5, 48000, 54), 48000)
    rep3 = prepare_main(argv)
    assert [os.path.basename(p) for p in rep3["written"]] == ["c.pt"]
    hr_c, _ = jio.load_latent_file(rep3["written"][0])
    third = torch.load(tmp_path / "out" / "running_stats.pt", weights_only=False)
    assert third["count"] == running["count"] + hr_c.shape[1]
    assert torch.allclose(third["sum"][:1024], running["sum"][:1024] + hr_c.double().sum(dim=1), rtol=0, atol=1e-9)

    # one training step of a micro model on a batch cut from the written files with the written statistics
    from jatsr_amd.train import Trainer
    cfg = dict(recipe.CONFIGS["micro"], input_channels=1024, cond_channels=1024)
    model = jatsr_amd.JaT_AudioSR_V3(**cfg, dropout=0.0, drop_path_rate=0.0)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in recipe.make_state_dict(cfg).items()}, strict=False)
    frames = 64
    tr = Trainer(model.to("cuda"), batch_size=2, frames=frames, use_grad_scaler=False, distributed=False, seed=0)
    hr = torch.stack([p[0][:, :frames] for p in pairs]).cuda()
    lr = torch.stack([p[1][:, :frames] for p in pairs]).cuda()
    st = jio.load_stats(str(tmp_path / "out" / "global_stats_separated.json"), device="cuda")
    out = tr.train_step(hr, lr, st["hr_mean"], st["hr_std"], st["lr_mean"], st["lr_std"])
    assert np.isfinite(out["loss"]) and out["loss"] > 0


def _infer_setup(tmp_path):
    cfg = dict(recipe.CONFIGS["micro"], input_channels=1024, cond_channels=1024)
    torch.save({"model_state_dict": {k: torch.from_numpy(v) for k, v in recipe.make_state_dict(cfg).items()},
                "config": dict(cfg)}, tmp_path / "last.pt")
    ones, zeros = [1.0] * 1024, [0.0] * 1024
    (tmp_path / "stats.json").write_text(json.dumps({"hr_mean": zeros, "hr_std": ones, "lr_mean": zeros, "lr_std": ones}))
    return ["--checkpoint", str(tmp_path / "last.pt"), "--stats-file", str(tmp_path / "stats.json"), "--steps", "2",
            "--seed", "3"]


def test_infer_resample_flag(tmp_path, dac_file, codec):
    from jatsr_amd.infer import main as infer_main
    base = _infer_setup(tmp_path) + ["--dac-weights", dac_file]
    x16 = clip(3.0, 16000, 61)
    jio.write_wav_float32(tmp_path / "clip.wav", x16, 16000)
    infer_main(base + ["--input-audio", str(tmp_path / "clip.wav"), "--output-dir", str(tmp_path / "o16"), "--resample"])
    out = torch.load(tmp_path / "o16" / "clip_generated.pt", weights_only=False)
    xr, sr = jio.read_wav(tmp_path / "clip.wav")
    z = codec.encode(resample(torch.from_numpy(xr).cuda()[None], 16000, 44100)[None])[0]
    assert "hr_latent" not in out and torch.equal(out["lr_latent"], z[0].cpu().half())
    assert out["lr_latent"].shape == (1024, -(-R.out_length(len(xr), 16000, 44100) // 512))
    assert sorted(f for f in os.listdir(tmp_path / "o16") if f.endswith(".wav")) == ["clip_generated.wav", "clip_lr_input.wav"]
    # at 44.1 kHz the flag changes nothing
    jio.write_wav_float32(tmp_path / "c44.wav", clip(3.0, 44100, 62), 44100)
    for name, extra in (("plain", []), ("flag", ["--resample"])):
        infer_main(base + ["--input-audio", str(tmp_path / "c44.wav"), "--output-dir", str(tmp_path / name)] + extra)
    a = torch.load(tmp_path / "plain" / "c44_generated.pt", weights_only=False)
    b = torch.load(tmp_path / "flag" / "c44_generated.pt", weights_only=False)
    assert torch.equal(a["lr_latent"], b["lr_latent"]) and torch.equal(a["generated_latent"], b["generated_latent"])
    for wav in ("c44_generated.wav", "c44_lr_input.wav"):
        assert (tmp_path / "plain" / wav).read_bytes() == (tmp_path / "flag" / wav).read_bytes()
    with pytest.raises(SystemExit, match="need --input-audio"):
        infer_main(base + ["--input-file", "x.pt", "--resample"])


def test_infer_simulate_lr_flag(tmp_path, dac_file, codec):
    from jatsr_amd.infer import main as infer_main
    base = _infer_setup(tmp_path) + ["--dac-weights", dac_file]
    x = clip(3.0, 22050, 63)
    jio.write_wav_float32(tmp_path / "song.wav", x, 22050)
    infer_main(base + ["--input-audio", str(tmp_path / "song.wav"), "--output-dir", str(tmp_path / "o"), "--simulate-lr"])
    out = torch.load(tmp_path / "o" / "song_generated.pt", weights_only=False)
    xr, sr = jio.read_wav(tmp_path / "song.wav")
    res = prepare_audio(xr, sr, codec)
    assert torch.equal(out["hr_latent"], res["hr_latent"].cpu().half())
    assert torch.equal(out["lr_latent"], res["lr_latent"].cpu().half())
    assert out["generated_latent"].shape == out["lr_latent"].shape
    names = sorted(f for f in os.listdir(tmp_path / "o") if f.endswith(".wav"))
    assert names == ["song_generated.wav", "song_hr_gt.wav", "song_lr_input.wav"]
    for name in names:
        raw = (tmp_path / "o" / name).read_bytes()
        assert np.frombuffer(raw[raw.index(b"data") + 8:], "<f4").size == res["count"] * 512
