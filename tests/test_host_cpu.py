"""CPU-side tests (no GPU): the C-ABI library loads and exports every declared symbol, host validation
mirrors the reference's error behaviour, state_dict layout matches the reference, and the product path
fails loudly instead of falling back to a CPU implementation."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import jatsr_amd
import jatsr_amd._lib as L
import jatsr_amd.recipe as recipe
from jatsr_amd.model import JaT_AudioSR_V2, JaT_AudioSR_V3, load_model
from oracle import jat_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
no_gpu = not torch.cuda.is_available()


@pytest.fixture(scope="session", autouse=True)
def built_lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.lib()


def test_library_exports_every_declared_symbol(built_lib):
    header = open(os.path.join(ROOT, "include", "jat_hip.h")).read()
    declared = set(re.findall(r"\b(jat_[a-z0-9_]+)\s*\(", header))
    assert declared == set(L.SIGNATURES), declared ^ set(L.SIGNATURES)
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (jat_[a-z0-9_]+)", nm))
    assert declared <= exported, declared - exported
    assert built_lib.jat_version() >= 1


def _create(**over):
    base = dict(input_channels=1024, cond_channels=1024, patch_len=4, hidden_size=1280, depth=28, num_q_heads=20,
                num_kv_heads=4, bottleneck_dim=512, mlp_hidden=5120, norm_mode=0)
    base.update(over)
    cfg = L.JatConfig(*[base[n] for n, _ in L.JatConfig._fields_])
    h = C.c_void_p()
    rc = L.lib().jat_model_create(C.byref(cfg), C.byref(h))
    return rc, h


def test_model_create_validation_and_workspace():
    rc, h = _create()
    assert rc == 0 and h
    sizes = []
    for B, T in [(1, 512), (28, 512), (56, 512), (56, 1378)]:
        sz = C.c_size_t()
        assert L.lib().jat_model_workspace_bytes(h, B, T, C.byref(sz)) == 0
        sizes.append(sz.value)
    assert sizes == sorted(sizes) and sizes[0] > 0
    # forward before load_weights -> state error, never a silent fallback
    rc2 = L.lib().jat_forward(h, None, None, None, None, 1, 8, None, 0, None)
    assert rc2 == L.JAT_E_STATE
    L.lib().jat_model_destroy(h)
    for bad in (dict(num_q_heads=3), dict(num_kv_heads=3), dict(patch_len=2), dict(hidden_size=1000, num_q_heads=10),
                dict(norm_mode=7), dict(depth=0)):
        rc, _ = _create(**bad)
        assert rc == L.JAT_E_INVALID, bad
        assert L.lib().jat_last_error()


def _route(N, npad, lse=0, drop=0, lib=None):
    g, qt, kvb = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    rc = (lib or L.lib()).jat_k_attention_route(N, npad, lse, drop, C.byref(g), C.byref(qt), C.byref(kvb))
    return rc, (g.value, qt.value, kvb.value)


def test_attention_route_by_default_and_under_the_switches():
    """`jat_k_attention_route` (the function `launch_attention` launches by): the group kernel for an eval call of at most 128
    tokens whose V is padded to 128 keys or more, else attn_fwd_kernel<1, 64>; the training forward (lse, dropout) never takes
    the group kernel.  The switches are read once per process: each setting in a fresh child (tests/test_gpu_widths.py runs the
    kernels under the same three settings)."""
    if not any(os.environ.get(k) for k in ("JAT_ATTN_GROUP", "JAT_ATTN_QT", "JAT_ATTN_KVB")):
        assert _route(128, 128) == (0, (1, 1, 64)) and _route(100, 128) == (0, (1, 1, 64)) and _route(1, 128) == (0, (1, 1, 64))
        assert _route(64, 64) == (0, (0, 1, 64)) and _route(129, 192) == (0, (0, 1, 64)) and _route(2048, 2048) == (0, (0, 1, 64))
        assert _route(128, 128, lse=1) == (0, (0, 1, 64)) and _route(128, 128, drop=1) == (0, (0, 1, 64))
    g = C.c_int32(-1)
    for bad in ((0, 64), (-3, 64), (65, 64), (64, 100)):
        assert _route(*bad) == (L.JAT_E_INVALID, (-1, -1, -1)), bad
    assert L.lib().jat_k_attention_route(64, 64, 0, 0, None, C.byref(g), C.byref(g)) == L.JAT_E_INVALID and g.value == -1
    code = ("import ctypes as C, jatsr_amd._lib as L\n"
            "def r(N, npad, lse=0):\n"
            "    o = [C.c_int32(-1) for _ in range(3)]\n"
            "    L.check(L.lib().jat_k_attention_route(N, npad, lse, 0, *[C.byref(x) for x in o]))\n"
            "    return tuple(x.value for x in o)\n"
            "print(r(128, 128), r(345, 384), r(128, 128, 1), r(64, 64))\n")
    for env, want in ((dict(JAT_ATTN_KVB="128", JAT_ATTN_GROUP="0"), "(0, 1, 128) (0, 1, 128) (0, 1, 128) (0, 1, 64)"),
                      (dict(JAT_ATTN_QT="2", JAT_ATTN_GROUP="0"), "(0, 2, 64) (0, 2, 64) (0, 2, 64) (0, 2, 64)"),
                      (dict(JAT_ATTN_KVB="128", JAT_ATTN_QT="2"), "(1, 2, 128) (0, 2, 128) (0, 2, 128) (0, 2, 64)")):
        out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, **env), capture_output=True, text=True,
                             timeout=120)
        assert out.returncode == 0 and out.stdout.strip() == want, (env, out.stdout, out.stderr[-500:])


@pytest.mark.parametrize("cfg_name", ["micro", "tiny"])
@pytest.mark.parametrize("norm", ["rms", "ln"])
def test_state_dict_layout_matches_reference(cfg_name, norm):
    cfg = recipe.CONFIGS[cfg_name]
    m = (JaT_AudioSR_V3 if norm == "rms" else JaT_AudioSR_V2)(**cfg, dropout=0.1, drop_path_rate=0.05)
    sd = m.state_dict()
    want = recipe.model_param_shapes(cfg, norm)
    params = {k: tuple(v.shape) for k, v in sd.items() if ".rope." not in k}
    assert params == dict(want)
    # persistent RoPE buffers are part of the reference checkpoint format (jat_audiosr_v3.py:78,84-85)
    inv, cos, sin = recipe.rope_buffers(64)
    assert torch.allclose(sd["blocks.0.attn.rope.inv_freq"], torch.from_numpy(inv), rtol=1e-6)
    assert sd["blocks.0.attn.rope.cos_cached"].shape == (4096, 64)
    # 1-ulp differences in powf() for inv_freq grow to ~2e-4 rad at position 4095
    assert torch.allclose(sd["blocks.1.attn.rope.sin_cached"], torch.from_numpy(sin), atol=1e-3)
    # zero-init of adaLN + final linear (jat_audiosr_v3.py:395-404)
    assert float(sd["blocks.0.adaLN_modulation.1.weight"].abs().max()) == 0.0
    assert float(sd["final_layer.1.weight"].abs().max()) == 0.0


def test_load_model_strips_prefixes_and_is_non_strict():
    cfg = recipe.CONFIGS["micro"]
    sd = {("_orig_mod.module." + k): torch.from_numpy(v) for k, v in recipe.make_state_dict(cfg).items()}
    sd.pop("_orig_mod.module.blocks.0.norm1.weight")     # strict=False: missing keys tolerated (:74)
    ck = {"model_state_dict": sd, "config": dict(cfg, dropout=0.1, drop_path_rate=0.05), "epoch": 3, "global_step": 99}
    m = load_model(ck, device="cpu")
    assert isinstance(m, JaT_AudioSR_V3) and not m.training
    assert m.load_info["epoch"] == 3 and "blocks.0.norm1.weight" in m.load_info["missing"]
    assert torch.equal(m.blocks[1].attn.q_proj.weight, sd["_orig_mod.module.blocks.1.attn.q_proj.weight"])


@pytest.mark.skipif(not no_gpu, reason="checks the no-GPU failure mode")
def test_product_path_fails_loudly_without_gpu():
    m = JaT_AudioSR_V3(**recipe.CONFIGS["micro"])
    x = torch.zeros(1, 32, 8)
    with pytest.raises(L.JatError):
        m(x, torch.zeros(1), x)
    with pytest.raises(L.JatError):
        jatsr_amd.flow_matching_sample(m, x, num_steps=2, verbose=False)
    with pytest.raises(L.JatError):
        m.blocks[0](torch.zeros(1, 2, 256), torch.zeros(1, 256))


def test_product_does_not_import_oracle():
    """The product package must never import or call the oracle (it is test infrastructure)."""
    pkg = os.path.join(ROOT, "jatsr-just-audio-transformer-super-solution_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h")):
                assert "oracle" not in open(os.path.join(dp, f), encoding="utf-8").read().replace(
                    "CPU oracle", "").replace("the oracle", ""), f


def test_recipe_is_deterministic_and_flops_closed_form():
    u = recipe.uniform("a", (4,))
    assert np.allclose(u, [-0.16541618, 0.8985061, 0.58957404, 0.12038141])
    assert recipe.forward_flops(recipe.CONFIGS["v3mod2"], 1, 512) == 127627689984
    for c, B, T in (("tiny", 2, 128), ("micro", 3, 22), ("v3mod2", 28, 1378)):
        assert recipe.forward_flops(recipe.CONFIGS[c], B, T) == O.forward_flops(recipe.CONFIGS[c], B, T)


def test_chunk_plan_and_shard_range():
    from jatsr_amd.dist import shard_range
    from jatsr_amd.sampler import chunk_plan
    assert chunk_plan(4096) == O.chunk_plan(4096)
    assert chunk_plan(500, 200, 40) == O.chunk_plan(500, 200, 40)
    sizes = [shard_range(28, 8, r) for r in range(8)]
    assert [b - a for a, b in sizes] == [4, 4, 4, 4, 3, 3, 3, 3]
    assert sizes[0][0] == 0 and sizes[-1][1] == 28 and all(sizes[i][1] == sizes[i + 1][0] for i in range(7))
    assert shard_range(2, 4, 3) == (2, 2)


def test_fast_gelu_expression_is_far_below_a_bf16_ulp():
    """csrc/gemm.hip `gelu_erf_n` evaluates nn.GELU() (erf form, jat_audiosr_v3.py:223,268) as x * clamp01(1/2 + x * Q(s)),
    s = clamp01((x / 4.5)^2), Q of degree 8 in s (no transcendental; the clamps are free output modifiers); the same fp32
    expression in numpy against scipy's erf: |error| <= 7e-5 for all x (the result is then rounded to bf16: half an ulp
    is 2e-3 at |gelu| ~ 1); beyond 4.5 Phi saturates at exactly 0 / 1."""
    import numpy as np
    from scipy.special import erf
    m = np.array([0.398712717, -1.33619357, 3.9305869, -8.61624417, 13.6928242, -15.1604596, 10.9725412, -4.62950545,
                  0.858849732], np.float32)

    def fma(a, b, c):     # one rounding, like v_fma_f32
        return (a.astype(np.float64) * b.astype(np.float64) + np.float64(c)).astype(np.float32)

    def gelu_fast(x):
        x = x.astype(np.float32)
        xs = (x * np.float32(0.22222222)).astype(np.float32)
        s = np.clip(fma(xs, xs, 0.0), 0, 1).astype(np.float32)
        q = np.full_like(s, m[-1])
        for k in range(len(m) - 2, -1, -1):
            q = fma(q, s, m[k])
        phi = np.clip(fma(x, q, 0.5), 0, 1).astype(np.float32)
        return (x * phi).astype(np.float32)
    x = np.linspace(-8, 8, 1_600_001).astype(np.float32)
    ref = x.astype(np.float64) * 0.5 * (1 + erf(x.astype(np.float64) / np.sqrt(2)))
    assert np.abs(gelu_fast(x) - ref).max() < 7e-5
    big = np.array([10.0, 100.0, 1e4], np.float32)
    assert np.all(np.abs(gelu_fast(big) / big - 1) < 1.2e-5)
    assert np.all(np.abs(gelu_fast(-big)) < 1.2e-5 * big)


def test_gemm_plan_matches_the_recorded_plans():
    """Which tile variant and K-split the forward gives each GEMM (csrc/gemm_plan.cpp through jat_k_gemm_plan) against
    tests/golden/gemm_plan.json, recorded before the planner was moved out of jat_api.cpp (tools/gen_gemm_plan_golden.py says
    how): every entry, exactly.  The chooser reads its A/B variables once per process, so the plans are collected in a child
    process without them."""
    import json
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_gemm_plan_golden as G
    finally:
        sys.path.pop(0)
    env = {k: v for k, v in os.environ.items() if k not in G.CHOOSER_ENV}
    got = json.loads(subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_gemm_plan_golden.py"), "--print"],
                                    capture_output=True, text=True, check=True, env=env, cwd=ROOT).stdout)
    want = json.load(open(G.PATH))
    assert got["M"] == want["M"] == G.MS and got["NK"] == want["NK"]
    assert set(got["plans"]) == set(want["plans"]) == set(G.MODELS)
    n = 0
    for model, by_switch in want["plans"].items():
        assert set(got["plans"][model]) == set(by_switch) == set(G.SWITCHES)
        for sw, table in by_switch.items():
            for site in range(5):
                for folding in (0, 1):
                    for i, (N, K) in enumerate(want["NK"][model]):
                        for j, M in enumerate(want["M"]):
                            assert got["plans"][model][sw][site][folding][i][j] == table[site][folding][i][j], \
                                (model, sw, site, folding, M, N, K)
                            n += 1
    assert n == 2 * 3 * 5 * 2 * 9 * len(G.MS)


def test_gemm_variant_table_is_consistent():
    """The variant table (csrc/gemm_variants.h) against itself: the wave-tile width of every id 0..39 is what it was before the
    table replaced the hand-kept arrays (recorded in tests/golden/gemm_plan.json), and the live ids are the ones the GPU tests
    sweep (tests/test_gpu_kernels.py LIVE_VARIANTS)."""
    import json
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "gemm_plan.json")))["wave_n"]
    got = [L.lib().jat_k_gemm_wave_n(v) for v in range(40)]
    assert len(want) == 40 and got == want
    src = open(os.path.join(ROOT, "tests", "test_gpu_kernels.py")).read()
    live = [int(v) for v in re.search(r"^LIVE_VARIANTS = \[([0-9, ]+)\]", src, re.M).group(1).split(",")]
    assert [v for v in range(40) if got[v]] == live
    assert L.lib().jat_k_gemm_wave_n(-1) == 0 and L.lib().jat_k_gemm_wave_n(40) == 0
    # every plan the forward makes names a live variant
    plans = json.load(open(os.path.join(ROOT, "tests", "golden", "gemm_plan.json")))["plans"]
    used = {p[0] for m in plans.values() for t in m.values() for a in t for b in a for c in b for p in c}
    assert used <= set(live)
