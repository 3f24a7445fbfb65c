"""Which launch a weight gradient takes (csrc/gemm_tn.hip `gemm_tn_tile` / `gemm_tn_ksplit`, reported by
`jat_k_weight_grad_plan`), against a Python restatement of the rule; and proof that every weight of every model
`jat_model_create` admits has widths the weight-gradient GEMM takes, which is why the trainer has no other path.  No GPU."""
import ctypes as C
import itertools
import os

import pytest

import jatsr_amd._lib as L
import jatsr_amd.recipe as recipe
from weight_grad_rule import dw_shapes, tn_path

TOKENS = (1, 63, 64, 100, 511, 512, 1100, 2048, 9660, 11040)
WIDTHS = range(128, 5121, 128)


@pytest.fixture(scope="module", autouse=True)
def built_lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.lib()


def plan(out, inn, tokens):
    tile, ks = C.c_int32(-1), C.c_int32(-1)
    L.check(L.lib().jat_k_weight_grad_plan(out, inn, tokens, C.byref(tile), C.byref(ks)))
    return tile.value, ks.value


def test_plan_matches_the_rule_for_every_width_to_5120():
    bad = [(o, i, t, plan(o, i, t), tn_path(o, i, t)) for o in WIDTHS for i in WIDTHS for t in TOKENS if plan(o, i, t) != tn_path(o, i, t)]
    assert not bad, bad[:10]
    # the four launch paths (tile x one / several slices) and the MLP weights at the benchmarked shape
    assert plan(128, 128, 100) == (128, 1)
    assert plan(256, 256, 1100)[0] == 128 and plan(256, 256, 1100)[1] > 1
    assert plan(1024, 1024, 200) == (256, 1)
    assert plan(1024, 1024, 1100)[0] == 256 and plan(1024, 1024, 1100)[1] > 1
    assert plan(5120, 1280, 9660) == (256, 2)
    assert all(1 <= plan(o, i, t)[1] <= min(16, max(1, (t + 63) // 64)) for o in (128, 1280, 5120) for i in (128, 1280) for t in TOKENS)


def test_bad_arguments_are_an_error_not_a_plan():
    tile, ks = C.c_int32(-1), C.c_int32(-1)
    f = L.lib().jat_k_weight_grad_plan
    assert f(256, 256, 100, None, C.byref(ks)) == L.JAT_E_INVALID
    assert f(256, 256, 100, C.byref(tile), None) == L.JAT_E_INVALID
    for out, inn, tokens in ((0, 256, 100), (256, 0, 100), (256, 256, 0), (-128, 256, 100), (256, -256, 100), (256, 256, -5),
                             (192, 256, 100), (256, 192, 100), (64, 64, 100), (1280, 1000, 9660)):
        assert f(out, inn, tokens, C.byref(tile), C.byref(ks)) == L.JAT_E_INVALID, (out, inn, tokens)
    assert (tile.value, ks.value) == (-1, -1)                           # nothing was written


def admitted_configs():
    """A grid over what jat_model_create admits: hidden_size % 256 == 0 (<= 2048), head_dim 64, num_kv_heads | num_q_heads,
    bottleneck_dim and mlp_hidden multiples of 128, channel counts multiples of 32, patch_len 4."""
    for D in range(256, 2049, 256):
        Hq = D // 64
        for Hkv in (h for h in range(1, Hq + 1) if Hq % h == 0):
            for bott, mlp, Cin, Cc in itertools.product((128, 512), (128, 4 * D), (32, 96, 1024), (32, 96, 1024)):
                yield dict(hidden_size=D, num_kv_heads=Hkv, bottleneck_dim=bott, mlp_hidden=mlp, input_channels=Cin, cond_channels=Cc)


def test_every_weight_of_every_admitted_model_has_widths_the_gemm_takes():
    n = 0
    for cfg in admitted_configs():
        shapes = dw_shapes(**cfg)
        assert len(shapes) == 7
        for out, inn in shapes:
            assert out % 128 == 0 and inn % 128 == 0, (cfg, out, inn)
            assert plan(out, inn, 9660)[0] in (128, 256)                # the library takes it
        n += 1
    assert n == sum(len([h for h in range(1, D // 64 + 1) if (D // 64) % h == 0]) for D in range(256, 2049, 256)) * 2 * 2 * 9
    assert set(recipe.CONFIGS) == {"v3mod2", "tiny", "wide2", "micro"}
    for name, cfg in recipe.CONFIGS.items():
        D = cfg["hidden_size"]
        assert D // cfg["num_q_heads"] == 64 and cfg["patch_len"] == 4, name
        shapes = dw_shapes(D, cfg["num_kv_heads"], cfg["bottleneck_dim"], int(D * cfg["mlp_ratio"]), cfg["input_channels"],
                           cfg["cond_channels"])
        assert all(out % 128 == 0 and inn % 128 == 0 for out, inn in shapes), (name, shapes)
        for out, inn in shapes:
            plan(out, inn, 9660)
    micro = recipe.CONFIGS["micro"]
    assert sorted({w for s in dw_shapes(256, micro["num_kv_heads"], 128, 1024, 32, 32) for w in s}) == [128, 256, 512, 1024]
