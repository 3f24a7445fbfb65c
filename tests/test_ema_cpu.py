"""Host side of the EMA of the weights: the decay schedule, the fp64 twin against the closed form, the state-dict choice
behind `load_model(use_ema=...)`, and the new flags of the fit / infer parsers.  No GPU."""
import numpy as np
import pytest

import ema_ref as R
from jatsr_amd import fit as F
from jatsr_amd import infer as I
from jatsr_amd.model import select_state_dict
from jatsr_amd.train import ema_decay_at


@pytest.mark.parametrize("fn", [ema_decay_at, R.ema_decay_at])
def test_decay_schedule(fn):
    assert [fn(n, 0.9999, True) for n in (1, 2, 3)] == [2 / 11, 3 / 12, 4 / 13]
    assert fn(70, 0.9, True) == 71 / 80 and fn(81, 0.9, True) == 0.9       # (1 + n) / (10 + n) reaches 0.9 at n = 80
    assert all(fn(n, 0.9, True) == 0.9 for n in (82, 1000, 10 ** 9))
    assert all(fn(n, 0.9999, False) == 0.9999 for n in (1, 2, 50, 10 ** 6))
    assert fn(5, 0.0, True) == 0.0
    vals = [fn(n, 0.9999, True) for n in range(1, 200000, 997)]
    assert all(a <= b for a, b in zip(vals, vals[1:])) and vals[-1] == 0.9999


def test_host_schedule_equals_the_twin():
    for n in list(range(1, 200)) + [10 ** 5, 10 ** 7]:
        for d in (0.0, 0.9, 0.999, 0.9999):
            for w in (True, False):
                assert ema_decay_at(n, d, w) == R.ema_decay_at(n, d, w)


@pytest.mark.parametrize("decay", [0.0, 0.9, 0.999])
def test_twin_against_the_closed_form_for_constant_parameters(decay):
    """g = 0, m = 0, no weight decay: AdamW leaves p where it is, and e_N = p + d^N (e_0 - p)."""
    rng = np.random.default_rng(3)
    p0, e0 = rng.standard_normal(64), rng.standard_normal(64)
    st = dict(p=p0, m=np.zeros(64), v=np.zeros(64), e=e0)
    N = 25
    for step in range(1, N + 1):
        st = R.adamw_ema_step(st["p"], np.zeros(64), st["m"], st["v"], st["e"], 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 1.0, step, decay)
        assert np.array_equal(st["p"], p0)
    want = p0 + decay ** N * (e0 - p0)
    assert np.abs(st["e"] - want).max() <= 4 * N * 2.0 ** -53 * np.abs(np.stack([p0, e0])).max()


def test_twin_skips_a_non_finite_step_and_moves_towards_the_new_parameters():
    rng = np.random.default_rng(4)
    p, g, m, e = (rng.standard_normal(16) for _ in range(4))
    v = np.abs(rng.standard_normal(16))
    bad = g.copy()
    bad[3] = np.inf
    out = R.adamw_ema_step(p, bad, m, v, e, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1.0, 1.0, 2, 0.9)
    assert all(np.array_equal(out[k], x) for k, x in (("p", p), ("m", m), ("v", v), ("e", e)))
    out = R.adamw_ema_step(p, g, m, v, e, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1.0, 1.0, 2, 0.9)
    assert not np.array_equal(out["p"], p) and np.allclose(out["e"], 0.9 * e + 0.1 * out["p"], rtol=0, atol=1e-15)
    # decay 0: the average follows the parameters (e + (p - e), one fp64 rounding away from p)
    assert np.allclose(R.adamw_ema_step(p, g, m, v, e, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1.0, 1.0, 2, 0.0)["e"], out["p"], rtol=0, atol=1e-15)


def test_state_dict_selector():
    raw, ema = {"w": 1}, {"w": 2}
    ck = dict(model_state_dict=raw, ema_state_dict=ema)
    assert select_state_dict(ck) == (raw, "raw") and select_state_dict(ck, use_ema=False) == (raw, "raw")
    assert select_state_dict(ck, use_ema=True) == (ema, "ema")
    assert select_state_dict(dict(model_state_dict=raw), False) == (raw, "raw")
    with pytest.raises(KeyError, match="ema_state_dict"):
        select_state_dict(dict(model_state_dict=raw), use_ema=True)


def test_parsers_take_the_new_flags_and_default_to_off():
    a = F.build_parser().parse_args([])
    assert a.ema_decay is None and a.ema_warmup is True
    a = F.build_parser().parse_args(["--ema-decay", "0.9999", "--no-ema-warmup"])
    assert a.ema_decay == 0.9999 and a.ema_warmup is False
    assert F.build_parser().parse_args(["--ema-decay", "0.9"]).ema_warmup is True
    assert I.build_parser().parse_args([]).ema is False
    assert I.build_parser().parse_args(["--ema"]).ema is True
