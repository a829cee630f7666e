"""Host side of the run-time-shaped kernels' parameter-range cases (tests/rt_param_range_cases.py): every fixture is
sound -- the float64 oracle's outputs and gradients are finite (apart from nonfinite_weight's column), the fp32 oracle is
within the non-stress head-room of it in every comparison the GPU test makes -- and, computed in float64, reaches the path
it is named for; the layer_spread fixtures are the base case to the fp32 oracle, bit for bit.  No GPU."""
import numpy as np
import pytest
import torch

import rt_bwd_range_cases as R
import rt_fwd_range_cases as F
import rt_param_range_cases as P
from helpers import MAX_WIDENING, normwise_err, rowwise_err


def forward_widenings(fx, ref) -> dict:
    """the head-room each of the GPU test's forward comparisons would claim"""
    out = {}
    for (label, p32, rowwise), (_, p64, _) in zip(P.y_parts(fx, ref.y32), P.y_parts(fx, ref.y64)):
        if fx.case.family == "nonfinite_weight" and not rowwise:
            continue
        out[label] = 2.0 * (rowwise_err if rowwise else normwise_err)(p32.numpy(), p64.numpy())
    out["ld"] = 2.0 * normwise_err(ref.ld32.numpy(), ref.ld64.numpy())
    return out


def gradient_widenings(fx, ref) -> dict:
    out = {}
    g32, g64 = ref.g[torch.float32], ref.g[torch.float64]
    for k, g in g64.items():
        assert g is not None and bool(torch.isfinite(g).all()), f"float64 oracle gradient {k} is not finite"
        if float(g.abs().max()) != 0.0:
            out[k] = 2.0 * normwise_err(g32[k].numpy(), g.numpy())
    for (label, p32), (_, p64) in zip(P.grad_parts(fx, g32), P.grad_parts(fx, g64)):
        out[label] = 2.0 * normwise_err(p32.numpy(), p64.numpy())
    return out


def reaches_its_path(case, fx):
    ly, fam = case.layer, case.family
    fig = P.path_figures(fx)
    if fam in P.BIG_BIAS:
        v = P.BIG_BIAS[fam]
        names = list(fx.dead) or [P.shift_head(ly, fx.sd) + ".bias"]
        assert max(float(fx.sd[n].abs().max()) for n in names) == v
        assert v / fig["weight_max"] >= v, fig["weight_max"]  # at 2^36: the ratio the derivation starts from
        assert fig["hidden_max"] < R.LIMIT
    if fam == "layer_spread":
        lo, hi = min(fig["per_linear"]), max(fig["per_linear"])
        assert lo / hi <= P.SPREAD_REACH.get(ly.tag, 2.0 ** -24), (lo, hi, np.log2(lo / hi))
        assert fig["hidden_max"] < R.LIMIT, fig["hidden_max"]
        print(f"{case.id}: per-Linear maxima 2^{np.log2(lo / hi):.1f} apart, largest hidden magnitude {fig['hidden_max']:.0f}")
    if fam == "hidden_outlier":
        assert fig["first_hidden_row_max"] >= P.OUTLIER, fig
        assert fig["first_hidden_second"] <= 2.0 ** 6, fig
    if fam == "zero_weights":
        assert fig["weight_max"] == 0.0 and any(float(v.abs().max()) > 0 for k, v in fx.sd.items() if k.endswith(".bias"))
    if fam == "nonfinite_weight":
        bad = [k for k, v in fx.sd.items() if not bool(torch.isfinite(v).all())]
        assert bad == [P.shift_head(ly, fx.sd) + ".weight"] and int((~torch.isfinite(fx.sd[bad[0]])).sum()) == 1
        assert 0.0 < fig["weight_max"] < 4.0


@pytest.mark.parametrize("case", P.FWD_CASES, ids=P.FWD_IDS)
def test_forward_case_is_sound_and_reaches_its_path(case):
    fx, ref = P.fixture(case), P.oracle(case)
    ly, fam = case.layer, case.family
    if fam == "nonfinite_weight":
        # non-finite exactly in the column the +inf feeds, in both oracles
        for y in (ref.y32, ref.y64):
            bad = ~torch.isfinite(y)
            assert bool(bad[:, fx.col].all()) and int(bad.sum()) == ly.rows
    else:
        assert bool(torch.isfinite(ref.y64).all()) and bool(torch.isfinite(ref.y32).all()), "oracle output is not finite"
    assert bool(torch.isfinite(ref.ld64).all()) and bool(torch.isfinite(ref.ld32).all())
    wide = forward_widenings(fx, ref)
    print(f"{case.id}: widening " + ", ".join(f"{k} {v:.2e}" for k, v in wide.items()))
    for k, w in wide.items():
        assert w <= MAX_WIDENING, f"{case.id}: fp32 oracle vs fp64 oracle, {k}: 2 x distance = {w:.3e} > {MAX_WIDENING:.1e}"
    reaches_its_path(case, fx)
    base = F.oracle(R.Case(ly, "base", case.inverse))
    if fam == "layer_spread":  # powers of two all the way: the same fp32 numbers
        F.same_bits(ref.y32, base.y32, f"{case.id}: fp32 oracle y, and the base case's")
        F.same_bits(ref.ld32, base.ld32, f"{case.id}: fp32 oracle ld, and the base case's")
    if fam in P.BIG_BIAS and ly.kind != "nsf":  # the float64 function of everything else is the base case's
        others = [c for c in range(ly.dim) if c != fx.col]
        assert torch.equal(ref.y64[:, others], base.y64[:, others]) and torch.equal(ref.ld64, base.ld64)
        assert float((ref.y64[:, fx.col] - base.y64[:, fx.col]).abs().min()) > 0.0
    if fam in P.BIG_BIAS and ly.kind == "nsf":
        c = ly.dim // 2 + P.NSF_DEAD_COLUMN
        assert bool(((fx.x[:, c].abs() > 4.0) & (fx.x[:, c].abs() < 5.0)).all())
        assert torch.equal(ref.y64[:, c], fx.x[:, c].double()) and torch.equal(ref.y32[:, c], fx.x[:, c])
        # dead: with the biases back at their base values the float64 outputs are the same numbers
        sd0 = {k: R.base_inputs(ly)[0][k] for k in fx.sd}
        with torch.no_grad():
            y0, ld0 = F.evaluate(case, sd0, fx.x, fx.mask, torch.float64)
        assert torch.equal(y0, ref.y64) and torch.equal(ld0, ref.ld64)


@pytest.mark.parametrize("case", P.GRAD_CASES, ids=P.GRAD_IDS)
def test_gradient_case_is_sound(case):
    fx, ref = P.fixture(case), P.grad_oracle(case)
    wide = gradient_widenings(fx, ref)
    print(f"{case.id}: widening at most {max(wide.values()):.2e} ({max(wide, key=wide.get)})")
    assert "x" in wide and len(wide) > 1
    for k, w in wide.items():
        assert w <= MAX_WIDENING, f"{case.id}: fp32 oracle vs fp64 oracle, grad {k}: 2 x distance = {w:.3e} > {MAX_WIDENING:.1e}"
    for name, idx in fx.dead.items():
        for dt in (torch.float32, torch.float64):
            assert float(ref.g[dt][name][idx].abs().max()) == 0.0
    if case.family == "zero_weights":  # the weights' own gradients are there to be compared
        assert any(k.endswith(".weight") for k in wide), wide.keys()
    for k, u in fx.zeroed.items():
        g = ref.g[torch.float64][k].abs()
        rest = [c for c in range(g.shape[1]) if c != u]
        assert float(g[:, u].max()) >= 2.0 ** 12 * float(g[:, rest].max())


def test_the_table_covers_the_issue():
    assert len(set(P.FWD_IDS)) == len(P.FWD_CASES) and len(set(P.GRAD_IDS)) == len(P.GRAD_CASES)
    assert P.GRAD_LAYERS == R.LAYERS
    assert [ly.tag for ly in P.FWD_ONLY_LAYERS] == ["ahf512", "ahf40w", "rnvp800", "nsf16"]
    assert max(ly.rows for ly in P.LAYERS) == 2100 and all(ly.rows == 300 for ly in P.FWD_ONLY_LAYERS)
    assert P.BIG_BIAS == {"big_bias_head_2p20": 2.0 ** 20, "big_bias_head_2p36": 2.0 ** 36}
    assert (P.SPREAD_F, P.SPREAD_F_ONE_HIDDEN, P.OUTLIER) == (2.0 ** 8, 2.0 ** 9, 2.0 ** 24)
    for ly in P.LAYERS:
        for d in ([""] if ly.kind == "rnvp" else ["-fwd", "-inv"]):
            for fam in P.FAMILIES:
                cid = f"{ly.tag}{d}-{fam}"
                want = not (fam == "nonfinite_weight" and ly.kind == "nsf")
                assert (cid in P.FWD_IDS) == (want and (ly.tag, fam) not in P.LEFT_OUT_FORWARD), cid
                want_g = ly in P.GRAD_LAYERS and fam != "nonfinite_weight"
                assert (cid in P.GRAD_IDS) == (want_g and (ly.tag, fam) not in P.LEFT_OUT_GRADIENT), cid
    one_hidden = {ly.tag for ly in P.LAYERS if len(ly.shape) == 1 and ly.kind != "nsf"}
    assert set(P.SPREAD_REACH) == one_hidden | {"rnvp64"} and min(P.SPREAD_REACH[t] for t in one_hidden) >= 2.0 ** -18
    assert not [k for k in P.STRESS if k.endswith("-layer_spread")]
    assert set(P.STRESS) <= set(P.FWD_IDS)
