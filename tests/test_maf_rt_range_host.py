"""Host side of the MAF / IAF matrix-core kernels' operating- and parameter-range cases (tests/maf_rt_range_cases.py): every
fixture is sound -- the float64 oracle's outputs and gradients are finite where they should be, the fp32 oracle lies within
MAX_WIDENING / 2 of it in every comparison the GPU test makes --, reaches in float64 the kernel path it is named for, and the
library's *_supported queries give every layer the plans the table claims.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

import maf_rt_range_cases as M
import rt_bwd_range_cases as R
from helpers import MAX_WIDENING, normwise_err, rowwise_err
from rt_fwd_range_cases import same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def forward_widenings(fx, ref) -> dict:
    """the head-room each of the GPU test's forward comparisons would claim"""
    out = {}
    for (label, p32, rowwise), (_, p64, _) in zip(M.y_parts(fx, ref.y32), M.y_parts(fx, ref.y64)):
        if fx.case.family == "nonfinite_weight" and not rowwise:
            continue
        out[label] = 2.0 * (rowwise_err if rowwise else normwise_err)(p32.numpy(), p64.numpy())
    if fx.bad_row is not None or not fx.special:
        out["ld"] = 2.0 * normwise_err(ref.ld32.numpy(), ref.ld64.numpy())
    else:
        keep, special = fx.ordinary, list(fx.special)
        out["ld (ordinary rows)"] = 2.0 * normwise_err(ref.ld32[keep].numpy(), ref.ld64[keep].numpy())
        out["ld (special rows)"] = 2.0 * normwise_err(ref.ld32[special].numpy(), ref.ld64[special].numpy())
    return out


def gradient_widenings(fx, ref) -> dict:
    out = {}
    g32, g64 = ref.g[torch.float32], ref.g[torch.float64]
    for k, g in g64.items():
        assert g is not None and bool(torch.isfinite(g).all()), f"float64 oracle gradient {k} is not finite"
        if float(g.abs().max()) != 0.0:
            out[k] = 2.0 * normwise_err(g32[k].numpy(), g.numpy())
    if fx.special and fx.bad_row is None:
        keep = fx.ordinary
        out["x (ordinary rows)"] = 2.0 * normwise_err(g32["x"][keep].numpy(), g64["x"][keep].numpy())
    for (label, p32), (_, p64) in zip(M.grad_parts(fx, g32), M.grad_parts(fx, g64)):
        out[label] = 2.0 * normwise_err(p32.numpy(), p64.numpy())
    return out


def sound_outputs(case, fx, ref):
    if case.family == "nonfinite_weight":  # non-finite exactly in the column the +inf feeds, in both oracles
        for y in (ref.y32, ref.y64):
            bad = ~torch.isfinite(y)
            assert bool(bad[:, fx.col].all()) and int(bad.sum()) == case.layer.rows
    else:
        assert bool(torch.isfinite(ref.y64).all()) and bool(torch.isfinite(ref.y32).all()), "oracle output is not finite"
    assert bool(torch.isfinite(ref.ld64).all()) and bool(torch.isfinite(ref.ld32).all())
    wide = forward_widenings(fx, ref)
    print(f"{case.id}: widening " + ", ".join(f"{k} {v:.2e}" for k, v in wide.items()))
    for k, w in wide.items():
        assert w <= MAX_WIDENING, f"{case.id}: fp32 oracle vs fp64 oracle, {k}: 2 x distance = {w:.3e} > {MAX_WIDENING:.1e}"


def special_tiles(fx, n) -> np.ndarray:
    big = np.zeros(n, dtype=bool)
    big[[r // 16 for r in fx.special]] = True
    return big


# ---------------------------------------------------------------------------------------------------- the forward table
@pytest.mark.parametrize("case", M.FWD_CASES, ids=M.FWD_IDS)
def test_forward_case_is_sound_and_reaches_its_path(case):
    fx, ref = M.fixture(case), M.oracle(case)
    ly, fam, inv, dim = case.layer, case.family, case.inverse, case.layer.dim
    sound_outputs(case, fx, ref)
    fig = M.path_figures(fx)
    if fam in ("big_rows", "big_late_elements"):
        tiles = fig["input_tiles"]
        assert ((tiles >= R.LIMIT) == special_tiles(fx, len(tiles))).all()  # the special rows' tiles, and no other
        assert fig["hidden_tiles"].max() < R.LIMIT  # (the small first-layer weights bring the rows back: inputs only)
        assert float(fx.sd["net.0.weight"].abs().max()) < 1e-3
    if fam == "big_late_elements":
        # the first half of the decode order stays at scale 1: the row's scale is 1 there and JUMPS once the first big
        # element has been decoded (maf_seq_rt retakes it at every step; maf_rt sees the whole row at once)
        late = M.late_columns(ly, inv)
        early = [c for c in range(dim) if c not in late]
        assert len(late) == dim - dim // 2 and float(fx.x[:, early].abs().max()) < 8.0
        assert sorted(M.net_index(ly, inv, c) for c in late) == list(range(dim // 2, dim))
        steps = []
        for r in fx.special:
            over = (fig["step_row_max"][r] >= R.LIMIT).nonzero()[:, 0]
            assert len(over) > 0, r
            steps.append(int(over[0]))
            assert float(fig["step_row_max"][r, dim // 2]) < 8.0  # up to and including step dim / 2: scale 1
        print(f"{case.id}: the rows' maximum over the elements decoded so far first reaches 2^13 at steps {steps} of {dim}")
        assert all(dim // 2 < s <= dim // 2 + 3 for s in steps), steps
        ordinary = fig["step_row_max"][fx.ordinary]
        assert float(ordinary.max()) < R.LIMIT
    if fam == "big_hidden":
        tiles = fig["hidden_tiles"]
        beyond = int((tiles >= R.LIMIT).sum())
        print(f"{case.id}: f = {M.BIG_HIDDEN_FACTOR[(ly.tag, inv)]:.0f}: {beyond} of {len(tiles)} tiles with a first hidden "
              f"vector >= 2^13 (largest {tiles.max():.0f})")
        assert beyond >= 2 and len(tiles) - beyond >= 2, beyond
        assert fig["input_tiles"].max() < R.LIMIT
    if fam == "big_heads":
        g = M.BIG_HEADS_GAIN[inv]
        big, base = M.head_outputs_max(fx), M.head_outputs_max(M.fixture(R.Case(ly, "base", inv)))
        print(f"{case.id}: largest conditioner output {big:.1f} (base case {base:.2f}), |y| up to "
              f"{float(ref.y64.abs().max()):.0f}, |log_det| up to {float(ref.ld64.abs().max()):.0f}")
        assert big >= 0.5 * g * base, (big, base)
    if fam == "nonfinite_row":
        bad = ~torch.isfinite(fx.x)
        assert int(bad.sum()) == 1 and bool(bad[fx.bad_row].any())
        col = int(torch.nonzero(bad[fx.bad_row])[0])
        assert M.net_index(ly, inv, col) == 1 and dim > 2  # elements 2 .. dim - 1 read it
        assert bool(M.masks_of(ly)[0][1, :].any())  # ... through a first-layer unit the mask connects it to
        assert len(R.tile_neighbours(fx.bad_row, ly.rows)) == 15
        y, ld = M.bad_row_outputs(fx)
        assert not bool(torch.isfinite(y).all()) and not bool(torch.isfinite(ld))
        if not inv:  # element 0 was decoded before the inf entered the net
            assert bool(torch.isfinite(y[0])) and not bool(torch.isfinite(y[1:]).any())
    if fam in M.INDEPENDENT:
        clean, base_x = M.base_rows(fx), M.base_inputs(ly)[1]
        assert torch.equal(clean, base_x) and not torch.equal(clean, fx.x)
        assert torch.equal(clean[fx.ordinary], fx.x[fx.ordinary])


# --------------------------------------------------------------------------------------------------- the gradient table
@pytest.mark.parametrize("case", M.GRAD_CASES, ids=M.GRAD_IDS)
def test_gradient_case_is_sound_and_reaches_its_path(case):
    fx, ref = M.fixture(case), M.grad_oracle(case)
    ly, fam = case.layer, case.family
    wide = gradient_widenings(fx, ref)
    print(f"{case.id}: widening at most {max(wide.values()):.2e} ({max(wide, key=wide.get)})")
    assert "x" in wide and len(wide) > 1
    for k, w in wide.items():
        assert w <= MAX_WIDENING, f"{case.id}: fp32 oracle vs fp64 oracle, grad {k}: 2 x distance = {w:.3e} > {MAX_WIDENING:.1e}"
    for k, gone in M.masked_out(ly).items():  # the oracle's own gradients of the masked-out entries are exactly zero
        assert int(gone.sum()) > 0
        for dt in (torch.float32, torch.float64):
            assert float(ref.g[dt][k][gone].abs().max()) == 0.0
    scale = R.grad_scale(fx.w_y, fx.w_l)
    if fam == "cot_small":
        assert scale >= 2.0 ** 20
        far = R.unsampled_mask(ly.rows)
        if far.any():  # rows beyond the sample larger than anything in it
            assert float(fx.w_y[torch.from_numpy(far)].abs().max()) * scale >= 16.0
    if fam == "cot_large":
        assert scale <= 2.0 ** -6
    if fam == "cot_outlier":
        r_y, r_l = fx.special
        far = R.unsampled_mask(ly.rows)
        assert far[r_y] and far[r_l]
        assert float(fx.w_y[r_y].abs().max()) * scale >= R.LIMIT and abs(float(fx.w_l[r_l])) * scale >= R.LIMIT
    if fam == "cot_y_only":
        assert fx.w_l is None and fx.w_y is not None
    if fam == "cot_ld_only":
        assert fx.w_y is None and fx.w_l is not None
    if fam in ("big_rows", "big_hidden", "nonfinite_row"):  # the forward table's fixture, not a copy of it
        assert fx is M.fixture(R.Case(ly, fam, case.inverse)) and R.Case(ly, fam, case.inverse) in M.FWD_CASES


# -------------------------------------------------------------------------------------------------- the parameter table
def reaches_its_path(case, fx):
    ly, fam, dim = case.layer, case.family, case.layer.dim
    fig = M.path_figures(fx)
    last = M.last_linear(ly)
    if fam in M.BIG_BIAS:
        v, j = M.BIG_BIAS[fam], M.mid_element(ly)
        assert float(fx.sd[f"{last}.bias"].abs().max()) == v == float(fx.sd[f"{last}.bias"][dim + j])
        assert 0 < j < dim - 1 and float(fx.sd["net.0.weight"][:, j].abs().max()) == 0.0
        assert 0.0 < fig["weight_max"] < 4.0 and fig["hidden_tiles"].max() < R.LIMIT
        assert fx.col == M.y_column(ly, case.inverse, j)
    if fam == "layer_spread":
        lo, hi = min(fig["per_linear"]), max(fig["per_linear"])
        assert lo / hi <= M.SPREAD_REACH.get(ly.tag, 2.0 ** -24), (lo, hi, np.log2(lo / hi))
        assert fig["hidden_tiles"].max() < R.LIMIT
        print(f"{case.id}: per-MaskedLinear unmasked maxima 2^{np.log2(lo / hi):.2f} apart, largest first hidden magnitude "
              f"{fig['hidden_tiles'].max():.0f}")
    if fam == "hidden_outlier":
        u, m = fx.unit, M.masks_of(ly)
        assert bool(m[0][:, u].any()) and bool(m[1][u, :].any())  # not vacuous: the unit has inputs and is read
        assert fig["first_hidden_row_max"] >= M.HIDDEN_OUTLIER and fig["first_hidden_second"] <= 2.0 ** 6, fig
    if fam == "zero_weights":
        assert fig["weight_max"] == 0.0 and all(float(fx.sd[k].abs().max()) == 0.0 for k in M.weight_names(ly))
        assert any(float(v.abs().max()) > 0 for k, v in fx.sd.items() if k.endswith(".bias"))
    if fam == "nonfinite_weight":
        bad = [k for k, v in fx.sd.items() if not bool(torch.isfinite(v).all())]
        assert bad == [f"{last}.weight"] and int((~torch.isfinite(fx.sd[bad[0]])).sum()) == 1
        where = (~torch.isfinite(fx.sd[bad[0]])).nonzero()[0]
        assert int(where[0]) == 2 * dim - 1 and not bool(M.masked_out(ly)[bad[0]][where[0], where[1]])  # t head, unmasked
        assert 0.0 < fig["weight_max"] < 4.0
    if fam == "masked_giant":
        base = M.path_figures(M.fixture(R.Case(ly, "base", case.inverse)))
        assert fig["per_linear"] == base["per_linear"]  # the largest unmasked weights stay where they were
        for k, gone in M.masked_out(ly).items():
            assert bool((fx.sd[k][gone] == M.GIANT).all()) and int(gone.sum()) > 0
            assert float(M.zeros_parked(fx)[k][gone].abs().max()) == 0.0


@pytest.mark.parametrize("case", M.PARAM_FWD_CASES, ids=M.PARAM_FWD_IDS)
def test_parameter_forward_case_is_sound_and_reaches_its_path(case):
    fx, ref = M.fixture(case), M.oracle(case)
    ly, fam = case.layer, case.family
    sound_outputs(case, fx, ref)
    reaches_its_path(case, fx)
    base = M.oracle(R.Case(ly, "base", case.inverse))
    if fam in ("layer_spread", "masked_giant"):  # powers of two all the way / exact zeros: the same fp32 numbers
        same_bits(ref.y32, base.y32, f"{case.id}: fp32 oracle y, and the base case's")
        same_bits(ref.ld32, base.ld32, f"{case.id}: fp32 oracle ld, and the base case's")
    if fam == "nonfinite_weight":  # every other column and log_det: the base case's
        others = [c for c in range(ly.dim) if c != fx.col]
        assert torch.equal(ref.y64[:, others], base.y64[:, others]) and torch.equal(ref.ld64, base.ld64)


@pytest.mark.parametrize("case", M.PARAM_GRAD_CASES, ids=M.PARAM_GRAD_IDS)
def test_parameter_gradient_case_is_sound(case):
    fx, ref = M.fixture(case), M.grad_oracle(case)
    wide = gradient_widenings(fx, ref)
    print(f"{case.id}: widening at most {max(wide.values()):.2e} ({max(wide, key=wide.get)})")
    assert "x" in wide and len(wide) > 1
    for k, w in wide.items():
        assert w <= MAX_WIDENING, f"{case.id}: fp32 oracle vs fp64 oracle, grad {k}: 2 x distance = {w:.3e} > {MAX_WIDENING:.1e}"
    if case.family == "zero_weights":  # the weights' own gradients are there to be compared
        assert any(k.endswith(".weight") for k in wide), wide.keys()
    for k, u in fx.zeroed.items():
        g = ref.g[torch.float64][k].abs()
        rest = [c for c in range(g.shape[1]) if c != u]
        assert float(g[:, u].max()) >= 2.0 ** 12 * float(g[:, rest].max())


# ------------------------------------------------------------------------------------------ the plans, and the tables' shape
@pytest.fixture(scope="module")
def lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as entry
    import torch_mnf_amd

    if not os.path.exists(torch_mnf_amd.library_path()):
        entry.build()
    return torch_mnf_amd._lib.load()


def net_bytes(ly) -> int:
    """the converted net as csrc/mnf_maf_rt.hip stages it: blocks of 2 KB, one per (32-column K-step, 16-unit output tile);
    the last MaskedLinear as s and t tiles of their own"""
    widths = (ly.dim, *ly.shape)
    blocks = sum(-(-a // 32) * -(-b // 16) for a, b in zip(widths, widths[1:]))
    blocks += -(-widths[-1] // 32) * 2 * -(-ly.dim // 16)
    return 2048 * blocks


@pytest.mark.parametrize("ly", M.LAYERS, ids=[ly.tag for ly in M.LAYERS])
def test_the_layers_have_the_plans_the_table_claims(lib, ly):
    from torch_mnf_amd._lib import int_array

    args = (ly.dim, len(ly.shape), int_array(list(ly.shape)))
    got = {"maf_rt": lib.mnf_maf_rt_supported(*args), "maf_seq_rt": lib.mnf_maf_seq_rt_supported(*args),
           "maf_bwd_rt": lib.mnf_maf_bwd_rt_supported(*args), "maf_seq_bwd_rt": lib.mnf_maf_seq_bwd_rt_supported(*args)}
    assert {k for k, v in got.items() if v == 1} == set(ly.kernels), got
    # maf_rt: resident or streaming.  maf_seq_rt has resident plans only (its query is maf_rt's plan AND resident AND the
    # waves' slabs fit); a net beyond the 150 KB the one-pass launcher keeps for a resident image is streamed
    if ly.streaming:
        assert got["maf_rt"] == 1 and got["maf_seq_rt"] == 0 and net_bytes(ly) > 150 * 1024, net_bytes(ly)
    else:
        assert got["maf_seq_rt"] == 1 and net_bytes(ly) <= 150 * 1024, net_bytes(ly)


def test_the_tables_cover_the_issue():
    assert [(ly.tag, ly.dim, ly.shape, ly.parity, ly.rows) for ly in M.LAYERS] == [
        ("maf6", 6, (16, 16), False, 700), ("maf37", 37, (20, 7, 33), True, 300), ("maf64", 64, (24, 24, 24), False, 300),
        ("maf40", 40, (64,), True, 300), ("maf40w", 40, (128,), True, 300), ("maf130s", 130, (128, 128), False, 300)]
    assert [ly.tag for ly in M.GRAD_LAYERS] == ["maf6", "maf37", "maf64", "maf40"]
    assert [ly.tag for ly in M.PARAM_LAYERS] == ["maf6", "maf37", "maf64", "maf40", "maf130s"]
    for ids, cases in ((M.FWD_IDS, M.FWD_CASES), (M.GRAD_IDS, M.GRAD_CASES), (M.PARAM_FWD_IDS, M.PARAM_FWD_CASES),
                       (M.PARAM_GRAD_IDS, M.PARAM_GRAD_CASES)):
        assert len(set(ids)) == len(cases)
    # the forward table: every family, both directions, unless the layer lacks the plan
    for ly in M.LAYERS:
        for d, inv, k in (("-inv", True, "maf_rt"), ("-fwd", False, "maf_seq_rt")):
            for fam in M.FWD_FAMILIES:
                assert (f"{ly.tag}{d}-{fam}" in M.FWD_IDS) == (k in ly.kernels and (ly.tag, inv, fam) not in M.LEFT_OUT_FORWARD)
        for d, inv, k in (("-inv", True, "maf_bwd_rt"), ("-fwd", False, "maf_seq_bwd_rt")):
            for fam in M.GRAD_FAMILIES:
                want = k in ly.kernels and (fam != "cot_outlier" or ly.rows > R.SAMPLE)
                assert (f"{ly.tag}{d}-{fam}" in M.GRAD_IDS) == (want and (ly.tag, inv, fam) not in M.LEFT_OUT_GRADIENT)
            for fam in M.PARAM_FAMILIES:
                fwd_k = "maf_rt" if inv else "maf_seq_rt"
                want = ly in M.PARAM_LAYERS and fwd_k in ly.kernels and (fam not in M.BIG_BIAS or fam in M.big_bias_families(inv, False))
                assert (f"{ly.tag}{d}-{fam}" in M.PARAM_FWD_IDS) == (want and (ly.tag, inv, fam) not in M.LEFT_OUT_PARAM_FORWARD)
                want_g = k in ly.kernels and fam != "nonfinite_weight" and (fam not in M.BIG_BIAS or fam in M.big_bias_families(inv, True))
                assert (f"{ly.tag}{d}-{fam}" in M.PARAM_GRAD_IDS) == (want_g and (ly.tag, inv, fam) not in M.LEFT_OUT_PARAM_GRADIENT)
    assert (len(M.FWD_CASES), len(M.GRAD_CASES), len(M.PARAM_FWD_CASES), len(M.PARAM_GRAD_CASES)) == (66, 58, 63, 48)
    assert "maf6-inv-cot_outlier" in M.GRAD_IDS and "maf6-fwd-cot_outlier" in M.GRAD_IDS
    assert M.BIG_BIAS == {"big_bias_head_2p20": 2.0 ** 20, "big_bias_head_2p21": 2.0 ** 21, "big_bias_head_2p24": 2.0 ** 24,
                          "big_bias_head_2p36": 2.0 ** 36}
    assert M.big_bias_families(True, False) == M.big_bias_families(True, True) == ("big_bias_head_2p20", "big_bias_head_2p36")
    # the element-by-element direction feeds y_j back: the row envelope (see the table's remark)
    assert M.big_bias_families(False, False) == ("big_bias_head_2p20", "big_bias_head_2p24")
    assert M.big_bias_families(False, True) == ("big_bias_head_2p20", "big_bias_head_2p21")
    assert (M.SPREAD_F, M.SPREAD_F_ONE_HIDDEN, M.HIDDEN_OUTLIER, M.GIANT) == (2.0 ** 8, 2.0 ** 9, 2.0 ** 24, 2.0 ** 40)
    assert M.BIG_HEADS_GAIN == {True: 16.0, False: 4.0}
    assert set(M.BIG_HIDDEN_FACTOR) == {(ly.tag, inv) for ly in M.LAYERS for inv in M.directions(ly)}
    # STRESS and LEFT_OUT_*: at most 5 % of each table, and never from the families whose float64 function is the base
    # case's or whose inputs are of scale 1
    never = ("-base", "-cot_small", "-cot_large", "-cot_outlier", "-cot_y_only", "-cot_ld_only", "-layer_spread",
             "-zero_weights", "-masked_giant")
    tables = {"fwd": (M.FWD_IDS, M.LEFT_OUT_FORWARD), "grad": (M.GRAD_IDS, M.LEFT_OUT_GRADIENT),
              "param-fwd": (M.PARAM_FWD_IDS, M.LEFT_OUT_PARAM_FORWARD), "param-grad": (M.PARAM_GRAD_IDS, M.LEFT_OUT_PARAM_GRADIENT)}
    assert all(k.split(" ")[0] in tables and k.split(" ")[1] in tables[k.split(" ")[0]][0] for k in M.STRESS), M.STRESS
    assert not [k for k in M.STRESS if k.endswith(never)]
    for name, (ids, left) in tables.items():
        assert not [k for k in left if ("-" + k[2]) in never], left
        out = len(left) + len([k for k in M.STRESS if k.startswith(name + " ")])
        assert out <= 0.05 * (len(ids) + len(left)), (name, out)
    # the children under MNF_DETERMINISTIC=1 run these
    for inv in (True, False):
        assert [c.family for c in M.deterministic_cases(M.DETERMINISTIC_LAYER, inv)] == ["cot_small", "cot_outlier", "big_rows"]
