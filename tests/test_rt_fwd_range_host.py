"""Host side of the run-time-shaped forward kernels' operating-range cases (tests/rt_fwd_range_cases.py): every fixture is
sound -- the float64 oracle's outputs are finite (apart from the row with the non-finite input), the fp32 oracle is within
the non-stress head-room of it row by row -- and, computed in float64, reaches the kernel path it is named for.  No GPU."""
import numpy as np
import pytest
import torch

import rt_bwd_range_cases as R
import rt_fwd_range_cases as F
from helpers import MAX_WIDENING, normwise_err, rowwise_err


def widenings(fx, ref) -> dict:
    """the head-room each of the GPU test's comparisons would claim"""
    keep = fx.ordinary
    out = {"y": 2.0 * rowwise_err(ref.y32.numpy(), ref.y64.numpy())}
    if fx.bad_row is not None or not fx.special:
        out["ld"] = 2.0 * normwise_err(ref.ld32.numpy(), ref.ld64.numpy())
    else:
        special = list(fx.special)
        out["ld (ordinary rows)"] = 2.0 * normwise_err(ref.ld32[keep].numpy(), ref.ld64[keep].numpy())
        out["ld (special rows)"] = 2.0 * normwise_err(ref.ld32[special].numpy(), ref.ld64[special].numpy())
    return out


@pytest.mark.parametrize("case", F.CASES, ids=F.CASE_IDS)
def test_case_is_sound_and_reaches_its_path(case):
    fx, ref = F.fixture(case), F.oracle(case)
    ly, fam, rows = case.layer, case.family, case.layer.rows
    assert bool(torch.isfinite(ref.y64).all()) and bool(torch.isfinite(ref.ld64).all()), "float64 oracle output is not finite"
    assert bool(torch.isfinite(ref.y32).all()) and bool(torch.isfinite(ref.ld32).all()), "fp32 oracle output is not finite"
    wide = widenings(fx, ref)
    print(f"{case.id}: widening " + ", ".join(f"{k} {v:.2e}" for k, v in wide.items()))
    for k, w in wide.items():
        assert w <= MAX_WIDENING, f"{case.id}: fp32 oracle vs fp64 oracle, {k}: 2 x distance = {w:.3e} > {MAX_WIDENING:.1e}"
    if fam in ("big_cond_rows", "big_second_rows"):
        fig = F.path_figures(fx)
        net = {"ahf": "s_net", "rnvp": "net", "nsf": "f1" if fam == "big_cond_rows" else "f2"}[ly.kind]
        tiles = fig["input_tiles"][net]
        assert R.straddles(tiles), tiles.max()
        big = np.zeros(len(tiles), dtype=bool)
        big[[r // 16 for r in fx.special]] = True
        assert ((tiles >= R.LIMIT) == big).all()  # the special rows' tiles, and no other
        assert fig["hidden_all"].max() < R.LIMIT  # (the small first-layer weights bring the rows back: inputs only)
    if fam == "big_act_rows":
        assert R.straddles(R.tile_max(fx.x[:, R.act_columns(ly)]))
        assert R.tile_max(fx.x[:, R.cond_columns(ly)]).max() < R.LIMIT
    if fam == "big_hidden":
        fig = F.path_figures(fx)
        beyond = int((fig["hidden_all"] >= R.LIMIT).sum())
        print(f"{case.id}: {beyond} of {len(fig['hidden_all'])} tiles with a hidden magnitude >= 2^13 "
              f"(largest {fig['hidden_all'].max():.0f})")
        if ly in F.FWD_LAYERS:
            assert beyond >= 3 and len(fig["hidden_all"]) - beyond >= 3, beyond
        else:
            assert R.straddles(fig["hidden_all"])
        assert fig["input_all"].max() < R.LIMIT
    if fam == "big_heads":
        g = F.BIG_HEADS_GAIN[ly.tag]
        big, base = F.conditioner_outputs_max(fx), F.conditioner_outputs_max(F.fixture(R.Case(ly, "base", case.inverse)))
        print(f"{case.id}: largest conditioner output {big:.1f} (base case {base:.2f})")
        assert big >= 0.5 * g * base, (big, base)
    if fam == "nonfinite_row":
        assert int((~torch.isfinite(fx.x)).sum()) == 1 and not bool(torch.isfinite(fx.x[fx.bad_row]).all())
        col = int(torch.nonzero(~torch.isfinite(fx.x[fx.bad_row]))[0])
        assert R.cond_columns(ly).start <= col < R.cond_columns(ly).stop
        assert fx.mask is None or float(fx.mask[fx.bad_row, col]) == 1.0
        assert len(R.tile_neighbours(fx.bad_row, rows)) == 15
        fin = F.bad_row_finite(fx)
        assert not bool(fin.all()) and not bool(fin[col])
        if ly.kind == "nsf":  # each half has an element inside [-B, B]: log_det of the row is NaN in both directions
            h = ly.dim // 2
            inside = fx.x[fx.bad_row].abs() <= F.TAIL
            assert bool(inside[:h].any()) and bool(inside[h:].any())
    if fam in F.INDEPENDENT:
        clean, base_x = F.base_rows(fx), R.base_inputs(ly)[1]
        assert torch.equal(clean, base_x) and not torch.equal(clean, fx.x)
        assert torch.equal(clean[fx.ordinary], fx.x[fx.ordinary])
    if ly.kind == "nsf":  # the pass-through check has elements to look at
        assert bool((fx.x.abs() > F.TAIL).any())


def test_the_table_covers_the_issue():
    ids = set(F.CASE_IDS)
    assert len(ids) == len(F.CASES) == 116
    assert [ly.tag for ly in F.LAYERS[:6]] == [ly.tag for ly in R.LAYERS] and F.LAYERS[:6] == R.LAYERS
    assert [ly.tag for ly in F.FWD_LAYERS] == ["ahf512", "ahf128", "ahf40w", "rnvp800", "rnvp130", "nsf16"]
    assert all(ly.rows == 300 for ly in F.FWD_LAYERS)
    for ly in F.LAYERS:
        for d in ([""] if ly.kind == "rnvp" else ["-fwd", "-inv"]):
            for fam in F.FAMILIES:
                want = {"big_act_rows": ly.kind == "ahf", "big_second_rows": ly.kind == "nsf"}.get(fam, True)
                assert (f"{ly.tag}{d}-{fam}" in ids) == want, (ly.tag, d, fam)
        assert ly.tag in F.BIG_HIDDEN_FACTOR and ly.tag in F.BIG_HEADS_GAIN
    for tag, f in R.BIG_HIDDEN_FACTOR.items():
        assert F.BIG_HIDDEN_FACTOR[tag] == f
    for ly in F.LAYERS:
        g = 16.0 if ly.tag in ("ahf64", "ahf10", "ahf512") or ly.kind == "rnvp" else 4.0
        assert F.BIG_HEADS_GAIN[ly.tag] == g
    # the shared families are the gradient table's fixtures, not copies of them
    for ly in F.LAYERS[:6]:
        for fam in ("big_cond_rows", "big_hidden", "nonfinite_row"):
            assert F.fixture(R.Case(ly, fam, False)) is R.fixture(R.Case(ly, fam, False))
    never = ("-base", "-big_cond_rows", "-big_second_rows", "-big_hidden")
    assert not [k for k in F.STRESS if k.endswith(never)]
    assert set(F.STRESS) <= ids | {F.STACK_ID}


def test_the_stack_is_sound_and_reaches_its_paths():
    sds, x, big = F.stack_inputs()
    ref = F.stack_oracle()
    (z32, ld32, lp32), (z64, ld64, lp64) = ref[torch.float32], ref[torch.float64]
    keep = torch.ones(R.RUN_ROWS, dtype=torch.bool)
    keep[list(big)] = False
    special = list(big)
    assert len(z64) == len(sds) + 1
    for k in range(1, len(z64)):
        assert bool(torch.isfinite(z64[k]).all())
        w = 2.0 * rowwise_err(z32[k].numpy(), z64[k].numpy())
        assert w <= MAX_WIDENING, (k, w)
    for name, a, b in (("ld", ld32, ld64), ("log_prob", lp32, lp64)):
        for rows in (keep, special):
            assert bool(torch.isfinite(b[rows]).all())
            w = 2.0 * normwise_err(a[rows].numpy(), b[rows].numpy())
            assert w <= MAX_WIDENING, (name, w)
    # rows beyond 2^13 reach the conditioner of the first layer the inverse pass meets and the transformed half of the next
    assert R.straddles(R.tile_max(x[:, :R.RUN_DIM // 2]))
    assert R.straddles(R.tile_max(z64[1][:, :R.RUN_DIM // 2])) and R.straddles(R.tile_max(z64[2][:, :R.RUN_DIM // 2]))


def test_row_parity_rule():
    """helpers.assert_row_parity: each row on its own maximum; non-finite reference rows left out, pattern held."""
    from helpers import PARITY_LOG, assert_parity, assert_row_parity

    ref = np.array([[1.0, 2.0], [1e5, -3e5], [1e-3, 4e-3]])
    got = ref.copy()
    got[2, 0] += 4e-8  # 1e-5 of ITS row's maximum; 1.3e-13 of the tensor's
    n = len(PARITY_LOG)
    assert assert_parity(got, ref, what="rule") < 1e-12
    assert abs(assert_row_parity(got, ref, what="rule") - 1e-5) < 1e-9
    got[2, 0] += 4e-8
    with pytest.raises(AssertionError, match="row-wise error"):
        assert_row_parity(got, ref, what="rule")
    ref64 = ref.copy()
    ref64[0, 1] += 2e-5  # the references differ by 1e-5 of row 0: budget 1e-5 + 2e-5
    assert_row_parity(got, ref, ref64, what="rule")
    assert abs(PARITY_LOG[-1]["budget"] - 3e-5) < 1e-9 and PARITY_LOG[-1]["widening_share"] > 0.6
    ref64[0, 1] += 4e-5
    with pytest.raises(AssertionError, match="head-room"):
        assert_row_parity(got, ref, ref64, what="rule")
    assert_row_parity(got, ref, ref64, what="rule", max_widening=None)
    assert PARITY_LOG[-1]["stress"]
    bad_ref, bad_got = ref.copy(), ref.copy()
    bad_ref[1, 0] = np.nan
    with pytest.raises(AssertionError, match="pattern"):
        assert_row_parity(bad_got, bad_ref, what="rule")
    bad_got[1, 1] = np.inf
    assert assert_row_parity(bad_got, bad_ref, what="rule") == 0.0
    del PARITY_LOG[n:]  # (a CPU session has no audit; keep the log as it was all the same)
