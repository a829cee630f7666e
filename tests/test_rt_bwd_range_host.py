"""Host side of the run-time-shaped gradient kernels' operating-range cases (tests/rt_bwd_range_cases.py): every
fixture is sound -- the float64 oracle's gradients are finite, the fp32 oracle is within the non-stress head-room of it
(which also rejects a fixture on a LeakyReLU kink or a spline knot) -- and, computed in float64, reaches the kernel path
it is named for.  No GPU."""
import numpy as np
import pytest
import torch

import rt_bwd_range_cases as R
from helpers import MAX_WIDENING, normwise_err


def widenings(ref) -> dict:
    out = {}
    for k, g64 in ref.g[torch.float64].items():
        if g64 is None or float(g64.abs().max()) == 0.0:
            continue
        assert bool(torch.isfinite(g64).all()), f"float64 oracle gradient {k} is not finite"
        out[k] = 2.0 * normwise_err(ref.g[torch.float32][k].numpy(), g64.numpy())
    return out


@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_case_is_sound_and_reaches_its_path(case):
    fx, ref = R.fixture(case), R.oracle(case)
    wide = widenings(ref)
    print(f"{case.id}: widening at most {max(wide.values()):.2e} ({max(wide, key=wide.get)})")
    assert "x" in wide and len(wide) > 1
    for k, w in wide.items():
        assert w <= MAX_WIDENING, f"{case.id}: fp32 oracle vs fp64 oracle, grad {k}: 2 x distance = {w:.3e} > {MAX_WIDENING:.1e}"
    # grad_x of the ordinary rows on their own norm (what the GPU test holds the kernel to as well)
    if fx.special and fx.bad_row is None:
        keep = fx.ordinary
        w = 2.0 * normwise_err(ref.g[torch.float32]["x"][keep].numpy(), ref.g[torch.float64]["x"][keep].numpy())
        assert w <= MAX_WIDENING, f"{case.id}: grad x of the ordinary rows: widening {w:.3e}"
    fig = R.path_figures(fx)
    rows, fam = case.layer.rows, case.family
    far = R.unsampled_mask(rows)
    if fam.startswith("cot_"):
        assert fig["scale"] != 1.0 and np.log2(fig["scale"]) == int(np.log2(fig["scale"])), fig["scale"]
    if fam == "cot_small" and rows >= R.SAMPLE:
        # the unsampled rows are larger than anything the scale was taken from
        assert far.any() and float(fx.w_y[torch.from_numpy(far)].abs().max()) * fig["scale"] >= 8.0
    if fam == "cot_outlier":
        assert fig["outliers_unsampled"], fx.special
        assert fig["outlier_y"] >= R.LIMIT and fig["outlier_l"] >= R.LIMIT, fig
        # ... not only at the layer's output: the cotangents that reach the conditioner's outputs, which is what the first
        # chain step splits (a row whose transformed columns all lay beyond the spline's tail bound would lose them on
        # the way), are at or beyond 2^13 in both outlier rows and far below it in every other row
        assert fig["outlier_y_at_net"] >= R.LIMIT and fig["outlier_l_at_net"] >= R.LIMIT, fig
        assert fig["others_at_net"] < R.LIMIT / 64, fig
        # ... and nothing else is: the ordinary rows stay within the split range
        keep = fx.ordinary
        assert float(fx.w_y[keep].abs().max()) * fig["scale"] < 16.0 and float(fx.w_l[keep].abs().max()) * fig["scale"] < 16.0
    if fam == "big_cond_rows":
        assert R.straddles(fig["input_tiles"]), fig["input_tiles"].max()
        assert fig["hidden_tiles"].max() < R.LIMIT  # (the small first-layer weights bring the rows back: inputs only)
    if fam == "big_hidden":
        assert R.straddles(fig["hidden_tiles"]), (fig["hidden_tiles"].min(), fig["hidden_tiles"].max())
        assert fig["input_tiles"].max() < R.LIMIT
        print(f"{case.id}: {int((fig['hidden_tiles'] >= R.LIMIT).sum())} of {len(fig['hidden_tiles'])} tiles with a hidden "
              f"magnitude >= 2^13 (largest {fig['hidden_tiles'].max():.0f})")
    if fam == "big_act_rows":
        assert R.straddles(fig["input_tiles"])
        assert R.straddles(fig["g_s_tiles"]), fig["g_s_tiles"].max()  # g_s crosses the limit: the rescue path
    if fam == "nonfinite_row":
        assert int((~torch.isfinite(fx.x)).sum()) == 1 and not bool(torch.isfinite(fx.x[fx.bad_row]).all())
        col = int(torch.nonzero(~torch.isfinite(fx.x[fx.bad_row]))[0])
        assert R.cond_columns(case.layer).start <= col < R.cond_columns(case.layer).stop
        assert fx.mask is None or float(fx.mask[fx.bad_row, col]) == 1.0
        assert len(R.tile_neighbours(fx.bad_row, rows)) == 15


def test_the_table_covers_the_issue():
    ids = set(R.CASE_IDS)
    assert len(ids) == len(R.CASES)
    for ly in R.LAYERS:
        dirs = [""] if ly.kind == "rnvp" else ["-fwd", "-inv"]
        for d in dirs:
            for fam in R.FAMILIES:
                want = not (fam == "cot_outlier" and ly.rows < R.SAMPLE) and not (fam == "big_act_rows" and ly.kind != "ahf")
                assert (f"{ly.tag}{d}-{fam}" in ids) == want, (ly.tag, d, fam)
    # the cot_* families stay at GBASE: the scale is a power of two
    assert not [k for k in R.STRESS if "-cot_" in k]
    assert set(R.STRESS) <= ids | {R.RUN_ID}


def test_sampling_rule_and_seeded_mask():
    assert list(R.sampled_rows(300)) == list(range(300))
    assert list(R.sampled_rows(700)) == list(range(512))
    s = R.sampled_rows(2100)
    assert len(s) == 512 and s[1] == 4 and s[-1] == 2044
    for rows in (700, 2100):
        far = R.unsampled_mask(rows)
        assert all(far[r] for r in R.outlier_rows_of(rows))
    assert R.grad_scale(torch.tensor([[3.9]]), None) == 0.5 and R.grad_scale(torch.tensor([[4.0]]), None) == 0.25
    assert R.grad_scale(None, torch.tensor([1e-7])) == 2.0 ** 24 and R.grad_scale(torch.zeros(2, 2), None) == 1.0
    m = R.seeded_mask(R.RNVP_SEED, 700, 64)
    assert m.shape == (700, 64) and 0.45 < float(m.mean()) < 0.55 and set(m.unique().tolist()) == {0.0, 1.0}


def test_the_run_is_sound_and_reaches_its_paths():
    sds, x, w, special = R.run_fixture()
    ref = R.run_oracle()
    wide = widenings(ref)
    print(f"{R.RUN_ID}: widening at most {max(wide.values()):.2e} ({max(wide, key=wide.get)})")
    for k, v in wide.items():
        assert v <= MAX_WIDENING, f"{R.RUN_ID}: grad {k}: widening {v:.3e}"
    keep = torch.ones(R.RUN_ROWS, dtype=torch.bool)
    keep[list(special)] = False
    v = 2.0 * normwise_err(ref.g[torch.float32]["x"][keep].numpy(), ref.g[torch.float64]["x"][keep].numpy())
    assert v <= MAX_WIDENING, v
    # the outlier row is unsampled and its d loss / d log p reaches 2^13 in units of the sampled scale
    assert R.unsampled_mask(R.RUN_ROWS)[R.RUN_OUTLIER_ROW]
    scale = R.grad_scale(None, w)
    assert float(w[R.RUN_OUTLIER_ROW]) * scale >= R.LIMIT and float(w[keep].max()) * scale < 4.0
    assert R.straddles(R.tile_max(x[:, :R.RUN_DIM // 2]))
