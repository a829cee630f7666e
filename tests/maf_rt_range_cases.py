"""The operating and the parameter range of the MAF / IAF matrix-core kernels (maf_rt, maf_seq_rt, maf_bwd_rt and
maf_seq_bwd_rt = the solve kernel plus a maf_bwd_rt launch at x := y): the layer table, the three case tables, the
fixtures, the oracles and the runners.  Not collected: tests/test_maf_rt_range_host.py (CPU: every fixture is sound, reaches
the path it is named for, and the layer has the plan the table claims), tests/test_hip_maf_rt_range.py (GPU),
tests/maf_rt_deterministic_child.py / maf_seq_bwd_rt_deterministic_child.py (MNF_DETERMINISTIC=1) and
tools/maf_rt_range_table.py import it, so that all look at the same inputs.

Structure, vocabulary and comparison rules are those of tests/rt_bwd_range_cases.py, rt_fwd_range_cases.py and
rt_param_range_cases.py (AffineHalfFlow, NSF_CL, RNVP), whose helpers are used here and not copied.  What those tables do
not vouch for: the MAF kernels mask the weights in the scan and in the staging, use ReLU, read EVERY column as conditioner
input and transform it too, and the element-by-element direction feeds its own outputs back dim times.  The code that
inputs and weights of scale 1 never execute:

  first_layer    the per-row power-of-two down-scale; maf_seq_rt takes it again at every decode step (the row's maximum
                 over the columns decoded so far changes)                                    big_rows, big_late_elements
  finish_layer   the second split of a hidden vector at or beyond 2^13 (h.up[t]), used again in out_tile and in the next
                 layer's scale                                                               big_hidden, hidden_outlier
  weights        weight_exponent over the MASKED maximum, Source::wdown / wup, the turned blocks of the gradient kernels
                                                         layer_spread, zero_weights, masked_giant, big_bias_head, big_heads
  maf_bwd_rt     two exchange scales per round (d s carries the factor x e^s), the rescue of the chain accumulators, the
                 sampled gradient scale (512 rows)                                           cot_*, big_rows (gradients)
  the solve      split_rows_both scales rows up as well as down                              cot_small, cot_outlier
  exp            on conditioner outputs far from scale 1                                     big_heads

Directions: a case with inverse = True ("-inv") is the ONE-PASS direction MAF.inverse (maf_rt / maf_bwd_rt), one with
inverse = False ("-fwd") the ELEMENT-BY-ELEMENT direction MAF.forward (maf_seq_rt / maf_seq_bwd_rt).  The net's input index
i of column c: the one-pass direction reads x as it is (i = c; a parity layer flips y); the element-by-element direction
flips x first when parity (i = dim - 1 - c) and returns the decoded elements in net order."""
from __future__ import annotations

import functools
import time
from dataclasses import dataclass, field

import numpy as np
import torch

import recipes
import rt_bwd_range_cases as R
import rt_fwd_range_cases as F
import rt_param_range_cases as P
from oracle import flow_oracle as O
from rt_bwd_range_cases import (BAD_ROW, BIG_ROWS, DEV, GBASE, LIMIT, OUTLIER, SAMPLE, Case, Fixture, OracleGrads,
                                big_rows_of, check_vs_float64, scaled, tile_max, tile_neighbours, unsampled_mask)
from rt_fwd_range_cases import Outputs, same_bits

FWD_KERNELS = ("maf_rt", "maf_seq_rt")
ALL_FOUR = ("maf_rt", "maf_seq_rt", "maf_bwd_rt", "maf_seq_bwd_rt")


@dataclass(frozen=True)
class Layer(R.Layer):
    kernels: tuple = ALL_FOUR
    streaming: bool = False  # maf_rt's plan: weights streamed through LDS (else resident)


def _layer(tag, dim, hidden, parity, rows=300, kernels=ALL_FOUR, streaming=False) -> Layer:
    return Layer(tag, "maf", dim, tuple(hidden), rows, parity=parity, kernels=kernels, streaming=streaming)


# 300 rows: 19 tiles of 16, the last one ragged.  maf6: 700 rows, so that cot_outlier has rows beyond the 512-row sample
LAYERS = [
    _layer("maf6", 6, (16, 16), False, rows=700),          # the element-wise row path
    _layer("maf37", 37, (20, 7, 33), True),                # odd everywhere, partial tiles, flipped unaligned rows
    _layer("maf64", 64, (24, 24, 24), False),              # dwordx4 rows, two first-layer K-steps
    _layer("maf40", 40, (64,), True),                      # one hidden layer, the widest gradient class, vec + flip
    _layer("maf40w", 40, (128,), True, kernels=FWD_KERNELS),                      # the widest forward width
    _layer("maf130s", 130, (128, 128), False, kernels=("maf_rt",), streaming=True),  # streamed weights
]
BY_TAG = {ly.tag: ly for ly in LAYERS}
GRAD_LAYERS = [ly for ly in LAYERS if "maf_bwd_rt" in ly.kernels]
PARAM_LAYERS = GRAD_LAYERS + [BY_TAG["maf130s"]]


def kernel_of(case: Case, gradient: bool = False, force_generic: int = 2) -> str:
    if force_generic != 2:
        return "maf_bwd_generic" if gradient else "maf_generic"
    return {(True, False): "maf_rt", (False, False): "maf_seq_rt", (True, True): "maf_bwd_rt",
            (False, True): "maf_seq_bwd_rt"}[(case.inverse, gradient)]


def has(ly: Layer, inverse: bool, gradient: bool = False) -> bool:
    return kernel_of(Case(ly, "base", inverse), gradient) in ly.kernels


def directions(ly: Layer, gradient: bool = False) -> list[bool]:
    """inverse flags of the directions the layer has the plan for: one-pass (True) first"""
    return [inv for inv in (True, False) if has(ly, inv, gradient)]


# big_hidden: net.0.weight x f, net.2.weight / f -- per layer AND direction (the element-by-element direction's hidden
# vectors come from its own decoded outputs).  4500 is the AffineHalfFlow table's figure and the starting point; it is
# kept wherever at least 2 of the tiles have a first hidden vector at or beyond 2^13 and at least 2 lie below
# (tests/test_maf_rt_range_host.py holds every entry to that and prints the counts).
BIG_HIDDEN_FACTOR = {(ly.tag, inv): 4500.0 for ly in LAYERS for inv in directions(ly)}
# (40, (128,)) element by element: 128 units and the decoded outputs' wider spread put 18 of 19 tiles beyond 2^13 at 4500
BIG_HIDDEN_FACTOR[("maf40w", False)] = 3800.0

# big_heads: the last MaskedLinear (weight and bias) x g.  One-pass: 16 (|y| up to ~760, |log_det| up to ~29).
# Element-by-element: the outputs are fed back, and 16 makes the fp32 ORACLE non-finite for (40, (64,)), 8 for (40, (128,)):
# 4 there.
BIG_HEADS_GAIN = {True: 16.0, False: 4.0}

FWD_FAMILIES = ["base", "big_rows", "big_late_elements", "big_hidden", "big_heads", "nonfinite_row"]
INDEPENDENT = ("big_rows", "big_late_elements", "nonfinite_row")  # the special rows change no other row, bit for bit
GRAD_FAMILIES = ["cot_small", "cot_large", "cot_outlier", "cot_y_only", "cot_ld_only", "big_rows", "big_hidden",
                 "nonfinite_row"]
# big_bias_head: 2^20 and 2^36 on one bias entry of the t head, as rt_param_range_cases.BIG_BIAS.  The element-by-element
# direction DECODES y_j = (z_j - t_j) e^{-s_j} into the row the net reads next: the row then holds an element of that
# magnitude A, and first_layer's one power-of-two scale per row leaves its neighbours v at A 2^-49 / |v| relative
# (csrc/mnf_rt.h, DESIGN.md 3.8: fp32 grade up to A ~ 2^25, 1e-5 at ~2^32) whatever the weights of that column are; its
# gradient pass (maf_bwd_rt at x := y) has d s_j = C_j y_j e^{s_j} of that magnitude in an exchange tile with ONE scale per
# head and wave-tile.  2^36 is beyond that envelope (measured, profiles/r24/maf_rt_range.txt: y 1.2e-5 .. 4.7e-5 row-wise,
# gradients 1.6e-2 .. 1.7e-1; the fp32 VALU kernels at most 11 % of any budget), and so is 2^24 for the gradients (forward at
# most 8 % of the budget, grad net.0.weight 2.5e-5 .. 6.0e-5).  That direction takes the magnitudes inside the envelope:
# 2^24 forward, 2^21 for the gradients (2^22: up to 89 % of the budget); the one-pass direction, which reads x and only writes y_j, keeps 2^36.
BIG_BIAS = {**P.BIG_BIAS, "big_bias_head_2p21": 2.0 ** 21, "big_bias_head_2p24": 2.0 ** 24}
BIG_BIAS_ONE_PASS = ("big_bias_head_2p20", "big_bias_head_2p36")
BIG_BIAS_SEQUENTIAL = ("big_bias_head_2p20", "big_bias_head_2p24")
BIG_BIAS_SEQUENTIAL_GRADIENT = ("big_bias_head_2p20", "big_bias_head_2p21")


def big_bias_families(inverse: bool, gradient: bool) -> tuple:
    return BIG_BIAS_ONE_PASS if inverse else (BIG_BIAS_SEQUENTIAL_GRADIENT if gradient else BIG_BIAS_SEQUENTIAL)


SPREAD_F, SPREAD_F_ONE_HIDDEN = P.SPREAD_F, P.SPREAD_F_ONE_HIDDEN
# layer_spread: min / max of the per-MaskedLinear UNMASKED maxima a fixture must reach: 2^-24, except where the stated
# factors cannot give it.  The factors ARE 2^24 apart; (64, (24, 24, 24)) and (130, (128, 128)) fall short by the ratio of
# the base case's own maxima of the two MaskedLinears concerned (under 7 %); one hidden layer has two MaskedLinears to move
# apart, by f^2 = 2^18 (the hidden vector has to stay below 2^13).
SPREAD_REACH = {"maf64": 2.0 ** -23.9, "maf130s": 2.0 ** -23.9, "maf40": 2.0 ** -18}
HIDDEN_OUTLIER = P.OUTLIER  # 2^24
DETERMINISTIC_LAYER = "maf6"  # its gradient cases run under MNF_DETERMINISTIC=1 too (the only layer with cot_outlier)
GIANT = 2.0 ** 40
PARAM_FAMILIES = ["big_bias_head_2p20", "big_bias_head_2p21", "big_bias_head_2p24", "big_bias_head_2p36", "layer_spread", "hidden_outlier", "zero_weights", "nonfinite_weight", "masked_giant"]
PARAM_GRAD_FAMILIES = [f for f in PARAM_FAMILIES if f != "nonfinite_weight"]

# Cases whose fp32 ORACLE is further than MAX_WIDENING / 2 from the float64 oracle at the stated magnitude: (tag,
# direction, family) -> the figure; they leave the family, the cap is never raised.  Empty: the host test holds every case
# of the three tables to the cap.
LEFT_OUT_FORWARD: dict[tuple, str] = {}
LEFT_OUT_GRADIENT: dict[tuple, str] = {}
LEFT_OUT_PARAM_FORWARD: dict[tuple, str] = {}
LEFT_OUT_PARAM_GRADIENT: dict[tuple, str] = {}


def _table(layers, families, gradient, left_out) -> list[Case]:
    out = []
    for ly in layers:
        for inv in directions(ly, gradient):
            for fam in families:
                if fam == "cot_outlier" and ly.rows < SAMPLE:  # every row is sampled
                    continue
                if fam in BIG_BIAS and fam not in big_bias_families(inv, gradient):
                    continue
                if (ly.tag, inv, fam) not in left_out:
                    out.append(Case(ly, fam, inv))
    return out


FWD_CASES = _table(LAYERS, FWD_FAMILIES, False, LEFT_OUT_FORWARD)
GRAD_CASES = _table(GRAD_LAYERS, GRAD_FAMILIES, True, LEFT_OUT_GRADIENT)
PARAM_FWD_CASES = _table(PARAM_LAYERS, PARAM_FAMILIES, False, LEFT_OUT_PARAM_FORWARD)
PARAM_GRAD_CASES = _table(GRAD_LAYERS, PARAM_GRAD_FAMILIES, True, LEFT_OUT_PARAM_GRADIENT)
FWD_IDS, GRAD_IDS = [c.id for c in FWD_CASES], [c.id for c in GRAD_CASES]
PARAM_FWD_IDS, PARAM_GRAD_IDS = [c.id for c in PARAM_FWD_CASES], [c.id for c in PARAM_GRAD_CASES]

# Cases that NO fp32 evaluation holds within 80 % of its budget: "<table> <id>" (table: fwd | grad | param-fwd |
# param-grad) -> the error of the fp32 VALU kernel (force_generic = 1: maf_generic / maf_bwd_generic) on the same inputs;
# the budget there is twice that figure.  Never from base, the cot_* families, layer_spread, zero_weights or masked_giant.
# Measured (profiles/r24/maf_rt_range.txt, tools/maf_rt_range_table.py): empty -- the VALU kernels use at most 11 % of any
# budget.  (grad maf37-inv-big_hidden used 88 % on maf_bwd_rt and 3 % on maf_bwd_generic: not a stress case but a finding
# about the kernel, fixed in csrc/mnf_rt_bwd.h delta_exponent; tests/test_hip_maf_rt_range.py says more.)
STRESS: dict[str, float] = {}


# ------------------------------------------------------------------------------------------------------- the fixtures
@dataclass
class MafFixture(Fixture):
    col: int | None = None                       # the column of y a bias / weight entry of the t head feeds
    zeroed: dict = field(default_factory=dict)   # weight name -> the column that was zeroed (hidden_outlier)
    unit: int | None = None                      # hidden_outlier: the unit

    def fn(self):
        ly, inverse = self.case.layer, self.case.inverse
        m = masks_of(ly)
        return lambda x, p: O.maf(x, p, m, ly.parity, inverse)


@functools.lru_cache(maxsize=None)
def masks_of(ly: Layer) -> tuple:
    return tuple(O.made_masks(ly.dim, ly.shape, 2 * ly.dim))


def weight_names(ly: Layer) -> list[str]:
    return [f"net.{2 * i}.weight" for i in range(len(ly.shape) + 1)]


def last_linear(ly: Layer) -> str:
    return f"net.{2 * len(ly.shape)}"


def masked_out(ly: Layer) -> dict:
    """weight name -> bool (out, in): the entries the mask removes"""
    return {k: ~m.T for k, m in zip(weight_names(ly), masks_of(ly))}


def net_index(ly: Layer, inverse: bool, col):
    """the net's input index of column ``col`` of x (see the module's docstring); its own inverse"""
    return ly.dim - 1 - col if (ly.parity and not inverse) else col


def y_column(ly: Layer, inverse: bool, i: int) -> int:
    """the column of y that element i of the net (s_i, t_i) lands in"""
    return ly.dim - 1 - i if (ly.parity and inverse) else i


def late_columns(ly: Layer, inverse: bool) -> list[int]:
    """the columns of x whose net index lies in the second half of the decode order"""
    return sorted(net_index(ly, inverse, i) for i in range(ly.dim // 2, ly.dim))


def base_inputs(ly: Layer):
    dim, rows = ly.dim, ly.rows
    sd = recipes.maf_params(2100 + dim + len(ly.shape), dim, ly.shape, gain=1.2, last_gain=0.5)
    x = recipes.gaussian(2200 + dim, rows, dim)
    w_y, w_l = recipes.gaussian(2300 + dim, rows, dim), recipes.gaussian(2301 + dim, rows, 1)[:, 0]
    return {k: v.clone() for k, v in sd.items()}, x.clone(), w_y.clone(), w_l.clone()


def outlier_unit(ly: Layer) -> int:
    """the first unit of the first hidden vector that has an input and that the next layer's mask lets connect"""
    m = masks_of(ly)
    for u in range(ly.shape[0]):
        if bool(m[0][:, u].any()) and bool(m[1][u, :].any()):
            return u
    raise ValueError(ly.tag)


def mid_element(ly: Layer) -> int:
    """the element of the t head the bias cases use: later elements exist and would read it"""
    return ly.dim // 2


@functools.lru_cache(maxsize=None)
def fixture(case: Case) -> MafFixture:
    ly, fam, inv = case.layer, case.family, case.inverse
    rows, dim = ly.rows, ly.dim
    sd, x, w_y, w_l = base_inputs(ly)
    fx = MafFixture(case, sd, x, w_y, w_l)
    last = last_linear(ly)
    if fam in ("base", "cot_large", "cot_small", "cot_y_only", "cot_ld_only", "cot_outlier"):
        if fam == "cot_small":  # a mean over many rows; rows beyond the sample larger than anything in it
            far = torch.from_numpy(unsampled_mask(rows))
            fx.w_y, fx.w_l = w_y * 1e-7, w_l * 1e-7
            fx.w_y[far] *= 37.0
            fx.w_l[far] *= 37.0
        elif fam == "cot_large":
            fx.w_y, fx.w_l = w_y * 40.0, w_l * 40.0
        elif fam == "cot_outlier":
            r_y, r_l = R.outlier_rows_of(rows)
            w_y[r_y] *= OUTLIER
            w_l[r_l] = float(np.copysign(OUTLIER, float(w_l[r_l])))
            fx.special = (r_y, r_l)
        elif fam == "cot_y_only":
            fx.w_l = None
        elif fam == "cot_ld_only":
            fx.w_y = None
    elif fam in ("big_rows", "big_late_elements"):
        big = big_rows_of(rows)
        cols = list(range(dim)) if fam == "big_rows" else late_columns(ly, inv)
        for r in big:
            x[r, cols] *= BIG_ROWS
        fx.sd = scaled(sd, {"net.0.weight": 1e-4})
        fx.special = big
    elif fam == "big_hidden":
        f = BIG_HIDDEN_FACTOR[(ly.tag, inv)]
        fx.sd = scaled(sd, {"net.0.weight": f, "net.2.weight": 1.0 / f})
    elif fam == "big_heads":
        g = BIG_HEADS_GAIN[inv]
        fx.sd = scaled(sd, {f"{last}.weight": g, f"{last}.bias": g})
    elif fam == "nonfinite_row":  # net index 1: every later element reads it
        x[BAD_ROW, net_index(ly, inv, 1)] = float("inf")
        fx.special, fx.bad_row = (BAD_ROW,), BAD_ROW
    elif fam in BIG_BIAS:
        # t_j at 2^20 / 2^36: y_j follows it; the element-by-element direction feeds y_j back, so the first MaskedLinear's
        # column for it is zeroed (both directions: the same parameters) and no later element's conditioner sees it
        j = mid_element(ly)
        sd[f"{last}.bias"][dim + j] = BIG_BIAS[fam]
        sd["net.0.weight"][:, j] = 0.0
        fx.col = y_column(ly, inv, j)
    elif fam == "layer_spread":
        if len(ly.shape) >= 2:
            f = g = SPREAD_F
            plan = [(f, f), (1.0 / (f * g), 1.0 / g), (g, 1.0)]
        else:
            f = SPREAD_F_ONE_HIDDEN
            plan = [(f, f), (1.0 / f, 1.0)]
        factors = {}
        for i, (fw, fb) in enumerate(plan):
            factors[f"net.{2 * i}.weight"], factors[f"net.{2 * i}.bias"] = fw, fb
        fx.sd = scaled(sd, factors)
    elif fam == "hidden_outlier":
        u = outlier_unit(ly)
        sd["net.0.weight"][u, :] = 0.0
        sd["net.0.bias"][u] = HIDDEN_OUTLIER
        sd["net.2.weight"][:, u] = 0.0
        fx.zeroed["net.2.weight"], fx.unit = u, u
    elif fam == "zero_weights":
        for k in weight_names(ly):
            sd[k].zero_()
    elif fam == "nonfinite_weight":
        # the LAST element's shift: nothing reads y_{dim-1} back, in either direction
        j = dim - 1
        k = int(torch.nonzero(masks_of(ly)[-1][:, dim + j])[0])
        sd[f"{last}.weight"][dim + j, k] = float("inf")
        fx.col = y_column(ly, inv, j)
    elif fam == "masked_giant":
        for k, out in masked_out(ly).items():
            sd[k][out] = GIANT
    else:
        raise ValueError(fam)
    return fx


def zeros_parked(fx: MafFixture) -> dict:
    """the fixture's parameters with exactly 0 in every masked-out weight"""
    sd = {k: v.clone() for k, v in fx.sd.items()}
    for k, out in masked_out(fx.case.layer).items():
        sd[k][out] = 0.0
    return sd


def base_rows(fx: MafFixture) -> torch.Tensor:
    """the batch with the special rows put back to their values in the base case"""
    x = fx.x.clone()
    if fx.special:
        x[list(fx.special)] = base_inputs(fx.case.layer)[1][list(fx.special)]
    return x


def evaluate(case: Case, sd: dict, x: torch.Tensor, dt) -> tuple:
    ly = case.layer
    return O.maf(x.to(dt), {k: v.to(dt) for k, v in sd.items()}, masks_of(ly), ly.parity, case.inverse)


@functools.lru_cache(maxsize=None)
def oracle(case: Case) -> Outputs:
    """fp32 and float64 oracle outputs (nonfinite_row: of the batch WITHOUT that row; rows are independent)"""
    fx = fixture(case)
    keep = fx.ordinary if fx.bad_row is not None else slice(None)
    with torch.no_grad():
        y32, ld32 = evaluate(case, fx.sd, fx.x[keep], torch.float32)
        y64, ld64 = evaluate(case, fx.sd, fx.x[keep], torch.float64)
    return Outputs(y32, ld32, y64, ld64)


@functools.lru_cache(maxsize=None)
def grad_oracle(case: Case) -> OracleGrads:
    """fp32 and float64 oracle gradients (nonfinite_row: of the batch WITHOUT that row: the loss is a sum over rows)"""
    fx = fixture(case)
    if fx.bad_row is None:
        return OracleGrads(fx.loss(), fx.x, fx.sd)
    keep = fx.ordinary
    sub = MafFixture(case, fx.sd, fx.x[keep], None if fx.w_y is None else fx.w_y[keep],
                     None if fx.w_l is None else fx.w_l[keep])
    return OracleGrads(sub.loss(), sub.x, sub.sd)


def bad_row_outputs(fx: MafFixture) -> tuple:
    """(y, log_det) of the fp32 oracle on the row with the non-finite input"""
    r = fx.bad_row
    with torch.no_grad():
        y, ld = evaluate(fx.case, fx.sd, fx.x[r:r + 1], torch.float32)
    return y[0], ld[0]


def y_parts(fx: MafFixture, y: torch.Tensor) -> list[tuple]:
    return P.y_parts(fx, y)


def grad_parts(fx: MafFixture, g: dict) -> list[tuple]:
    return P.grad_parts(fx, g)


# --------------------------------------------------------------------- float64: does a case reach the path it is named for
def net_inputs(fx: MafFixture) -> torch.Tensor:
    """float64 (rows, dim) in net order: what the first MaskedLinear reads -- x itself in the one-pass direction, the
    decoded elements in the element-by-element one (at step i: the columns below i of it, zeros beyond)"""
    x = fx.x.double()
    if fx.case.inverse:
        return x
    with torch.no_grad():
        y, _ = evaluate(fx.case, fx.sd, fx.x, torch.float64)
    return y


def first_hidden(fx: MafFixture, v: torch.Tensor) -> torch.Tensor:
    """float64 magnitudes (rows, n_0) of the first hidden vector; element-by-element: the largest over the decode steps"""
    ly, sd = fx.case.layer, fx.sd
    W = sd["net.0.weight"].double().T * masks_of(ly)[0].double()
    b = sd["net.0.bias"].double()
    fin = torch.where(torch.isfinite(v), v, torch.zeros_like(v))
    if fx.case.inverse:
        return torch.relu(fin @ W + b)
    out = torch.relu(b).expand(v.shape[0], -1).clone()
    for i in range(1, ly.dim + 1):
        part = fin.clone()
        part[:, i:] = 0.0
        out = torch.maximum(out, torch.relu(part @ W + b))
    return out


def step_row_max(fx: MafFixture, v: torch.Tensor) -> torch.Tensor:
    """(rows, dim): the row's largest magnitude over the columns below i, for every decode step i"""
    a = v.abs()
    a = torch.where(torch.isfinite(a), a, torch.zeros_like(a))
    run = torch.cummax(a, dim=1).values
    return torch.cat([torch.zeros(a.shape[0], 1, dtype=a.dtype), run[:, :-1]], dim=1)


def head_outputs_max(fx: MafFixture) -> float:
    """the largest float64 magnitude of the conditioner's outputs (s, t) at the net's final inputs"""
    ly = fx.case.layer
    with torch.no_grad():
        out = O.made(net_inputs(fx), {k: p.double() for k, p in fx.sd.items()}, masks_of(ly))
    return float(out.abs().max())


def path_figures(fx: MafFixture) -> dict:
    """what the host test asserts on, computed in float64"""
    ly, sd = fx.case.layer, fx.sd
    v = net_inputs(fx)
    h = first_hidden(fx, v)
    out = {"input_tiles": tile_max(v), "hidden_tiles": tile_max(h), "step_row_max": step_row_max(fx, v),
           "scale": R.grad_scale(fx.w_y, fx.w_l) if (fx.w_y is not None or fx.w_l is not None) else 1.0}
    unmasked = []
    for k, gone in masked_out(ly).items():
        w = sd[k].double().abs()
        w = torch.where(gone | ~torch.isfinite(w), torch.zeros_like(w), w)
        unmasked.append(float(w.max()))
    out["per_linear"], out["weight_max"] = unmasked, max(unmasked)
    out["first_hidden_row_max"] = float(h.max(dim=1).values.min())
    out["first_hidden_second"] = float(h.topk(2, dim=1).values[:, 1].max())
    return out


# ---------------------------------------------------------------------------------------------------------- the runners
def module_of(amd, ly: Layer, sd: dict, force_generic: int = 2):
    f = amd.MAF(ly.dim, parity=ly.parity, h_sizes=ly.shape)
    missing = f.load_state_dict(sd, strict=False)
    assert all(k.endswith(".mask") for k in missing.missing_keys) and not missing.unexpected_keys
    for m, ours in zip(f._masked(), masks_of(ly)):
        assert torch.equal(m.mask != 0, ours), "O.made_masks is not the library's mask"
    f.force_generic = force_generic
    return f.to(DEV)


def opt_in() -> object:
    """The solve route is opt-in (tests/test_hip_maf_seq_bwd_rt.py does the same with monkeypatch): returns the value to
    put back."""
    from torch_mnf_amd import _dispatch

    old = _dispatch.MAF_SEQ_BWD_RT_MIN_ROWS
    _dispatch.MAF_SEQ_BWD_RT_MIN_ROWS = 0
    return old


def opt_back(old) -> None:
    from torch_mnf_amd import _dispatch

    _dispatch.MAF_SEQ_BWD_RT_MIN_ROWS = old


def call(amd, f, case: Case, x: torch.Tensor, want: str):
    """(y, log_det) on the CPU of one pass without gradients; the kernel that ran is the one wanted"""
    with torch.no_grad():
        y, ld = (f.inverse if case.inverse else f.forward)(x.to(DEV))
    torch.cuda.synchronize()
    assert amd.last_kernel() == want, (case.id, amd.last_kernel(), want)
    return y.cpu(), ld.cpu()


def _stress_key(table: str, cid: str) -> str:
    return f"{table} {cid}"


def compare(key: str, got, ref32, ref64, what: str, rowwise: bool = False) -> float:
    """rt_fwd_range_cases.compare with this module's STRESS"""
    from helpers import MAX_WIDENING, RTOL, assert_parity, assert_row_parity

    rule = assert_row_parity if rowwise else assert_parity
    if key in STRESS:  # the budget is twice the VALU kernel's figure, without head-room on top
        return rule(got, ref32.numpy(), None, what, rtol=2.0 * STRESS[key], max_widening=None)
    return rule(got, ref32.numpy(), ref64.numpy(), what, rtol=RTOL, max_widening=MAX_WIDENING)


def run_forward(amd, case: Case, prefix: str = "", force_generic: int = 2) -> dict:
    """One case of the forward or of the parameter table through maf_rt / maf_seq_rt (force_generic = 1: maf_generic).
    Returns {"y", "log_det", "kernel", "seconds"}."""
    fx = fixture(case)
    ref = oracle(case)
    ly, fam, cid = case.layer, case.family, case.id
    table = "fwd" if fam in FWD_FAMILIES else "param-fwd"
    what, key = f"{prefix}{table} {cid}", _stress_key(table, cid)
    want = kernel_of(case, False, force_generic)
    t0 = time.time()
    f = module_of(amd, ly, fx.sd, force_generic)
    y, ld = call(amd, f, case, fx.x, want)
    clean = call(amd, f, case, base_rows(fx), want) if fam in INDEPENDENT else None
    parked = call(amd, module_of(amd, ly, zeros_parked(fx), force_generic), case, fx.x, want) if fam == "masked_giant" else None
    seconds = time.time() - t0
    keep, special = fx.ordinary, list(fx.special)
    if fx.bad_row is not None:
        # the row with the non-finite input is finite where the fp32 oracle's is; the others do not notice
        by, bld = bad_row_outputs(fx)
        got_fin, fin = torch.isfinite(y[fx.bad_row]), torch.isfinite(by)
        assert torch.equal(got_fin, fin), f"{what}: y of the bad row is finite in {got_fin.nonzero()[:, 0].tolist()}, " \
                                          f"the reference's in {fin.nonzero()[:, 0].tolist()}"
        assert bool(torch.isfinite(ld[fx.bad_row])) == bool(torch.isfinite(bld)), what
        compare(key, y[keep], ref.y32, ref.y64, what + " y (other rows)", rowwise=True)
        compare(key, ld[keep], ref.ld32, ref.ld64, what + " ld (other rows)")
        near = tile_neighbours(fx.bad_row, ly.rows)
        sub = [r - (r > fx.bad_row) for r in near]
        assert len(near) == 15
        compare(key, ld[near], ref.ld32[sub], ref.ld64[sub], what + " ld (the 15 tile neighbours)")
    else:
        if fam == "nonfinite_weight":
            fin, want_fin = torch.isfinite(y), torch.isfinite(ref.y32)
            assert torch.equal(fin, want_fin), f"{what}: y is non-finite in columns {(~fin).any(0).nonzero()[:, 0].tolist()}, " \
                                               f"the reference's in {(~want_fin).any(0).nonzero()[:, 0].tolist()}"
        for (label, part, rowwise), (_, p32, _), (_, p64, _) in zip(y_parts(fx, y), y_parts(fx, ref.y32), y_parts(fx, ref.y64)):
            if fam == "nonfinite_weight" and not rowwise:
                continue  # (the non-finite column: its pattern is held above)
            compare(key, part, p32, p64, f"{what} {label}", rowwise=rowwise)
        compare(key, ld[keep], ref.ld32[keep], ref.ld64[keep], what + (" ld (ordinary rows)" if special else " ld"))
        if special:
            compare(key, ld[special], ref.ld32[special], ref.ld64[special], what + " ld (special rows)")
    if clean is not None:
        same_bits(y[keep], clean[0][keep], what + " y of the ordinary rows, with and without the special rows")
        same_bits(ld[keep], clean[1][keep], what + " ld of the ordinary rows, with and without the special rows")
    if parked is not None:
        same_bits(y, parked[0], what + " y, with 2^40 and with 0 in the masked-out weights")
        same_bits(ld, parked[1], what + " ld, with 2^40 and with 0 in the masked-out weights")
    return {"y": y, "log_det": ld, "kernel": want, "seconds": seconds}


def gpu_grads(amd, fx: MafFixture, force_generic: int = 2, sd: dict | None = None):
    """(gradients {"x", parameter names}, name of the gradient kernel) of one backward pass on the GPU.  The caller has
    opted the solve route in."""
    case = fx.case
    f = module_of(amd, case.layer, fx.sd if sd is None else sd, force_generic)
    x = fx.x.detach().to(DEV).requires_grad_(True)
    y, ld = (f.inverse if case.inverse else f.forward)(x)
    terms = ([(y * fx.w_y.to(DEV)).sum()] if fx.w_y is not None else []) + \
            ([(ld * fx.w_l.to(DEV)).sum()] if fx.w_l is not None else [])
    sum(terms).backward()
    torch.cuda.synchronize()
    return {"x": x.grad, **{n: q.grad for n, q in f.named_parameters()}}, amd.last_kernel()


def masked_entries_are_zero(ly: Layer, got: dict, what: str):
    for k, gone in masked_out(ly).items():
        g = got[k].detach().cpu()
        assert bool((g[gone] == 0).all()), f"{what}: grad {k} has {int((g[gone] != 0).sum())} masked-out entries that are not exactly 0"


def run_gradients(amd, case: Case, prefix: str = "", force_generic: int = 2) -> dict:
    """One case of the gradient or of the parameter table through maf_bwd_rt / maf_seq_bwd_rt (force_generic = 1:
    maf_bwd_generic): kernel name, every gradient within the audited budget of the float64 oracle, grad_x of the ordinary
    rows on their own norm, the masked-out entries exactly zero.  Returns the gradients."""
    fx, ref = fixture(case), grad_oracle(case)
    ly, fam = case.layer, case.family
    table = "grad" if fam in GRAD_FAMILIES else "param-grad"
    what = f"{prefix}{table} {case.id}"
    key = _stress_key(table, case.id)
    base = 2.0 * STRESS[key] if key in STRESS else GBASE  # (a base other than GBASE is recorded as a stress comparison)
    want = kernel_of(case, True, force_generic)
    old = opt_in()
    try:
        got, kernel = gpu_grads(amd, fx, force_generic)
        parked = gpu_grads(amd, fx, force_generic, sd=zeros_parked(fx))[0] if fam == "masked_giant" else None
    finally:
        opt_back(old)
    assert kernel == want, (what, kernel, want)
    masked_entries_are_zero(ly, got, what)
    keep = fx.ordinary
    r32, r64 = ref.g[torch.float32]["x"], ref.g[torch.float64]["x"]
    gx = got["x"].detach().cpu()
    if fx.bad_row is not None:
        assert bool(torch.isfinite(gx[keep]).all()), what
        check_vs_float64(gx[keep], r32, r64, what + " grad x (other rows)", base)
        near = tile_neighbours(fx.bad_row, ly.rows)
        sub = [r - (r > fx.bad_row) for r in near]
        assert len(near) == 15
        check_vs_float64(gx[near], r32[sub], r64[sub], what + " grad x (the 15 tile neighbours)", base)
        return got
    ref.check_all(got, what, base=base)
    if fx.special:  # a normwise bound over all rows lets an outlier row's magnitude hide errors everywhere else
        check_vs_float64(gx[keep], r32[keep], r64[keep], what + " grad x (ordinary rows)", base)
    cpu = {k: v.detach().cpu() for k, v in got.items()}
    for (label, g), (_, p32), (_, p64) in zip(grad_parts(fx, cpu), grad_parts(fx, ref.g[torch.float32]),
                                               grad_parts(fx, ref.g[torch.float64])):
        check_vs_float64(g, p32, p64, f"{what} {label}", base)
    if parked is not None:
        # grad_x is row-local; the parameter sums of the default mode are atomic adds over several workgroups, whose last
        # bits differ from run to run with ANY weights: those are held to the oracle above, in both runs
        same_bits(gx, parked["x"].detach().cpu(), what + " grad x, with 2^40 and with 0 in the masked-out weights")
        masked_entries_are_zero(ly, parked, what + " (zeros parked)")
        ref.check_all(parked, what + " (zeros parked)", base=base)
        if amd.deterministic():
            for k in got:
                same_bits(cpu[k], parked[k].detach().cpu(), f"{what} grad {k}, with 2^40 and with 0 in the masked-out weights")
    return got


def deterministic_cases(tag: str, inverse: bool) -> list[Case]:
    """the gradient cases of one layer that the MNF_DETERMINISTIC=1 child scripts run as well"""
    return [c for c in GRAD_CASES if c.layer.tag == tag and c.inverse == inverse
            and c.family in ("cot_small", "cot_outlier", "big_rows")]


def run_deterministic(amd, tag: str, inverse: bool) -> int:
    """Those cases on the fixed-order kernels: the same budget as every other gradient comparison, and a second pass whose
    gradients are the first one's bit for bit.  Returns how many ran."""
    assert amd.deterministic()
    cases = deterministic_cases(tag, inverse)
    for case in cases:
        got = run_gradients(amd, case, prefix="deterministic ")
        old = opt_in()
        try:
            again, kernel = gpu_grads(amd, fixture(case))
        finally:
            opt_back(old)
        assert kernel == kernel_of(case, True), (case.id, kernel)
        for k in got:
            assert torch.equal(got[k].view(torch.int32), again[k].view(torch.int32)), (case.id, k)
    return len(cases)


def table(records: list[dict]) -> str:
    return R.table(records)
