"""The PARAMETER range of the run-time-shaped kernels (ahf_rt, nsf_rt, rnvp_rt and the three *_bwd_rt): the case table and
the runner.  Not collected: tests/test_rt_param_range_host.py (CPU: every fixture is sound and reaches the path it is named
for), tests/test_hip_rt_param_range.py (GPU), tests/rt_deterministic_child.py (the gradient half under MNF_DETERMINISTIC=1)
and tools/rt_param_range_table.py import it, so that all look at the same inputs.

tests/rt_bwd_range_cases.py and tests/rt_fwd_range_cases.py move the INPUTS out of the split range; every weight-side
fixture they have keeps the one quantity the weight staging depends on where it was: the launch's staging exponent
(csrc/mnf_rt.h block_weight_max, weight_exponent: every weight of every net of the layer is staged as w 2^-e with the
largest one just below 2^15).  The families here move that exponent, or the spread of magnitudes under it:

  big_bias_head    one bias entry of an output head at 2^20 / 2^36, placed where the float64 function of everything else
                   does not change.  A scan that lets the bias into the maximum stages weights of ~0.1 at 2^-21: f16
                   subnormals, carried to 2^-36 absolute = ~1e-3 relative (the scan looks at weights only)
  layer_spread     per-Linear maxima 2^24 apart through LeakyReLU's positive homogeneity (powers of two: the fp32 oracle's
                   outputs are the base case's bit for bit), hidden vectors below 2^13: the smallest Linear is staged near
                   2^-10, where the split still carries fp32's precision (the envelope: 2^27)
  hidden_outlier   one unit of the first hidden vector at 2^24, the next Linear's column for it zeroed: every row takes
                   finish_layer's second split with the other units scaled to ~2^-11 of their size (fp32 grade up to 2^25)
  zero_weights     weight_exponent(0) = 0; outputs are functions of the biases alone
  nonfinite_weight one +inf in a shift head: finite_abs keeps it out of the maximum, the output column it feeds is
                   non-finite (as the reference's), every other column does not notice

Comparison rule: the forward table's (helpers.assert_parity / assert_row_parity at RTOL with MAX_WIDENING against the fp32
and the float64 oracle, y row by row) and the gradient table's (OracleGrads at GBASE); every comparison is recorded for
tests/test_zz_audit.py's 80 % rule."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np
import torch

import rt_bwd_range_cases as R
import rt_fwd_range_cases as F
from helpers import assert_parity
from oracle import flow_oracle as O
from rt_bwd_range_cases import GBASE, Case, Fixture, Layer, OracleGrads, base_inputs, check_vs_float64, module_of, scaled
from rt_fwd_range_cases import call, compare, same_bits

TAIL = F.TAIL
GRAD_LAYERS = list(R.LAYERS)
FWD_ONLY_LAYERS = [ly for ly in F.FWD_LAYERS if ly.tag in ("ahf512", "ahf40w", "rnvp800", "nsf16")]
LAYERS = GRAD_LAYERS + FWD_ONLY_LAYERS

BIG_BIAS = {"big_bias_head_2p20": 2.0 ** 20, "big_bias_head_2p36": 2.0 ** 36}
SPREAD_F, SPREAD_F_ONE_HIDDEN = 2.0 ** 8, 2.0 ** 9
SPREAD_G = SPREAD_F  # the third Linear's factor: f in the table; tools/rt_param_range_table.py --beyond raises it alone
# min / max of the per-Linear maxima a layer_spread fixture must reach (tests/test_rt_param_range_host.py): 2^-24, except
# where the stated factors cannot give it.  One hidden layer has two Linears to move apart, by f^2 = 2^18 (the hidden
# vector has to stay below 2^13); RNVP(800, (100,)) loses another 1.5 bits to its first Linear's init range (fan-in 800:
# 0.053 against the heads' 0.15).  RNVP(64, (7, 9, 11)): the Linear that is divided has the LARGEST base maximum (fan-in
# 7: 0.558 against 0.499 for the one that ends up largest): 2^-23.84.
SPREAD_REACH = {"rnvp50": 2.0 ** -18, "ahf40w": 2.0 ** -18, "rnvp800": 2.0 ** -16, "rnvp64": 2.0 ** -23.5}
OUTLIER = 2.0 ** 24
OUTLIER_UNIT = 3
FAMILIES = [*BIG_BIAS, "layer_spread", "hidden_outlier", "zero_weights", "nonfinite_weight"]
GRAD_FAMILIES = [f for f in FAMILIES if f != "nonfinite_weight"]

# (layer, family) pairs whose fp32 oracle is further than MAX_WIDENING / 2 from the float64 oracle at the stated magnitude
# (tests/test_rt_param_range_host.py holds every case of the table to that cap): tag, family -> the figure.  The
# magnitude is not lowered for them; they leave the family.
LEFT_OUT_FORWARD: dict[tuple, str] = {}
LEFT_OUT_GRADIENT: dict[tuple, str] = {}


def _dirs(ly: Layer):
    return (False,) if ly.kind == "rnvp" else (False, True)


def wanted(ly: Layer, family: str) -> bool:
    return not (family == "nonfinite_weight" and ly.kind == "nsf")


FWD_CASES = [Case(ly, fam, inv) for ly in LAYERS for inv in _dirs(ly) for fam in FAMILIES
             if wanted(ly, fam) and (ly.tag, fam) not in LEFT_OUT_FORWARD]
GRAD_CASES = [Case(ly, fam, inv) for ly in GRAD_LAYERS for inv in _dirs(ly) for fam in GRAD_FAMILIES
              if (ly.tag, fam) not in LEFT_OUT_GRADIENT]
FWD_IDS = [c.id for c in FWD_CASES]
GRAD_IDS = [c.id for c in GRAD_CASES]

# Forward cases that NO fp32 evaluation holds within 80 % of RTOL + widening: id -> the error of the fp32 VALU kernel
# (force_generic = 1) on the same inputs; the budget there is twice that figure.  layer_spread never belongs here: its
# float64 function is the base case's.  Measured (profiles/r11/rt_param_range.txt): empty.
STRESS: dict[str, float] = {}


# ------------------------------------------------------------------------------------------------------- the fixtures
@dataclass
class ParamFixture(Fixture):
    col: int | None = None      # the column of y the case's bias / weight entry feeds (ahf, rnvp)
    dead: dict = field(default_factory=dict)      # bias name -> indices whose gradient is exactly zero (nsf)
    zeroed: dict = field(default_factory=dict)    # weight name -> the column that was zeroed (hidden_outlier)


def nets_of(ly: Layer) -> tuple:
    return {"ahf": ("s_net", "t_net"), "nsf": ("f1", "f2"), "rnvp": ("net",)}[ly.kind]


def stages(ly: Layer, sd: dict, net: str) -> list[list[str]]:
    """the Linears of one conditioner net in order, as parameter-name prefixes; RNVP: its two heads are the last stage"""
    out = [[f"{net}.{i}"] for i in O.linear_indices(sd, net)]
    return out + [["t", "s"]] if ly.kind == "rnvp" else out


def weight_names(ly: Layer, sd: dict) -> list[str]:
    return [f"{p}.weight" for net in nets_of(ly) for st in stages(ly, sd, net) for p in st]


def shift_head(ly: Layer, sd: dict) -> str:
    """the prefix of the Linear whose outputs are the shift (ahf: t_net's last; rnvp: t)"""
    return "t" if ly.kind == "rnvp" else stages(ly, sd, "t_net")[-1][0]


def head_index(ly: Layer) -> int:
    """j: the entry of the shift head the case uses (5 as in the issue's check; the half of dim 10 has 5 entries)"""
    n = ly.dim if ly.kind == "rnvp" else ly.dim // 2
    return 5 if n > 5 else n - 2


def y_column(ly: Layer, j: int) -> int:
    return j if ly.kind == "rnvp" else R.act_columns(ly).start + j


NSF_DEAD_COLUMN = 1  # of the upper half (the one f1 transforms, in either direction)


@functools.lru_cache(maxsize=None)
def fixture(case: Case) -> ParamFixture:
    ly, fam = case.layer, case.family
    sd, x, w_y, w_l, mask = base_inputs(ly)
    sd = {k: v.clone() for k, v in sd.items()}
    fx = ParamFixture(case, sd, x, w_y, w_l, mask)
    if fam in BIG_BIAS:
        v = BIG_BIAS[fam]
        if ly.kind == "nsf":
            # the 3K - 1 output biases of one transformed column; every input of that column beyond the tail bound, where
            # the spline passes it through whatever its parameters are
            h, n = ly.dim // 2, 3 * ly.shape[0] - 1
            c = h + NSF_DEAD_COLUMN
            x[:, c] = torch.where(x[:, c] < 0, -1.0, 1.0) * (4.0 + x[:, c].abs() % 1.0)
            name = stages(ly, sd, "f1")[-1][0] + ".bias"
            idx = torch.arange(NSF_DEAD_COLUMN * n, (NSF_DEAD_COLUMN + 1) * n)
            sd[name][idx] = v
            fx.dead = {name: idx}
        else:
            j = head_index(ly)
            sd[shift_head(ly, sd) + ".bias"][j] = v
            fx.col = y_column(ly, j)
    elif fam == "layer_spread":
        factors = {}
        for net in nets_of(ly):
            st = stages(ly, sd, net)
            if len(st) - 1 >= 2:
                f, g = SPREAD_F, SPREAD_G
                plan = [(f, f), (1.0 / (f * g), 1.0 / g), (g, 1.0)]
            else:
                f = SPREAD_F_ONE_HIDDEN
                plan = [(f, f), (1.0 / f, 1.0)]
            for prefixes, (fw, fb) in zip(st, plan):
                for p in prefixes:
                    factors[f"{p}.weight"], factors[f"{p}.bias"] = fw, fb
        fx.sd = scaled(sd, factors)
    elif fam == "hidden_outlier":
        # (row u of the first Linear is zeroed too, so that the unit IS 2^24 in every row and not 2^24 - 0.3 in half of
        #  them: the host test's figure is "at least 2^24")
        u = OUTLIER_UNIT
        for net in nets_of(ly):
            st = stages(ly, sd, net)
            sd[f"{st[0][0]}.weight"][u, :] = 0.0
            sd[f"{st[0][0]}.bias"][u] = OUTLIER
            for p in st[1]:
                sd[f"{p}.weight"][:, u] = 0.0
                fx.zeroed[f"{p}.weight"] = u
    elif fam == "zero_weights":
        for k in weight_names(ly, sd):
            sd[k].zero_()
    elif fam == "nonfinite_weight":
        j = head_index(ly)
        sd[shift_head(ly, sd) + ".weight"][j, 1] = float("inf")
        fx.col = y_column(ly, j)
    else:
        raise ValueError(fam)
    return fx


def y_parts(fx: ParamFixture, y: torch.Tensor) -> list[tuple]:
    """(label, part of y, row-wise?): y as the comparisons take it -- with a column of its own magnitude on its own"""
    if fx.col is None:
        return [("y", y, True)]
    others = [c for c in range(y.shape[1]) if c != fx.col]
    return [("y (other columns)", y[:, others], True), (f"y (column {fx.col})", y[:, fx.col], False)]


@functools.lru_cache(maxsize=None)
def oracle(case: Case) -> F.Outputs:
    fx = fixture(case)
    with torch.no_grad():
        y32, ld32 = F.evaluate(case, fx.sd, fx.x, fx.mask, torch.float32)
        y64, ld64 = F.evaluate(case, fx.sd, fx.x, fx.mask, torch.float64)
    return F.Outputs(y32, ld32, y64, ld64)


@functools.lru_cache(maxsize=None)
def grad_oracle(case: Case) -> OracleGrads:
    fx = fixture(case)
    return OracleGrads(fx.loss(), fx.x, fx.sd)


def grad_parts(fx: ParamFixture, g: dict) -> list[tuple]:
    """(label, tensor) beyond the whole tensors: a zeroed column's gradient (2^24 times its neighbours') on its own
    maximum, and the other columns on theirs"""
    out = []
    for k, u in fx.zeroed.items():
        rest = [c for c in range(g[k].shape[1]) if c != u]
        out += [(f"grad {k} (column {u})", g[k][:, u]), (f"grad {k} (other columns)", g[k][:, rest])]
    return out


# --------------------------------------------------------------------- float64: does a case reach the path it is named for
def path_figures(fx: ParamFixture) -> dict:
    ly, sd = fx.case.layer, fx.sd
    per_linear = [float(sd[f"{p}.weight"].double().abs().max()) for net in nets_of(ly) for st in stages(ly, sd, net) for p in st]
    finite = [float(v[torch.isfinite(v)].abs().max()) for v in (sd[k].double() for k in weight_names(ly, sd))]
    out = {"per_linear": per_linear, "weight_max": max(finite)}
    ins = R.conditioner_inputs(fx)
    hidden = {net: R.mlp_hidden(v, sd, net, ly.kind == "rnvp") for net, v in ins.items()}
    out["hidden_max"] = max(float(h.abs().max()) for hs in hidden.values() for h in hs)
    first = [hs[0].abs() for hs in hidden.values()]
    out["first_hidden_row_max"] = min(float(h.max(dim=1).values.min()) for h in first)
    out["first_hidden_second"] = max(float(h.topk(2, dim=1).values[:, 1].max()) for h in first)
    return out


# ---------------------------------------------------------------------------------------------------------- the runner
def _compare(cid: str, got, ref32, ref64, what: str, rowwise: bool = False) -> float:
    if cid in STRESS:  # the budget is twice the VALU kernel's figure, without head-room on top
        assert not rowwise or got.ndim == 2
        from helpers import assert_row_parity
        return (assert_row_parity if rowwise else assert_parity)(got, ref32.numpy(), None, what, rtol=2.0 * STRESS[cid],
                                                                   max_widening=None)
    return compare(cid, got, ref32, ref64, what, rowwise=rowwise)


def run_forward(amd, case: Case, prefix: str = "", force_generic: int = 2) -> dict:
    """One case through the forward kernel.  Returns {"y", "log_det"}."""
    fx, ref = fixture(case), oracle(case)
    ly, what, cid = case.layer, f"{prefix}{case.id}", case.id
    f = module_of(amd, fx)
    f.force_generic = force_generic
    if ly.seeded:
        assert torch.equal(f.mask_for(R.RNVP_SEED, ly.rows).cpu(), fx.mask), "seeded_mask() is not the library's mask"
    y, ld = call(amd, f, fx, fx.x, F.kernel_of(ly, force_generic))
    F.passes_through(fx, fx.x, y, what)
    if fx.dead:  # the column whose spline parameters are 2^20 / 2^36: selected, not multiplied by an indicator
        c = ly.dim // 2 + NSF_DEAD_COLUMN
        assert bool((fx.x[:, c].abs() > TAIL).all())
        same_bits(y[:, c], fx.x[:, c], what + ": the column beyond the tail bound")
    if case.family == "nonfinite_weight":
        fin, want = torch.isfinite(y), torch.isfinite(ref.y32)
        assert torch.equal(fin, want), f"{what}: y is non-finite in columns {(~fin).any(0).nonzero()[:, 0].tolist()}, " \
                                       f"the reference's in {(~want).any(0).nonzero()[:, 0].tolist()}"
    for (label, part, rowwise), (_, p32, _), (_, p64, _) in zip(y_parts(fx, y), y_parts(fx, ref.y32), y_parts(fx, ref.y64)):
        if case.family == "nonfinite_weight" and not rowwise:
            continue  # (the non-finite column: its pattern is held above)
        _compare(cid, part, p32, p64, f"{what} {label}", rowwise=rowwise)
    _compare(cid, ld, ref.ld32, ref.ld64, what + " ld")
    return {"y": y, "log_det": ld}


def run_gradients(amd, case: Case, prefix: str = "", force_generic: int = 2) -> dict:
    """One case through the gradient kernel: its name, every gradient within GBASE + widening of the float64 oracle."""
    fx, ref = fixture(case), grad_oracle(case)
    what = f"{prefix}{case.id}"
    got, kernel = R.gpu_grads(amd, fx, force_generic)
    want = case.layer.kernel if force_generic == 2 else case.layer.kernel.replace("_rt", "_generic")
    assert kernel == want, (what, kernel)
    ref.check_all(got, what, base=GBASE)
    cpu = {k: v.detach().cpu() for k, v in got.items()}
    for (label, g), (_, r32), (_, r64) in zip(grad_parts(fx, cpu), grad_parts(fx, ref.g[torch.float32]),
                                               grad_parts(fx, ref.g[torch.float64])):
        check_vs_float64(g, r32, r64, f"{what} {label}", GBASE)
    for name, idx in fx.dead.items():
        assert float(cpu[name][idx].abs().max()) == 0.0, f"{what}: grad {name} of the dead spline parameters is not zero"
    return got


def table(records: list[dict]) -> str:
    return R.table(records)
