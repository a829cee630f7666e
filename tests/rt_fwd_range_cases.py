"""The operating range of the run-time-shaped FORWARD kernels (ahf_rt, ahf_stack_rt, nsf_rt, rnvp_rt): the case table and
the runner.  Not collected: tests/test_rt_fwd_range_host.py (CPU: every fixture is sound and reaches the path it is named
for), tests/test_hip_rt_fwd_range.py (GPU) and tools/rt_fwd_range_table.py import it, so that all look at the same inputs.

These kernels run the conditioner in split f16 and have no fp32 fix-up pass; outside the split range (|v| >= 2^13) they
stay right only through code in csrc/mnf_rt.h that inputs and weights of scale 1 never execute, instantiated per size class
(MT_MAX 4 / 8 / 16) and per staging variant (weights resident in LDS / streamed):

  first_layer   the per-row power-of-two down-scale of the input rows (max_over_q, scale[t])
  finish_layer  the second split of a hidden vector beyond the range (h.up[t]), applied again in out_tile and in the next
                layer's scale[t]
  weights       staged at the top of f16's range (weight_exponent, Source::wdown, wup)
  epilogues     exp / reciprocal / log intrinsics on conditioner outputs far beyond scale 1 (big_heads)

The gradient table (tests/rt_bwd_range_cases.py) reaches some of these through its fixtures but looks at gradients only,
and the gradient kernels recompute the conditioner: y and log_det on those inputs are looked at here.  Its six layers are
taken over unchanged; six forward-only layers add the widths and staging variants the gradient kernels do not have.

Every comparison is against the float64 oracle: y ROW BY ROW (helpers.assert_row_parity: each row on its own maximum, so a
row of magnitude 1e5 cannot hide its neighbours), log_det on the ordinary and on the special rows as tensors of their own."""
from __future__ import annotations

import functools
import time
from dataclasses import dataclass

import numpy as np
import torch

import rt_bwd_range_cases as R
from helpers import MAX_WIDENING, RTOL, assert_parity, assert_row_parity
from oracle import flow_oracle as O
from rt_bwd_range_cases import (BAD_ROW, BIG_ROWS, DEV, LIMIT, Case, Fixture, Layer, big_rows_of, conditioner_inputs,
                                mlp_hidden, module_of, scaled, straddles, tile_max)

TAIL = 3.0  # NSF_CL's tail bound B (module_of builds the layers with B=3)

# forward-only layers, 300 rows each (19 tiles of 16 rows, the last one of 12)
FWD_LAYERS = [
    Layer("ahf512", "ahf", 512, (24, 24, 24), 300),             # streaming weights
    Layer("ahf128", "ahf", 128, (100,), 300),                   # MT_MAX 8, one hidden layer
    Layer("ahf40w", "ahf", 40, (256,), 300, parity=True),       # MT_MAX 16
    Layer("rnvp800", "rnvp", 800, (100,), 300),                 # streaming
    Layer("rnvp130", "rnvp", 130, (130,), 300, seeded=True),    # rows not 16-byte aligned: the widest streaming class
    Layer("nsf16", "nsf", 16, (16, 64), 300),                   # K = 16, n_h = 64: the envelope's upper edge
]
LAYERS = list(R.LAYERS) + FWD_LAYERS

# big_hidden: first-layer weights x f, the next layer's / f (rt_bwd_range_cases.BIG_HIDDEN_FACTOR says how f is chosen);
# for the forward-only layers f is set so that at least 3 of the 19 tiles have a hidden magnitude at or beyond 2^13 and at
# least 3 lie below it (tests/test_rt_fwd_range_host.py holds every entry to that and prints the counts)
BIG_HIDDEN_FACTOR = {**R.BIG_HIDDEN_FACTOR, "ahf512": 4700.0, "ahf128": 4096.0, "ahf40w": 3500.0, "rnvp800": 3500.0,
                     "rnvp130": 3500.0, "nsf16": 3000.0}

# big_heads: the last Linear of every conditioner net (weight and bias) x g.  AffineHalfFlow's exp(+-s) then spans about 20
# decades per batch, RNVP's gates saturate (|log_det| up to about 185), the spline sees large raw parameters.  g is as
# large as the ORACLE allows: at 64 the fp32 oracle returns non-finite RNVP rows; at 16 the fp32 oracle's own distance from
# float64 is 2e-4 for NSF_CL and 4.2e-5 for ahf40w (the cap for a non-stress fixture is 5e-5)
BIG_HEADS_GAIN = {"ahf64": 16.0, "ahf10": 16.0, "ahf512": 16.0, "ahf128": 4.0, "ahf40w": 4.0,
                  "nsf50": 4.0, "nsf6": 4.0, "nsf16": 4.0,
                  "rnvp50": 16.0, "rnvp64": 16.0, "rnvp800": 16.0, "rnvp130": 16.0}

FAMILIES = ["base", "big_cond_rows", "big_act_rows", "big_second_rows", "big_hidden", "big_heads", "nonfinite_row"]
# families whose special rows must not change any other row, bit for bit
INDEPENDENT = ("big_cond_rows", "big_act_rows", "big_second_rows", "nonfinite_row")


def wanted(ly: Layer, family: str) -> bool:
    return not (family == "big_act_rows" and ly.kind != "ahf") and not (family == "big_second_rows" and ly.kind != "nsf")


def _cases() -> list[Case]:
    return [Case(ly, fam, inverse) for ly in LAYERS for inverse in ((False,) if ly.kind == "rnvp" else (False, True))
            for fam in FAMILIES if wanted(ly, fam)]


CASES = _cases()
CASE_IDS = [c.id for c in CASES]
STACK_ID = "stack-ahf64x3"

# Cases that NO fp32 evaluation holds within 80 % of RTOL + widening: id -> the error of the fp32 VALU kernel
# (force_generic = 1) on the same inputs; the budget there is twice that figure (tools/rt_fwd_range_table.py
# measures both kernels; profiles/r10/rt_fwd_range.txt has both tables).  base, big_cond_rows, big_second_rows and big_hidden never belong here: their float64 function is
# the base case's.
# Measured (profiles/r10/rt_fwd_range.txt): empty.  No case reaches 80 % on either kernel family -- worst share of budget
# ahf_rt 39 %, ahf_stack_rt 6 %, nsf_rt 52 % (nsf16-inv-big_hidden), rnvp_rt 15 %; the fp32 VALU kernels on the same
# inputs: ahf_generic 68 %, nsf_generic 68 %, rnvp_generic 17 %.
STRESS: dict[str, float] = {}


def kernel_of(ly: Layer, force_generic: int = 2) -> str:
    return f"{ly.kind}_rt" if force_generic == 2 else f"{ly.kind}_generic"


def last_weights(ly: Layer, sd: dict) -> list[str]:
    """weight and bias of the last Linear of every conditioner net (RNVP: its two heads)"""
    if ly.kind == "rnvp":
        return ["t.weight", "t.bias", "s.weight", "s.bias"]
    nets = ("s_net", "t_net") if ly.kind == "ahf" else ("f1", "f2")
    return [f"{n}.{O.linear_indices(sd, n)[-1]}.{w}" for n in nets for w in ("weight", "bias")]


# ------------------------------------------------------------------------------------------------------- the fixtures
@functools.lru_cache(maxsize=None)
def fixture(case: Case) -> Fixture:
    """big_cond_rows, big_act_rows, nonfinite_row and the old layers' big_hidden: the gradient table's fixture()."""
    ly, fam = case.layer, case.family
    if fam in ("big_cond_rows", "big_act_rows", "nonfinite_row") or (fam == "big_hidden" and ly.tag in R.BIG_HIDDEN_FACTOR):
        return R.fixture(case)
    sd, x, w_y, w_l, mask = R.base_inputs(ly)
    fx = Fixture(case, sd, x, w_y, w_l, mask)
    if fam == "base":
        pass
    elif fam == "big_second_rows":  # forward: f2 reads the big half back from y; inverse: from x, in the first half-step
        big = big_rows_of(ly.rows)
        x[list(big), ly.dim // 2:] *= BIG_ROWS
        fx.sd = scaled(sd, {"f2.0.weight": 1e-4})
        fx.special = big
    elif fam == "big_hidden":
        f = BIG_HIDDEN_FACTOR[ly.tag]
        fx.sd = scaled(sd, {**{k: f for k in R.first_weights(ly)}, **{k: 1.0 / f for k in R.next_weights(ly)}})
    elif fam == "big_heads":
        fx.sd = scaled(sd, {k: BIG_HEADS_GAIN[ly.tag] for k in last_weights(ly, sd)})
    else:
        raise ValueError(fam)
    return fx


def base_rows(fx: Fixture) -> torch.Tensor:
    """the batch with the special rows put back to their values in the base case"""
    x = fx.x.clone()
    if fx.special:
        x[list(fx.special)] = R.base_inputs(fx.case.layer)[1][list(fx.special)]
    return x


def evaluate(case: Case, sd: dict, x: torch.Tensor, mask, dt) -> tuple:
    ly, p, x = case.layer, {k: v.to(dt) for k, v in sd.items()}, x.to(dt)
    if ly.kind == "ahf":
        return O.affine_half(x, p, ly.parity, case.inverse)
    if ly.kind == "nsf":
        return O.nsf_cl(x, p, ly.shape[0], TAIL, case.inverse)
    return O.rnvp(x, p, mask.to(dt))


@dataclass
class Outputs:
    y32: torch.Tensor
    ld32: torch.Tensor
    y64: torch.Tensor
    ld64: torch.Tensor


@functools.lru_cache(maxsize=None)
def oracle(case: Case) -> Outputs:
    """fp32 and float64 oracle outputs; nonfinite_row: of the batch WITHOUT that row (NSF_CL's oracle asserts on a NaN
    discriminant; rows are independent)."""
    fx = fixture(case)
    keep = fx.ordinary if fx.bad_row is not None else slice(None)
    mask = None if fx.mask is None else fx.mask[keep]
    with torch.no_grad():
        y32, ld32 = evaluate(case, fx.sd, fx.x[keep], mask, torch.float32)
        y64, ld64 = evaluate(case, fx.sd, fx.x[keep], mask, torch.float64)
    return Outputs(y32, ld32, y64, ld64)


def bad_row_finite(fx: Fixture) -> torch.Tensor:
    """Which elements of y in the row with the non-finite conditioner input are finite.  AffineHalfFlow, RNVP: what the
    fp32 oracle gives on that row.  NSF_CL: its oracle cannot run there (a NaN discriminant; bin index -1), so from its
    code: the net that reads the inf returns NaN, every element it transforms inside [-B, B] is NaN, every one outside
    passes through (the inf itself too); forward, f2 then reads those NaN and does the same to the lower half; inverse,
    f2 has run before on finite inputs and the lower half is finite but for the inf."""
    case, ly, r = fx.case, fx.case.layer, fx.bad_row
    row = fx.x[r:r + 1]
    if ly.kind != "nsf":
        with torch.no_grad():
            y, _ = evaluate(case, fx.sd, row, None if fx.mask is None else fx.mask[r:r + 1], torch.float32)
        return torch.isfinite(y[0])
    h = ly.dim // 2
    fin = (row[0].abs() > TAIL) & torch.isfinite(row[0])
    if case.inverse:
        fin[:h] = torch.isfinite(row[0, :h])
    return fin


# --------------------------------------------------------------------- float64: does a case reach the path it is named for
def conditioner_outputs_max(fx: Fixture) -> float:
    """the largest float64 magnitude any conditioner output takes (s, t; the raw spline parameters; RNVP's two heads)"""
    ly, p = fx.case.layer, {k: v.double() for k, v in fx.sd.items()}
    ins = conditioner_inputs(fx)
    if ly.kind == "rnvp":
        y = O.mlp(ins["net"], p, "net")
        heads = [torch.nn.functional.linear(y, p[f"{n}.weight"], p[f"{n}.bias"]) for n in ("t", "s")]
    else:
        heads = [O.mlp(v, p, net) for net, v in ins.items()]
    return max(float(t.abs().max()) for t in heads)


def path_figures(fx: Fixture) -> dict:
    """per conditioner net: the largest magnitude per 16-row tile of its inputs and of its hidden vectors"""
    ly = fx.case.layer
    ins = conditioner_inputs(fx)
    out = {"input_tiles": {net: tile_max(v) for net, v in ins.items()}, "hidden_tiles": {}}
    for net, v in ins.items():
        out["hidden_tiles"][net] = np.maximum.reduce([tile_max(h) for h in mlp_hidden(v, fx.sd, net, ly.kind == "rnvp")])
    out["hidden_all"] = np.maximum.reduce(list(out["hidden_tiles"].values()))
    out["input_all"] = np.maximum.reduce(list(out["input_tiles"].values()))
    return out


# ---------------------------------------------------------------------------------------------------------- the runner
def bits(a: torch.Tensor) -> torch.Tensor:
    return a.contiguous().view(torch.int32)


def same_bits(a: torch.Tensor, b: torch.Tensor, what: str):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert torch.equal(bits(a), bits(b)), f"{what}: {int((bits(a) != bits(b)).sum())} of {a.numel()} elements differ"


def limits(case_id: str) -> dict:
    """keyword arguments of the parity rule for a case: the project's, or (STRESS) twice the VALU kernel's error"""
    if case_id in STRESS:
        return {"rtol": 2.0 * STRESS[case_id], "max_widening": None}
    return {"rtol": RTOL, "max_widening": MAX_WIDENING}


def compare(case_id: str, got, ref32, ref64, what: str, rowwise: bool = False) -> float:
    lim = limits(case_id)
    if case_id in STRESS:  # the budget is the stated figure, without head-room on top
        ref64 = None
    return (assert_row_parity if rowwise else assert_parity)(got, ref32.numpy(), None if ref64 is None else ref64.numpy(),
                                                               what, **lim)


def call(amd, f, fx: Fixture, x: torch.Tensor, want: str):
    """(y, log_det) on the CPU of one pass without gradients; the kernel that ran is the one wanted"""
    ly, inverse = fx.case.layer, fx.case.inverse
    with torch.no_grad():
        if ly.kind == "ahf":
            y, ld = f.forward(x.to(DEV), inverse=inverse)
        elif ly.kind == "nsf":
            y, ld = (f.inverse if inverse else f.forward)(x.to(DEV))
        elif ly.seeded:
            y, ld = f.forward(x.to(DEV), seed=R.RNVP_SEED)
        else:
            y, ld = f.forward(x.to(DEV), mask=fx.mask.to(DEV))
    torch.cuda.synchronize()
    assert amd.last_kernel() == want, (fx.case.id, amd.last_kernel(), want)
    return y.cpu(), ld.cpu()


def passes_through(fx: Fixture, x: torch.Tensor, y: torch.Tensor, what: str):
    ly = fx.case.layer
    if ly.kind == "ahf":
        c = R.cond_columns(ly)
        same_bits(y[:, c], x[:, c], what + ": the conditioning half")
    elif ly.kind == "nsf":
        out = x.abs() > TAIL
        assert bool(out.any()), what
        same_bits(y[out], x[out], what + ": elements beyond the tail bound")


def run_case(amd, case: Case, prefix: str = "", force_generic: int = 2) -> dict:
    """One case on the GPU.  Returns {"y", "log_det", "seconds"} (seconds: the GPU side, module and copies included)."""
    fx, ref = fixture(case), oracle(case)
    ly, what, cid = case.layer, f"{prefix}{case.id}", case.id
    want = kernel_of(ly, force_generic)
    t0 = time.time()
    f = module_of(amd, fx)
    f.force_generic = force_generic
    if ly.seeded:
        assert torch.equal(f.mask_for(R.RNVP_SEED, ly.rows).cpu(), fx.mask), "seeded_mask() is not the library's mask"
    y, ld = call(amd, f, fx, fx.x, want)
    clean = call(amd, f, fx, base_rows(fx), want) if case.family in INDEPENDENT else None
    seconds = time.time() - t0
    keep = fx.ordinary
    special = list(fx.special)
    passes_through(fx, fx.x, y, what)
    if fx.bad_row is not None:
        # the row with the non-finite conditioner input is non-finite where the reference's is; the others do not notice
        fin = bad_row_finite(fx)
        got_fin = torch.isfinite(y[fx.bad_row])
        assert torch.equal(got_fin, fin), f"{what}: y of the bad row is finite in {got_fin.nonzero()[:, 0].tolist()}, " \
                                          f"the reference's in {fin.nonzero()[:, 0].tolist()}"
        assert not bool(torch.isfinite(ld[fx.bad_row])), what
        compare(cid, y[keep], ref.y32, ref.y64, what + " y (other rows)", rowwise=True)
        compare(cid, ld[keep], ref.ld32, ref.ld64, what + " ld (other rows)")
        # (y of the 15 tile neighbours: the row-wise rule above holds each of them on its own maximum already)
        near = R.tile_neighbours(fx.bad_row, ly.rows)
        sub = [r - (r > fx.bad_row) for r in near]  # their rows in the oracle's batch without the bad row
        assert len(near) == 15
        compare(cid, ld[near], ref.ld32[sub], ref.ld64[sub], what + " ld (the 15 tile neighbours)")
    else:
        compare(cid, y, ref.y32, ref.y64, what + " y", rowwise=True)
        compare(cid, ld[keep], ref.ld32[keep], ref.ld64[keep], what + (" ld (ordinary rows)" if special else " ld"))
        if special:
            compare(cid, ld[special], ref.ld32[special], ref.ld64[special], what + " ld (special rows)")
    if clean is not None:
        # csrc/mnf_rt.h takes the down-scale exponent per ROW (max_over_q): a row beyond the range changes nothing in
        # the 15 rows that share its MFMA tile, let alone elsewhere
        same_bits(y[keep], clean[0][keep], what + " y of the ordinary rows, with and without the special rows")
        same_bits(ld[keep], clean[1][keep], what + " ld of the ordinary rows, with and without the special rows")
    return {"y": y, "log_det": ld, "seconds": seconds}


# ------------------------------------------------------------------------------------------------------------ the stack
def stack_inputs():
    """rt_bwd_range_cases.run_fixture()'s three (64, (24, 24)) layers and 2,100 rows; special: the rows beyond 2^13"""
    sds, x, _, _ = R.run_fixture()
    return sds, x, big_rows_of(R.RUN_ROWS)


@functools.lru_cache(maxsize=None)
def stack_oracle() -> dict:
    """dtype -> (every intermediate of the inverse pass, log_det, log p) through the oracle, layer by layer"""
    sds, x, _ = stack_inputs()
    out = {}
    with torch.no_grad():
        for dt in (torch.float32, torch.float64):
            zs, ld = [x.to(dt)], 0
            for i in reversed(range(len(sds))):
                z, l1 = O.affine_half(zs[-1], {k: v.to(dt) for k, v in sds[i].items()}, bool(i % 2), True)
                zs.append(z)
                ld = ld + l1
            out[dt] = (zs, ld, ld + O.std_normal_log_prob(zs[-1]))
        p64 = {f"flows.{i}.{k}": v.double() for i, sd in enumerate(sds) for k, v in sd.items()}
        z, ld = R.run_chain(sds)(x.double(), p64)
    assert torch.equal(z, out[torch.float64][0][-1]) and torch.equal(ld, out[torch.float64][1])
    return out


def run_stack(amd, prefix: str = "") -> dict:
    """The three layers as one ahf_stack_rt launch: every intermediate and log_det against the float64 chain, the
    layer-by-layer route and the rows' independence bit for bit, the fused log-prob epilogue and its fp64 sum."""
    from test_hip_rt_stack import build

    sds, x_cpu, big = stack_inputs()
    n, what, ref = len(sds), f"{prefix}{STACK_ID}", stack_oracle()
    (z32, ld32, lp32), (z64, ld64, lp64) = ref[torch.float32], ref[torch.float64]
    keep = torch.ones(R.RUN_ROWS, dtype=torch.bool)
    keep[list(big)] = False
    special = list(big)
    t0 = time.time()
    fused = build(amd, R.RUN_DIM, R.RUN_HS, n, {}, sds=sds, fused=True, force=2)
    plain = build(amd, R.RUN_DIM, R.RUN_HS, n, {}, sds=sds, fused=False, force=2)
    x = x_cpu.to(DEV)
    x_clean = x_cpu.clone()
    x_clean[special] = R.run_base_x()[special]
    with torch.no_grad():
        zs, ld = fused.inverse(x)
        assert amd.last_kernel() == "ahf_stack_rt", amd.last_kernel()
        zs, ld = [z.cpu() for z in zs], ld.cpu()
        zs0, ld0 = plain.inverse(x)
        assert amd.last_kernel() == "ahf_rt", amd.last_kernel()
        zc, ldc = fused.inverse(x_clean.to(DEV))
        assert amd.last_kernel() == "ahf_stack_rt", amd.last_kernel()
        lp, total = fused.log_prob(x, return_sum=True)
        assert fused._logprob_done and amd.last_kernel() == "ahf_stack_rt"
        lp, total = lp.cpu(), float(total)
    seconds = time.time() - t0
    assert len(zs) == n + 1
    h = R.RUN_DIM // 2
    for k in range(1, n + 1):
        layer = n - k  # the inverse pass meets the last layer first
        c = slice(h, 2 * h) if layer % 2 else slice(0, h)
        same_bits(zs[k][:, c], zs[k - 1][:, c], f"{what} z{k}: the conditioning half")
        compare(STACK_ID, zs[k], z32[k], z64[k], f"{what} z{k}", rowwise=True)
        same_bits(zs[k], zs0[k].cpu(), f"{what} z{k}, fused and layer by layer")
        same_bits(zs[k][keep], zc[k].cpu()[keep], f"{what} z{k} of the ordinary rows, with and without the special rows")
    compare(STACK_ID, ld[keep], ld32[keep], ld64[keep], what + " ld (ordinary rows)")
    compare(STACK_ID, ld[special], ld32[special], ld64[special], what + " ld (special rows)")
    same_bits(ld, ld0.cpu(), what + " ld, fused and layer by layer")
    same_bits(ld[keep], ldc.cpu()[keep], what + " ld of the ordinary rows, with and without the special rows")
    compare(STACK_ID, lp[keep], lp32[keep], lp64[keep], what + " log_prob (ordinary rows)")
    compare(STACK_ID, lp[special], lp32[special], lp64[special], what + " log_prob (special rows)")
    exact = float(lp.double().sum())
    assert abs(total - exact) <= 1e-9 * abs(exact), (what, total, exact)
    return {"zs": zs, "log_det": ld, "log_prob": lp, "seconds": seconds}


def table(records: list[dict]) -> str:
    return R.table(records)
