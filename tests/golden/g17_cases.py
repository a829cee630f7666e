"""Fixture G17's case table: what gen_golden.g17_rt_grads() runs through the reference and what the tests rebuild.

Everything here is a recipe draw (``recipes.py``): a case is a few integers, and the fixture files carry the reference's
gradients and loss values only.  Rows = 333 everywhere: 20 full 16-row tiles and a 13-row tail.

Single layers: loss = sum(y * w_y) + sum(log_det * w_l), w_y = gaussian / (rows * dim), w_l = gaussian / rows.
Models: loss = -(base.log_prob(zs[-1]) + log_det).mean() after model.inverse(x).

The fixture is split by layer kind into four files (``PARTS``), so that each stays below the 1 MiB limit of a committed
file; the reference's float64 gradients are stored rounded to float32 (2^-24 relative: far below the 1e-5 rule), as
G5 and G6 store their float64 outputs."""
from __future__ import annotations

import recipes

ROWS = 333

# tag -> (dim, h_sizes, constructor keywords, parity, inverse)
AHF = {
    "ahf_d64_h24x24_inv": (64, (24, 24), {}, False, True),
    "ahf_d6_h8x24x17_fwd": (6, (8, 24, 17), {}, True, False),
    "ahf_d130_noshift_inv": (130, (24, 24, 24), {"shift": False}, True, True),
    "ahf_d10_h16x40_inv": (10, (16, 40), {}, True, True),
}
# tag -> (dim, K, n_h, inverse); B = 3, input scale 1.4
NSF = {
    "nsf_d6_K5_h8_inv": (6, 5, 8, True),
    "nsf_d128_K8_h8_inv": (128, 8, 8, True),
    "nsf_d50_K10_h12_fwd": (50, 10, 12, False),
}
NSF_INPUT_SCALE = 1.4
# tag -> (dim, h_sizes)
RNVP = {
    "rnvp_d50_h100": (50, (100,)),
    "rnvp_d100_h41": (100, (41,)),
    "rnvp_d64_h7x9x11": (64, (7, 9, 11)),
}
# tag -> (dim, inverse)
GLOW = {"glow_d48_fwd": (48, False), "glow_d48_inv": (48, True)}
# the 4-layer AffineHalfFlow run and the [ActNormFlow, Glow, NSF_CL] block
RUN = {"run_ahf4_d10": (10, (16, 40), 4)}
RUN_S_LAST_GAIN = 1.0  # (the recipe's default 4.0 sends -mean log p of four layers to 1e16)
BLOCK = {"block_d6_K5_h8": (6, 5, 8)}

KINDS = {"ahf": AHF, "nsf": NSF, "rnvp": RNVP, "glow": GLOW, "run": RUN, "block": BLOCK}
# fixture file -> the kinds it holds
PARTS = {"g17_rt_grads_ahf": ("ahf",), "g17_rt_grads_nsf": ("nsf",), "g17_rt_grads_rnvp": ("rnvp",),
         "g17_rt_grads_models": ("glow", "run", "block")}
SINGLE_LAYER_KINDS = ("ahf", "nsf", "rnvp", "glow")


def kind_of(tag: str) -> str:
    return next(k for k, table in KINDS.items() if tag in table)


def part_of(tag: str) -> str:
    kind = kind_of(tag)
    return next(name for name, kinds in PARTS.items() if kind in kinds)


def all_tags() -> list[str]:
    return [tag for table in KINDS.values() for tag in table]


def seed_of(tag: str) -> int:
    """1700 + 20 * (position in the table): parameters at +0 (a model's layer i at +i, its ActNorm at +8, its Glow at
    +9), x at +10, w_y at +11, w_l at +12, the RNVP mask at +13."""
    return 1700 + 20 * all_tags().index(tag)


def inputs(tag: str) -> dict:
    """x, and for the single layers the loss weights w_y and w_l (and RNVP's mask): float32 CPU tensors."""
    kind, seed = kind_of(tag), seed_of(tag)
    dim = KINDS[kind][tag][0]
    out = {"x": recipes.gaussian(seed + 10, ROWS, dim, scale=NSF_INPUT_SCALE if kind == "nsf" else 1.0)}
    if kind in SINGLE_LAYER_KINDS:
        out["w_y"] = recipes.gaussian(seed + 11, ROWS, dim) / (ROWS * dim)
        out["w_l"] = recipes.gaussian(seed + 12, ROWS, 1)[:, 0] / ROWS
    if kind == "rnvp":
        out["mask"] = recipes.bernoulli_mask(seed + 13, ROWS, dim)
    return out


def params(tag: str):
    """The case's parameters: a state_dict for a single layer (Glow: P, L, S, U), a list of state_dicts in model order
    for the two models."""
    kind, seed = kind_of(tag), seed_of(tag)
    spec = KINDS[kind][tag]
    if kind == "ahf":
        dim, hs, kw, _, _ = spec
        return recipes.affine_half_params(seed, dim, h_sizes=hs, s_last_gain=2.0, **kw)
    if kind == "nsf":
        dim, K, n_h, _ = spec
        return recipes.nsf_cl_params(seed, dim, K, n_h)
    if kind == "rnvp":
        dim, hs = spec
        return recipes.rnvp_params_layers(seed, dim, hs)
    if kind == "glow":
        return recipes.glow_params(seed, spec[0])
    if kind == "run":
        dim, hs, n = spec
        return [recipes.affine_half_params(seed + i, dim, h_sizes=hs, s_last_gain=RUN_S_LAST_GAIN) for i in range(n)]
    dim, K, n_h = spec
    return [recipes.actnorm_params(seed + 8, dim), recipes.glow_params(seed + 9, dim), recipes.nsf_cl_params(seed, dim, K, n_h)]


def grad_names(tag: str) -> list[str]:
    """Names of the gradients the fixture holds for the case, "x" first: the layer's state_dict keys (Glow: L, S, U);
    ``flows.{i}.{key}`` for the models."""
    kind, p = kind_of(tag), params(tag)
    if kind == "glow":
        return ["x", "L", "S", "U"]
    if kind in SINGLE_LAYER_KINDS:
        return ["x", *p]
    names = ["x"]
    for i, sd in enumerate(p):
        names += [f"flows.{i}.{k}" for k in sd if k != "P"]
    return names
