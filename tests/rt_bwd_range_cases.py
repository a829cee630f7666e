"""The operating range of the run-time-shaped gradient kernels (ahf_bwd_rt, nsf_bwd_rt, rnvp_bwd_rt): the case table and
the runner.  Not collected: tests/test_rt_bwd_range_host.py (CPU: the fixtures are sound and reach the path they are named
for), tests/test_hip_rt_bwd_range.py (GPU, default mode) and tests/rt_deterministic_child.py (MNF_DETERMINISTIC=1) import it,
so that all three look at the same inputs.

The kernels compute in split f16 (head + residual 2^-11) and have no fp32 fix-up pass; what keeps them right outside the
split range is code the round-6 gradient fixtures (inputs and cotangents of scale 1) never execute:

  rescue      the first chain step of a tile whose cotangents reach kSplitLimit = 2^13 rescales its accumulators
  !same       mnf_rt_bwd.h dw_phase_rows: a row block with a wave-tile whose exchange scale is not 1 multiplies every
              product back by sa[w] sb[w] (the bias by sa[w])
  down        exchange_store / split_rows scale a tile / a row down by down_exponent(., 13)
  weights     staged at the top of f16's range (weight_exponent, src.wdown), transposed blocks included
  scale       the gradient scale is a power of two from at most 512 sampled rows: the others may lie far off it

Shapes: the smallest of round 6 that still have several row blocks, a ragged last block, partial 16-column tiles and the
element-wise row path (dim 10, 6, 50: rows that are not 16-byte aligned).  Parameters and inputs: the recipes and seeds of
tests/test_hip_round6.py's gradient tests (AffineHalfFlow inputs from seed 232 + dim: see the remark there)."""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np
import torch

import recipes
from oracle import flow_oracle as O
from test_hip_autograd import GBASE, GBASE_STRESS, OracleGrads, check_vs_float64
from recipes import rnvp_params_layers as _rnvp_sd

DEV = "cuda"
LIMIT = 2.0 ** 13   # mnf_rt.h kSplitLimit; down_exponent(v, 13) is 0 below it
SAMPLE = 512        # rows mnf_affine_half_grad_scale looks at (include/mnf_hip.h): rows s * (rows // 512)
OUTLIER = 2.0 ** 17  # over a unit cotangent: 2^17 / 2^2 (the sample's maximum, ~4, is brought into [1, 2)) >= 2^13
BIG_ROWS = 3.0e4
RNVP_SEED = 77
BAD_ROW = 37        # tile 2 (rows 32 .. 47)


@dataclass(frozen=True)
class Layer:
    tag: str
    kind: str      # "ahf" | "nsf" | "rnvp"
    dim: int
    shape: tuple   # ahf, rnvp: hidden widths; nsf: (K, n_h)
    rows: int
    parity: bool = False
    seeded: bool = False

    @property
    def kernel(self) -> str:
        return f"{self.kind}_bwd_rt"


LAYERS = [
    Layer("ahf64", "ahf", 64, (24, 24), 2100, parity=False),
    Layer("ahf10", "ahf", 10, (16, 40), 300, parity=True),
    Layer("nsf50", "nsf", 50, (10, 12), 700),
    Layer("nsf6", "nsf", 6, (3, 5), 700),
    Layer("rnvp50", "rnvp", 50, (100,), 700),
    Layer("rnvp64", "rnvp", 64, (7, 9, 11), 700, seeded=True),
]

# big_hidden: first-layer weights x f, the next layer's / f.  f = 3000 where that puts the first hidden vector at or
# beyond 2^13 in some 16-row tiles and below it in others (the host test holds every entry to that).  A pre-activation
# is ~N(0, (0.58 f)^2) here (nn.Linear's init range on unit inputs), so 2^13 is 4.7 sigma away at f = 3000: NSF_CL,
# whose inputs are drawn at scale 1.4, has 8 and 14 of its 44 tiles there, but the largest hidden magnitude of the whole
# batch is 7,119 / 7,983 for the AffineHalfFlow shapes and 8,140 / 6,849 for the RNVP ones (masked inputs) -- no tile
# leaves the split range.  There f is raised until a tile's maximum (3 .. 3.5 sigma) straddles the limit: 59 of 132, 11
# of 19, 14 of 44 and 10 of 44 tiles at or beyond 2^13.  The float64 oracle stays finite at every one of them.
BIG_HIDDEN_FACTOR = {"ahf64": 4500.0, "ahf10": 4500.0, "nsf50": 3000.0, "nsf6": 3000.0, "rnvp50": 3500.0, "rnvp64": 4500.0}

FAMILIES = ["cot_small", "cot_large", "cot_outlier", "cot_y_only", "cot_ld_only", "big_cond_rows", "big_act_rows",
            "big_hidden", "nonfinite_row"]


@dataclass(frozen=True)
class Case:
    layer: Layer
    family: str
    inverse: bool = False

    @property
    def id(self) -> str:
        d = "" if self.layer.kind == "rnvp" else ("-inv" if self.inverse else "-fwd")
        return f"{self.layer.tag}{d}-{self.family}"


def _cases() -> list[Case]:
    out = []
    for ly in LAYERS:
        for inverse in ((False,) if ly.kind == "rnvp" else (False, True)):
            for fam in FAMILIES:
                if fam == "cot_outlier" and ly.rows < SAMPLE:  # every row is sampled
                    continue
                if fam == "big_act_rows" and ly.kind != "ahf":
                    continue
                out.append(Case(ly, fam, inverse))
    return out


CASES = _cases()
CASE_IDS = [c.id for c in CASES]
RUN_ID = "run-ahf64x3-weighted_nll"

# Cases a correct kernel cannot hold within 80 % of GBASE + widening: id -> the measured error (base = GBASE_STRESS there;
# profiles/r9/rt_bwd_range.txt: each case's worst comparison, both sum modes).  The cot_* families never belong here.
STRESS: dict[str, float] = {}


def base_of(case_id: str) -> float:
    return GBASE_STRESS if case_id in STRESS else GBASE


# ------------------------------------------------------------------------------------------- the header's sampling rule
def sampled_rows(rows: int) -> np.ndarray:
    sample = min(rows, SAMPLE)
    stride = rows // sample if sample else 1
    return np.arange(sample) * stride


def unsampled_mask(rows: int) -> np.ndarray:
    m = np.ones(rows, dtype=bool)
    m[sampled_rows(rows)] = False
    return m


def grad_scale(w_y, w_l) -> float:
    """mnf_affine_half_grad_scale in float64: the power of two that brings the sampled rows' largest |cotangent| into
    [1, 2); 1 for an all-zero sample."""
    rows = (w_y if w_y is not None else w_l).shape[0]
    s = sampled_rows(rows)
    m = 0.0
    if w_y is not None:
        m = max(m, float(w_y.double()[s].abs().max()))
    if w_l is not None:
        m = max(m, float(w_l.double()[s].abs().max()))
    if not (0.0 < m < float("inf")):
        return 1.0
    _, e = np.frexp(m)  # m = f 2^e, f in [0.5, 1)
    return float(2.0 ** (1 - int(e)))


def seeded_mask(seed: int, rows: int, dim: int) -> torch.Tensor:
    """csrc/mnf_device.h rnvp_mask_bit for seeds and row counts below 2^32 (the GPU test compares it with RNVP.mask_for)."""
    def mix32(h):
        h = h ^ (h >> np.uint64(16))
        h = (h * np.uint64(0x85ebca6b)) & M
        h = h ^ (h >> np.uint64(13))
        h = (h * np.uint64(0xc2b2ae35)) & M
        return h ^ (h >> np.uint64(16))

    M = np.uint64(0xffffffff)
    row = np.arange(rows, dtype=np.uint64)[:, None]
    col = np.arange(dim, dtype=np.uint64)[None, :]
    a = mix32((row * np.uint64(0x9e3779b1)) & M)
    word = mix32(a ^ (((col >> np.uint64(5)) * np.uint64(0x85ebca77) + np.uint64(seed)) & M))
    return torch.from_numpy(((word >> (col & np.uint64(31))) & np.uint64(1)).astype(np.float32))


# ------------------------------------------------------------------------------------------------------- the fixtures
@dataclass
class Fixture:
    case: Case
    sd: dict
    x: torch.Tensor
    w_y: torch.Tensor | None
    w_l: torch.Tensor | None
    mask: torch.Tensor | None = None
    special: tuple = ()   # rows that carry the case's outliers / big inputs / the non-finite input
    bad_row: int | None = None

    @property
    def ordinary(self) -> torch.Tensor:
        keep = torch.ones(self.x.shape[0], dtype=torch.bool)
        keep[list(self.special)] = False
        return keep

    def fn(self):
        """(x, params) -> (y, log_det) through the oracle"""
        ly, inverse, mask = self.case.layer, self.case.inverse, self.mask
        if ly.kind == "ahf":
            return lambda x, p: O.affine_half(x, p, ly.parity, inverse)
        if ly.kind == "nsf":
            return lambda x, p: O.nsf_cl(x, p, ly.shape[0], 3.0, inverse)
        return lambda x, p: O.rnvp(x, p, mask.to(x.dtype))

    def loss(self, w_y=None, w_l=None):
        fn = self.fn()
        w_y = self.w_y if w_y is None else w_y
        w_l = self.w_l if w_l is None else w_l

        def loss(x, p, dt):
            y, ld = fn(x, p)
            total = 0
            if w_y is not None:
                total = total + (y * w_y.to(dt)).sum()
            if w_l is not None:
                total = total + (ld * w_l.to(dt)).sum()
            return total
        return loss


def first_weights(ly: Layer, nets=None) -> list[str]:
    nets = nets or {"ahf": ("s_net", "t_net"), "nsf": ("f1", "f2"), "rnvp": ("net",)}[ly.kind]
    return [f"{n}.0.weight" for n in nets]


def next_weights(ly: Layer) -> list[str]:
    if ly.kind == "rnvp":
        return ["net.2.weight"] if len(ly.shape) > 1 else ["t.weight", "s.weight"]  # (one layer: both heads read it)
    return [f"{n}.2.weight" for n in (("s_net", "t_net") if ly.kind == "ahf" else ("f1", "f2"))]


def cond_columns(ly: Layer) -> slice:
    """the columns the FIRST conditioner of the layer reads in x (NSF_CL: f1 reads the lower half in both directions --
    the inverse's second half-step sees the lower half the first one passed through, unchanged beyond the tail bound)"""
    h = ly.dim // 2
    if ly.kind == "ahf":
        return slice(h, ly.dim) if ly.parity else slice(0, h)
    return slice(0, h) if ly.kind == "nsf" else slice(0, ly.dim)


def act_columns(ly: Layer) -> slice:
    h = ly.dim // 2
    return slice(0, h) if ly.parity else slice(h, ly.dim)


def big_rows_of(rows: int) -> tuple:
    return (3, 40, 41, rows - 1)  # two tiles, two rows of one tile, the ragged last tile


def outlier_rows_of(rows: int) -> tuple:
    """(row of the w_y outlier, row of the w_l outlier): r % (rows // 512) != 0, and the last row (beyond the sample)"""
    return (1001, rows - 1) if rows >= 2048 else (600, rows - 1)


def base_inputs(ly: Layer):
    rows, dim = ly.rows, ly.dim
    mask = None
    if ly.kind == "ahf":
        sd = recipes.affine_half_params(31 + dim, dim, h_sizes=ly.shape, s_last_gain=2.0)
        x = recipes.gaussian(232 + dim, rows, dim)
        w_y, w_l = recipes.gaussian(33, rows, dim), recipes.gaussian(34, rows, 1)[:, 0]
    elif ly.kind == "nsf":
        K, n_h = ly.shape
        sd = recipes.nsf_cl_params(51 + dim + K, dim, K, n_h)
        x = recipes.gaussian(52 + dim, rows, dim, scale=1.4)
        w_y, w_l = recipes.gaussian(53, rows, dim), recipes.gaussian(54, rows, 1)[:, 0]
    else:
        sd = _rnvp_sd(41 + dim, dim, ly.shape)
        x = recipes.gaussian(42 + dim, rows, dim)
        w_y, w_l = recipes.gaussian(43, rows, dim), recipes.gaussian(44, rows, 1)[:, 0]
        mask = seeded_mask(RNVP_SEED, rows, dim) if ly.seeded else recipes.bernoulli_mask(97, rows, dim)
    return sd, x.clone(), w_y.clone(), w_l.clone(), mask


def scaled(sd: dict, factors: dict) -> dict:
    return {k: (v * factors[k] if k in factors else v) for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def fixture(case: Case) -> Fixture:
    ly, fam = case.layer, case.family
    rows = ly.rows
    sd, x, w_y, w_l, mask = base_inputs(ly)
    fx = Fixture(case, sd, x, w_y, w_l, mask)
    if fam == "cot_small":  # a mean over many rows; rows beyond the sample larger than anything in it
        far = torch.from_numpy(unsampled_mask(rows))
        fx.w_y, fx.w_l = w_y * 1e-7, w_l * 1e-7
        fx.w_y[far] *= 37.0
        fx.w_l[far] *= 37.0
    elif fam == "cot_large":
        fx.w_y, fx.w_l = w_y * 40.0, w_l * 40.0
    elif fam == "cot_outlier":
        r_y, r_l = outlier_rows_of(rows)
        w_y[r_y] *= OUTLIER
        w_l[r_l] = float(np.copysign(OUTLIER, float(w_l[r_l])))
        fx.special = (r_y, r_l)
    elif fam == "cot_y_only":
        fx.w_l = None
    elif fam == "cot_ld_only":
        fx.w_y = None
    elif fam == "big_cond_rows":
        big = big_rows_of(rows)
        x[list(big), cond_columns(ly)] *= BIG_ROWS
        # (NSF_CL: f1 alone reads the big half; f2 keeps its weights, its inputs are the transformed half)
        nets = ("f1",) if ly.kind == "nsf" else None
        fx.sd = scaled(sd, {k: 1e-4 for k in first_weights(ly, nets)})
        fx.special = big
    elif fam == "big_act_rows":
        big = big_rows_of(rows)
        x[list(big), act_columns(ly)] *= BIG_ROWS
        fx.special = big
    elif fam == "big_hidden":
        f = BIG_HIDDEN_FACTOR[ly.tag]
        fx.sd = scaled(sd, {**{k: f for k in first_weights(ly)}, **{k: 1.0 / f for k in next_weights(ly)}})
    elif fam == "nonfinite_row":
        c = cond_columns(ly)
        col = c.start + 1
        if ly.kind == "rnvp":  # a column the mask lets through to the conditioner
            col = int(torch.nonzero(mask[BAD_ROW])[0])
        x[BAD_ROW, col] = float("inf")
        fx.special, fx.bad_row = (BAD_ROW,), BAD_ROW
    else:
        raise ValueError(fam)
    return fx


@functools.lru_cache(maxsize=None)
def oracle(case: Case) -> OracleGrads:
    """fp32 and float64 oracle gradients of the case; nonfinite_row: of the batch WITHOUT that row (the loss is a sum over
    rows, so the other rows' grad_x is what it is in the whole batch)."""
    fx = fixture(case)
    if fx.bad_row is None:
        return OracleGrads(fx.loss(), fx.x, fx.sd)
    keep = fx.ordinary
    sub = Fixture(case, fx.sd, fx.x[keep], None if fx.w_y is None else fx.w_y[keep], None if fx.w_l is None else fx.w_l[keep],
                  None if fx.mask is None else fx.mask[keep])
    return OracleGrads(sub.loss(), sub.x, sub.sd)


# --------------------------------------------------------------------- float64: does a case reach the path it is named for
def mlp_hidden(x: torch.Tensor, sd: dict, prefix: str, last_is_hidden: bool) -> list[torch.Tensor]:
    """the hidden vectors of oracle.mlp (after the activation; RNVP's net ends in one without activation)"""
    ids = O.linear_indices(sd, prefix)
    out = []
    for n, i in enumerate(ids):
        x = torch.nn.functional.linear(x, sd[f"{prefix}.{i}.weight"].double(), sd[f"{prefix}.{i}.bias"].double())
        if n + 1 < len(ids):
            x = torch.nn.functional.leaky_relu(x, O.LEAKY_SLOPE)
            out.append(x)
        elif last_is_hidden:
            out.append(x)
    return out


def tile_max(v: torch.Tensor) -> np.ndarray:
    """the largest finite magnitude per 16-row tile of a (rows, n) tensor"""
    a = v.detach().double().abs()
    a = torch.where(torch.isfinite(a), a, torch.zeros_like(a)).max(dim=1).values.numpy()
    pad = (-len(a)) % 16
    return np.pad(a, (0, pad)).reshape(-1, 16).max(axis=1)


def straddles(tiles: np.ndarray) -> bool:
    """at or beyond 2^13 in at least one 16-row tile, below it in at least one other"""
    return bool((tiles >= LIMIT).any() and (tiles < LIMIT).any())


def conditioner_inputs(fx: Fixture) -> dict:
    """net -> its float64 input rows"""
    ly, x = fx.case.layer, fx.x.double()
    h = ly.dim // 2
    if ly.kind == "ahf":
        c = x[:, cond_columns(ly)]
        return {"s_net": c, "t_net": c}
    if ly.kind == "rnvp":
        return {"net": fx.mask.double() * x}
    y, _ = fx.fn()(x, {k: v.double() for k, v in fx.sd.items()})
    fwd = not fx.case.inverse
    return {"f1": (x if fwd else y)[:, :h], "f2": (y if fwd else x)[:, h:]}


def conditioner_output_cotangents(fx: Fixture) -> torch.Tensor:
    """Per row, the largest float64 |d loss / d (a conditioner output)|: what the kernels' first chain step splits (g_s,
    g_t of AffineHalfFlow; the spline parameters' cotangents of both NSF_CL half-steps; RNVP's shift and scale heads)."""
    x = fx.x.double().requires_grad_(True)
    p = {k: v.double() for k, v in fx.sd.items()}
    seen = []

    def keep(t):
        t.retain_grad()
        seen.append(t)
        return t

    if fx.case.layer.kind == "rnvp":  # oracle.rnvp, with its two heads kept
        m, F = fx.mask.double(), torch.nn.functional
        y = O.mlp(m * x, p, "net")
        shift, scale = keep(F.linear(y, p["t.weight"], p["t.bias"])), keep(F.linear(y, p["s.weight"], p["s.bias"]))
        gate = torch.sigmoid(scale)
        out, ld = ((1 - m) * x * gate + (1 - gate) * shift) + m * x, ((1 - m) * gate.log()).sum(1)
        (out * fx.w_y.double()).sum().add((ld * fx.w_l.double()).sum()).backward()
    else:
        mlp = O.mlp
        O.mlp = lambda xx, pp, prefix: keep(mlp(xx, pp, prefix))
        try:
            fx.loss()(x, p, torch.float64).backward()
        finally:
            O.mlp = mlp
    rows = x.shape[0]
    return torch.stack([t.grad.reshape(rows, -1).abs().max(dim=1).values for t in seen]).max(dim=0).values


def path_figures(fx: Fixture) -> dict:
    """what the host test asserts on, computed in float64"""
    ly, fam = fx.case.layer, fx.case.family
    out = {"scale": grad_scale(fx.w_y, fx.w_l)}
    if fam == "cot_outlier":
        r_y, r_l = fx.special
        far = unsampled_mask(ly.rows)
        out["outliers_unsampled"] = bool(far[r_y] and far[r_l])
        out["outlier_y"] = float(fx.w_y[r_y].double().abs().max()) * out["scale"]
        out["outlier_l"] = abs(float(fx.w_l[r_l])) * out["scale"]
        cot = conditioner_output_cotangents(fx) * out["scale"]
        out["outlier_y_at_net"], out["outlier_l_at_net"] = float(cot[r_y]), float(cot[r_l])
        out["others_at_net"] = float(cot[fx.ordinary].max())
    if fam in ("big_cond_rows", "big_hidden"):
        ins = conditioner_inputs(fx)
        out["input_tiles"] = np.maximum.reduce([tile_max(v) for v in ins.values()])
        hid = []
        for net, v in ins.items():
            hid += [tile_max(hv) for hv in mlp_hidden(v, fx.sd, net, ly.kind == "rnvp")]
        out["hidden_tiles"] = np.maximum.reduce(hid)
    if fam == "big_act_rows":
        x = fx.x.double()
        v = x[:, act_columns(ly)]
        out["input_tiles"] = tile_max(v)
        # the scale net's output cotangent, in units of the gradient scale: forward g e^s v + g_ld, inverse -g y - g_ld
        s = O.mlp(x[:, cond_columns(ly)], {k: p.double() for k, p in fx.sd.items()}, "s_net")
        y, _ = fx.fn()(x, {k: p.double() for k, p in fx.sd.items()})
        g = fx.w_y.double()[:, act_columns(ly)]
        gl = fx.w_l.double()[:, None]
        g_s = (-g * y[:, act_columns(ly)] - gl) if fx.case.inverse else (g * s.exp() * v + gl)
        out["g_s_tiles"] = tile_max(g_s) * out["scale"]
    return out


# ---------------------------------------------------------------------------------------------------------- the runner
def module_of(amd, fx: Fixture):
    ly = fx.case.layer
    if ly.kind == "ahf":
        f = amd.AffineHalfFlow(ly.dim, ly.parity, h_sizes=ly.shape)
    elif ly.kind == "nsf":
        f = amd.NSF_CL(ly.dim, K=ly.shape[0], B=3, n_h=ly.shape[1])
    else:
        f = amd.RNVP(ly.dim, h_sizes=ly.shape)
    f.load_state_dict(fx.sd)
    f.force_generic = 2  # include/mnf_hip.h: the run-time-shaped kernel whatever the shape's specialised kernels
    return f.to(DEV)


def gpu_grads(amd, fx: Fixture, force_generic: int = 2):
    """(gradients {"x", parameter names}, name of the gradient kernel) of one backward pass on the GPU"""
    ly, inverse = fx.case.layer, fx.case.inverse
    f = module_of(amd, fx)
    f.force_generic = force_generic
    x = fx.x.detach().to(DEV).requires_grad_(True)
    if ly.kind == "ahf":
        y, ld = f.forward(x, inverse=inverse)
    elif ly.kind == "nsf":
        y, ld = (f.inverse if inverse else f.forward)(x)
    elif ly.seeded:
        assert torch.equal(f.mask_for(RNVP_SEED, ly.rows).cpu(), fx.mask), "seeded_mask() is not the library's mask"
        y, ld = f.forward(x, seed=RNVP_SEED)
    else:
        y, ld = f.forward(x, mask=fx.mask.to(DEV))
    terms = ([(y * fx.w_y.to(DEV)).sum()] if fx.w_y is not None else []) + \
            ([(ld * fx.w_l.to(DEV)).sum()] if fx.w_l is not None else [])
    sum(terms).backward()
    torch.cuda.synchronize()
    return {"x": x.grad, **{n: q.grad for n, q in f.named_parameters()}}, amd.last_kernel()


def tile_neighbours(row: int, rows: int) -> list[int]:
    return [r for r in range(16 * (row // 16), min(16 * (row // 16) + 16, rows)) if r != row]


def run_case(amd, case: Case, prefix: str = "", force_generic: int = 2) -> dict:
    """One case on the GPU: kernel name, every gradient within the audited budget of the float64 oracle, grad_x of the
    ordinary rows within it on their own norm.  Returns the gradients."""
    fx, ref = fixture(case), oracle(case)
    base, what = base_of(case.id), f"{prefix}{case.id}"
    got, kernel = gpu_grads(amd, fx, force_generic)
    want = case.layer.kernel if force_generic == 2 else case.layer.kernel.replace("_rt", "_generic")
    assert kernel == want, (what, kernel)
    keep = fx.ordinary
    r32, r64 = ref.g[torch.float32]["x"], ref.g[torch.float64]["x"]
    gx = got["x"].detach().cpu()
    if fx.bad_row is not None:
        # the row with the non-finite conditioner input is the reference's business (inf or NaN there, and in every sum
        # over the rows); the OTHER rows' grad_x is row-local and must not notice -- the 15 rows that share its MFMA
        # tile least of all
        assert bool(torch.isfinite(gx[keep]).all()), what
        check_vs_float64(gx[keep], r32, r64, what + " grad x (other rows)", base)
        near = tile_neighbours(fx.bad_row, case.layer.rows)
        sub = [r - (r > fx.bad_row) for r in near]  # their rows in the oracle's batch without the bad row
        assert len(near) == 15
        check_vs_float64(gx[near], r32[sub], r64[sub], what + " grad x (the 15 tile neighbours)", base)
        return got
    ref.check_all(got, what, base=base)
    if fx.special:  # a normwise bound over all rows lets an outlier row's magnitude hide errors everywhere else
        check_vs_float64(gx[keep], r32[keep], r64[keep], what + " grad x (ordinary rows)", base)
    return got


# --------------------------------------------------------------------------------------------- the one-node training run
RUN_DIM, RUN_HS, RUN_LAYERS, RUN_ROWS = 64, (24, 24), 3, 2100
RUN_OUTLIER_ROW = 1001


def run_base_x() -> torch.Tensor:
    """the run's input rows before any of them is scaled"""
    return recipes.gaussian(232 + RUN_DIM, RUN_ROWS, RUN_DIM).clone()


@functools.lru_cache(maxsize=None)
def run_fixture():
    """Three (64, (24, 24)) layers of alternating parity at 2,100 rows; the loss -sum_r w_r log p(x_r) with row weights
    ~1 / rows and one unsampled row at 2^17 times that; a few rows whose lower half (the conditioner input of layers 0
    and 2, the transformed half of layer 1) is x 3e4, first-layer weights x 1e-4."""
    from test_hip_rt_train_run import state_dicts

    sds = state_dicts(RUN_DIM, RUN_HS, RUN_LAYERS, {})
    sds = [scaled(sd, {"s_net.0.weight": 1e-4, "t_net.0.weight": 1e-4}) for sd in sds]
    x = run_base_x()
    big = big_rows_of(RUN_ROWS)
    x[list(big), :RUN_DIM // 2] *= BIG_ROWS
    w = (0.5 + recipes.gaussian(35, RUN_ROWS, 1)[:, 0].abs()) / RUN_ROWS
    w[RUN_OUTLIER_ROW] *= OUTLIER
    return sds, x, w, (*big, RUN_OUTLIER_ROW)


def run_chain(sds):
    def chain(x, p):
        ld = 0
        for i in reversed(range(len(sds))):
            x, l1 = O.affine_half(x, {k: p[f"flows.{i}.{k}"] for k in sds[i]}, bool(i % 2), True)
            ld = ld + l1
        return x, ld
    return chain


@functools.lru_cache(maxsize=None)
def run_oracle() -> OracleGrads:
    sds, x, w, _ = run_fixture()
    chain = run_chain(sds)

    def wnll(xx, p, dt):
        z, ld = chain(xx, p)
        return -((ld + O.std_normal_log_prob(z)) * w.to(dt)).sum()

    return OracleGrads(wnll, x, {f"flows.{i}.{k}": v for i, sd in enumerate(sds) for k, v in sd.items()})


def run_gpu_grads(amd, switch: bool):
    from test_hip_rt_train_run import build, grads_of

    sds, x_cpu, w, _ = run_fixture()
    model = build(amd, RUN_DIM, RUN_HS, RUN_LAYERS, {}, sds, switch, force=2)
    x = x_cpu.to(DEV).requires_grad_(True)
    lp = model.log_prob(x)
    k_fwd = amd.last_kernel()
    (-(lp * w.to(DEV)).sum()).backward()
    torch.cuda.synchronize()
    return grads_of(model, x), k_fwd, amd.last_kernel()


def run_the_run(amd, prefix: str = "") -> dict:
    """Both routes against the float64 oracle chain; x.grad of the two bit for bit."""
    ref = run_oracle()
    _, _, _, special = run_fixture()
    keep = torch.ones(RUN_ROWS, dtype=torch.bool)
    keep[list(special)] = False
    base = base_of(RUN_ID)
    got = {}
    for switch in (True, False):
        what = f"{prefix}{RUN_ID} fuse_rt_training={switch}"
        g, k_fwd, k_bwd = run_gpu_grads(amd, switch)
        assert (k_fwd, k_bwd) == (("ahf_stack_rt", "ahf_bwd_stack_rt") if switch else ("ahf_rt", "ahf_bwd_rt")), (what, k_fwd, k_bwd)
        ref.check_all(g, what, base=base)
        gx = g["x"].detach().cpu()
        check_vs_float64(gx[keep], ref.g[torch.float32]["x"][keep], ref.g[torch.float64]["x"][keep],
                         what + " grad x (ordinary rows)", base)
        got[switch] = g
    a, b = got[True]["x"].contiguous().view(torch.int32), got[False]["x"].contiguous().view(torch.int32)
    assert torch.equal(a, b), f"{prefix}{RUN_ID}: x.grad of the two routes differs in {int((a != b).sum())} of {a.numel()} elements"
    return got


def table(records: list[dict]) -> str:
    """one line per recorded comparison: error, budget, share used"""
    lines = [f"{'err':>10s} {'budget':>10s} {'widening':>10s} {'used':>6s}  what"]
    for r in records:
        lines.append(f"{r['err']:10.2e} {r['budget']:10.2e} {r['widening']:10.2e} {100 * r['err'] / r['budget']:5.0f}%  "
                     f"{'[stress] ' if r.get('stress') else ''}{r['what']}")
    return "\n".join(lines)
