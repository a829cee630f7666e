"""The run-time-shaped tier (csrc/mnf_rt.h, mnf_linear_mfma.hip; ``force_generic = 2``) against numbers the REAL
reference produced: the stack fixtures G1, G3, G6 and G9 with every layer on the tier, and fixture G17 -- the reference's
own autograd gradients (tests/golden/g17_cases.py) -- on every tier a case has.  The single-layer output fixtures (G2,
G5, G7, G10) run on the tier through tests/test_hip_parity.py's "rt" parametrisations.

Every comparison prints one line (tier, kernel family, error, budget, share used): ``pytest -s`` shows them, and
profiles/r12/rt_golden.txt is those lines from one session."""
import numpy as np
import pytest
import torch

import g17_cases as C
import recipes
import rt_golden_cases as RG
from helpers import PARITY_LOG, RTOL, assert_close, assert_parity, c2_layers, g1_layers, t
from test_hip_parity import build_c3

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def amd():
    import torch_mnf_amd

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    torch_mnf_amd._lib.load()
    return torch_mnf_amd


def close(got, ref, what, family, ref64=None):
    """helpers.assert_close at the project's 1e-5 (assert_parity where the fixture carries the reference's float64 run),
    recorded"""
    if ref64 is not None:
        try:
            assert_parity(got, ref, ref64, f"rt golden [{family}] {what}")
        finally:
            r = PARITY_LOG[-1]
            RG.record("rt", family, what, r["err"], r["budget"])
        return
    from helpers import normwise_err

    g = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    RG.record("rt", family, what, normwise_err(g, np.asarray(ref)), RTOL)
    assert_close(got, ref, RTOL, what)


def close_scalar(got, ref, what, family):
    RG.record("rt", family, what, abs(got - ref) / abs(ref), RTOL)
    assert abs(got - ref) <= RTOL * abs(ref), (what, got, ref)


def bits(a):
    return a.contiguous().view(torch.int32)


def ahf_stack_on_rt(amd, layers, dim, one_launch):
    flows = []
    for spec in layers:
        f = amd.AffineHalfFlow(dim, spec["parity"])
        f.load_state_dict(spec["params"])
        f.force_generic = 2
        flows.append(f)
    model = amd.NormalizingFlowModel(amd.StandardNormal(dim), flows).to(DEV)
    model.fuse_affine_runs = one_launch  # False: one ahf_rt launch per layer, as MNF_NO_RUN_FUSION=1
    return model


def stack_passes(amd, model, x, family):
    """inverse, forward from z, forward from x, log_prob: without gradients, every AffineHalfFlow launch of the family"""
    with torch.no_grad(), RG.recorded_families(amd) as seen:
        zs, ld_inv = model.inverse(x)
        assert amd.last_kernel() == family, amd.last_kernel()
        xs, ld_fwd = model.forward(zs[-1])
        assert amd.last_kernel() == family, amd.last_kernel()
        xs_x, ld_fwd_x = model.forward(x)
        blp = model.base_log_prob(x)
        lp, total = model.log_prob(x, return_sum=True)
        torch.cuda.synchronize()
    assert {k for k in seen.fresh if k.startswith("ahf")} <= {family}, seen.fresh
    return dict(zs=zs, ld_inv=ld_inv, xs=xs, ld_fwd=ld_fwd, xs_x=xs_x, ld_fwd_x=ld_fwd_x, blp=blp, lp=lp,
                mean=float(total.item()) / x.shape[0])


def same_bits_both_routes(a, b):
    """the one-launch route gives the layer-by-layer route's intermediates and log_det bit for bit"""
    for key in ("zs", "xs", "xs_x"):
        assert len(a[key]) == len(b[key])
        for i, (p, q) in enumerate(zip(a[key][1:], b[key][1:]), 1):
            assert torch.equal(bits(p), bits(q)), f"{key}[{i}]: {int((bits(p) != bits(q)).sum())} elements differ"
    for key in ("ld_inv", "ld_fwd", "ld_fwd_x", "blp"):
        assert torch.equal(bits(a[key]), bits(b[key])), f"{key}: {int((bits(a[key]) != bits(b[key])).sum())} elements differ"
    # (the epilogue forms log p from |z|^2 inside the launch and adds its fp64 sum with atomics: to rounding, as
    #  tests/test_hip_rt_stack.py::test_fused_log_prob holds it)
    assert_close(a["lp"], b["lp"], 1e-6, "log_prob, one launch vs layer by layer")


# ------------------------------------------------------------------------------------------------ G1, G3, G6, G9
@pytest.mark.parametrize("tag", ["init", "trained"])
def test_g1_c1_stack_rt(amd, golden, tag):
    """Fixture G1 (9 x AffineHalfFlow d = 2) with every layer on the run-time-shaped kernel, layer by layer ("ahf_rt")
    and as one launch ("ahf_stack_rt"): test_hip_parity.test_g1_c1_stack's comparisons and tolerance on every stored
    intermediate, and the two routes bit for bit."""
    fx = golden(f"g1_c1_stack_{tag}")
    x = t(fx["x"]).to(DEV)
    out = {}
    for family, one_launch in (("ahf_rt", False), ("ahf_stack_rt", True)):
        r = out[family] = stack_passes(amd, ahf_stack_on_rt(amd, g1_layers(fx), 2, one_launch), x, family)
        what = f"g1 {tag}"
        assert r["zs"][0] is x and len(r["zs"]) == 10
        close(r["ld_inv"], fx["ld_inv"], f"{what} ld_inv", family)
        for i in fx["keep"]:
            close(r["zs"][i], fx[f"zs{i}"], f"{what} zs{i}", family)
            close(r["xs"][i], fx[f"xs{i}"], f"{what} xs{i}", family)
        close(r["blp"], fx["base_log_prob"], f"{what} base_log_prob", family)
        close(r["ld_fwd"], fx["ld_fwd"], f"{what} ld_fwd", family)
        close(r["lp"], fx["ld_inv"] + fx["base_log_prob"], f"{what} log_prob", family)
        close_scalar(r["mean"], float(fx["mean_log_prob"]), f"{what} mean log_prob", family)
    same_bits_both_routes(out["ahf_rt"], out["ahf_stack_rt"])


@pytest.mark.parametrize("dim", [64, 256])
def test_g3_c2_stack_rt(amd, golden, dim):
    """Fixture G3 (the benchmark stack's weights, d = 64 and 256) the same two ways: test_hip_parity.test_g3_c2_stack's
    comparisons and tolerance, its float64 line included."""
    fx = golden("g3_c2_stack")
    x = t(fx[f"d{dim}.x"]).to(DEV)
    out = {}
    for family, one_launch in (("ahf_rt", False), ("ahf_stack_rt", True)):
        model = ahf_stack_on_rt(amd, c2_layers(dim), dim, one_launch)
        r = out[family] = stack_passes(amd, model, x, family)
        what = f"g3 d{dim}"
        close(r["zs"][-1], fx[f"d{dim}.z_last"], f"{what} z_last", family)
        close(r["zs"][4], fx[f"d{dim}.z_mid"], f"{what} z_mid", family)
        close(r["ld_inv"], fx[f"d{dim}.ld_inv"], f"{what} ld_inv", family)
        cur = x
        with torch.no_grad():
            for i, f in enumerate(reversed(model.flows)):
                cur, l1 = f.inverse(cur)
                assert amd.last_kernel() == "ahf_rt"
                close(l1, fx[f"d{dim}.ld_incr"][i], f"{what} ld_incr[{i}]", "ahf_rt")
        close(r["xs_x"][-1], fx[f"d{dim}.x_fwd_last"], f"{what} x_fwd_last", family)
        close(r["ld_fwd_x"], fx[f"d{dim}.ld_fwd"], f"{what} ld_fwd", family)
        close(r["blp"], fx[f"d{dim}.base_log_prob"], f"{what} base_log_prob", family)
        close(r["lp"], fx[f"d{dim}.ld_inv"] + fx[f"d{dim}.base_log_prob"], f"{what} log_prob", family)
        close_scalar(r["mean"], float(fx[f"d{dim}.mean_log_prob"]), f"{what} mean log_prob", family)
        close(r["zs"][-1], fx[f"d{dim}.z_last_f64"].astype(np.float32), f"{what} z_last vs fp64", family)
    same_bits_both_routes(out["ahf_rt"], out["ahf_stack_rt"])


def test_g6_c3_stack_rt(amd, golden):
    """Fixture G6 (3 x [ActNorm, Glow, NSF_CL], d = 32) with NSF_CL on "nsf_rt" and Glow on "linear_rows_rt":
    test_hip_parity.test_g6_c3_stack's assert_parity calls."""
    fx = golden("g6_c3_stack")
    x = t(fx["x"]).to(DEV)
    model = build_c3(amd, fx)
    for f in model.flows:
        f.force_generic = 2
    with torch.no_grad(), RG.recorded_families(amd) as seen:
        zs, ld = model.inverse(x)
        xs, ld_f = model.forward(x)
        torch.cuda.synchronize()
    want = {"nsf_rt", "linear_rows_rt"}
    assert want <= set(seen) and {k for k in seen.fresh if k.startswith(("nsf", "linear_rows", "glow"))} <= want, seen
    family = "nsf_rt+linear_rows_rt"
    close(zs[-1], fx["z_last"], "g6 z_last", family, fx["z_last64"])
    close(zs[5], fx["z_mid"], "g6 z_mid", family)
    close(ld, fx["ld_inv"], "g6 ld_inv", family, fx["ld_inv64"])
    close(xs[-1], fx["x_fwd_last"], "g6 x_fwd_last", family, fx["x_fwd_last64"])
    close(ld_f, fx["ld_fwd"], "g6 ld_fwd", family, fx["ld_fwd64"])


def test_g9_log_det_shapes_rt(amd, golden):
    """Fixture G9's log-det shapes with every layer that has a run-time-shaped kernel on it."""
    fx = golden("g9_logdet_shapes")
    x = recipes.gaussian(900, 8, 4).to(DEV)
    mods = {"affine_half": (amd.AffineHalfFlow(4, False), "ahf_rt"), "nsf_cl": (amd.NSF_CL(4, K=5), "nsf_rt"),
            "glow": (amd.Glow(4), "linear_rows_rt"), "rnvp": (amd.RNVP(4), "rnvp_rt")}
    with torch.no_grad():
        for name, (m, family) in mods.items():
            m.force_generic = 2
            m.to(DEV)
            assert tuple(m.forward(x)[1].shape) == tuple(fx[f"{name}.fwd"]), name
            assert amd.last_kernel() == family, (name, amd.last_kernel())
            if name != "rnvp":
                assert tuple(m.inverse(x)[1].shape) == tuple(fx[f"{name}.inv"]), name
                assert amd.last_kernel() == family, (name, amd.last_kernel())
        stack = amd.NormalizingFlow([amd.ActNormFlow(4).to(DEV), mods["glow"][0], mods["nsf_cl"][0]])
        zs, ld = stack.forward(x)
        assert amd.last_kernel() == "nsf_rt"
    assert tuple(ld.shape) == tuple(fx["stack.ld_shape"]) and zs[0] is x
    assert len(zs) == int(fx["stack.n_intermediates"])


# ------------------------------------------------------------------------------------------------ G17: gradients
LAYER_CASES = [(tag, force) for tag in RG.SINGLE_TAGS for force in ((2,) if C.kind_of(tag) == "glow" else (0, 1, 2))]
LAYER_IDS = [f"{tag}-{'tier_rt' if force == 2 else RG.TIER_NAME[force]}" for tag, force in LAYER_CASES]


@pytest.mark.parametrize("tag,force", LAYER_CASES, ids=LAYER_IDS)
def test_g17_layer_gradients(amd, golden, tag, force):
    """The reference's own autograd gradients of a single layer (x and every parameter) on default dispatch, the VALU
    kernels (force_generic = 1) and the run-time-shaped ones (2: the *_bwd_rt families by name; Glow: linear_rows_rt for
    grad_x, linear_rows_bwd_weight_rt for the weight gradient)."""
    RG.layer_case(amd, golden, tag, force)


@pytest.mark.parametrize("fused", [False, True], ids=["ahf_bwd_rt", "ahf_bwd_stack_rt"])
def test_g17_affine_run_gradients(amd, golden, fused):
    """The 4-layer AffineHalfFlow run under -mean log p: layer by layer, and as one autograd node (fuse_rt_training) with
    the cotangents of the last layer formed in the kernel."""
    loss = RG.run_case(amd, golden, fused)
    ref = float(golden(C.part_of(RG.RUN_TAG))[f"{RG.RUN_TAG}.loss"])
    close_scalar(loss, ref, f"{RG.RUN_TAG} loss", "ahf_stack_rt" if fused else "ahf_rt")


@pytest.mark.parametrize("pair", [False, True], ids=["layer_by_layer_rt", "glow_actnorm_inv_rt"])
def test_g17_spline_block_gradients(amd, golden, monkeypatch, pair):
    """One [ActNormFlow, Glow, NSF_CL] block under -mean log p with Glow and NSF_CL on the run-time-shaped kernels: layer
    by layer (linear_rows_rt, linear_rows_bwd_weight_rt, nsf_bwd_rt), and with the opt-in pair as one node
    (glow_actnorm_inv_rt, glow_actnorm_inv_bwd_rt, nsf_bwd_rt)."""
    from torch_mnf_amd import _dispatch

    monkeypatch.setattr(_dispatch, "GLOW_RT_MIN_ROWS", 0)  # (Glow's rt kernels at 333 rows without forcing the layer:
    monkeypatch.setattr(_dispatch, "GLOW_ACTNORM_RT", pair)  # glow.force_generic = 2 would take the pair either way)
    tag = RG.BLOCK_TAG
    model = RG.hip_module(amd, tag, 0)
    model.flows[2].force_generic = 2
    x = C.inputs(tag)["x"].to(DEV).requires_grad_(True)
    with RG.recorded_families(amd) as seen:
        loss = -model.log_prob(x).mean()
        loss.backward()
        torch.cuda.synchronize()
    want = ({"glow_actnorm_inv_rt", "glow_actnorm_inv_bwd_rt", "nsf_rt", "nsf_bwd_rt"} if pair else
            {"linear_rows_rt", "linear_rows_bwd_weight_rt", "nsf_rt", "nsf_bwd_rt"})
    ran = {k for k in seen.fresh if k.startswith(("nsf", "linear_rows", "glow", "xtg"))}
    assert want <= set(seen) and ran <= want, (seen, sorted(want))
    got = {"x": x.grad, **{k: q.grad for k, q in model.named_parameters()}}
    family = "glow_actnorm_inv_bwd_rt+nsf_bwd_rt" if pair else "linear_rows_bwd_weight_rt+nsf_bwd_rt"
    RG.check_grads(got, golden, tag, "rt", family)
    close_scalar(float(loss.detach()), float(golden(C.part_of(tag))[f"{tag}.loss"]), f"{tag} loss", family)
