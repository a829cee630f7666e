"""GPU tests of NSF_AR's one-pass direction on the matrix cores (``mnf_nsf_ar_rt`` behind ``NSF_AR.inverse``, kernel family
``nsf_ar_rt``): the reference's own ``NSF_AR.inverse`` runs (fixture G12), shapes on every path of the kernel against the
oracle, inputs on and outside the spline's interval, independence of the rows, the autoregressive structure, the round
trip through the VALU kernel's ``forward``, autograd through the new forward (the backward stays ``nsf_ar_bwd_generic``), a
two-layer model, and the routes.

Every case runs ``force_generic = 2`` and names the kernel it ran (``last_kernel()``).  Tolerances are the project's:
``helpers.assert_parity`` for values (1e-5 normwise plus twice the fp32 oracle's distance from the float64 oracle, that
widening capped at 5e-5), ``OracleGrads.check_all`` for gradients; both are recorded for tests/test_zz_audit.py."""
import functools

import pytest
import torch

import recipes
from helpers import assert_close, assert_parity
from test_hip_autograd import OracleGrads, cot_loss

pytestmark = pytest.mark.gpu
DEV = "cuda"
KERNEL = "nsf_ar_rt"
B = 3.0
G12_CASES = {"d2_k8": (2, 8, 16, 1.0), "d6_k5": (6, 5, 8, 1.0), "d16_k8": (16, 8, 8, 1.5)}  # dim, K, n_h, gain (fixture G12)

# (dim, K, n_h, rows): the reference's shape: one group, element 0 | . | odd width, unaligned rows, ragged last tile | top K,
# narrowest width, a last group of one element | two K-steps of input, dim % 4 = 1 | three K-steps, the widest class | . |
# a persistent grid smaller than the row blocks
SHAPES = [(2, 8, 16, 17), (3, 5, 8, 130), (6, 3, 5, 257), (13, 16, 4, 145), (37, 5, 8, 145), (70, 8, 16, 33), (33, 10, 12, 129),
          (6, 8, 8, 70003)]
MANY_BLOCKS = (6, 8, 8, 70003)


@pytest.fixture(scope="module")
def amd():
    import torch_mnf_amd

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    torch_mnf_amd._lib.load()
    return torch_mnf_amd


@pytest.fixture(scope="module")
def O():
    from oracle import flow_oracle

    return flow_oracle


def params(dim, K, n_h):
    return recipes.nsf_ar_params(3100 + dim + K, dim, K, n_h)


def make(amd, dim, K, n_h, sd=None, force=2):
    layer = amd.NSF_AR(dim, K=K, B=3, n_h=n_h)
    layer.load_state_dict(sd if sd is not None else params(dim, K, n_h))
    layer.force_generic = force
    return layer.to(DEV)


def layer_kernel():
    import torch_mnf_amd

    torch.cuda.synchronize()
    return torch_mnf_amd.last_kernel()


def run(layer, x, kernel=KERNEL):
    with torch.no_grad():
        z, ld = layer.inverse(x.to(DEV) if x.device.type == "cpu" else x)
    assert layer_kernel() == kernel
    return z, ld


def oracle_pair(O, x, sd, K):
    """fp32 and float64 (z, log_det) of NSF_AR.inverse as numpy arrays"""
    z32, ld32 = O.nsf_ar(x, sd, K, B, True)
    z64, ld64 = O.nsf_ar(x.double(), {k: v.double() for k, v in sd.items()}, K, B, True)
    return (z32.numpy(), ld32.numpy()), (z64.numpy(), ld64.numpy())


@functools.lru_cache(maxsize=None)
def oracle_values(dim, K, n_h, rows):
    """(x, fp32 (z, log_det), fp64 (z, log_det)) of a shape-matrix case: computed once, shared, never written"""
    from oracle import flow_oracle as O

    x = recipes.gaussian(3600 + dim, rows, dim, scale=1.4)
    return (x, *oracle_pair(O, x, params(dim, K, n_h), K))


# ---------------------------------------------------------------------------------------------------------------------
# 1. the reference's own runs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", sorted(G12_CASES))
def test_g12_reference_runs_on_the_rt_kernel(amd, O, golden, tag):
    """Fixture G12, the reference's own NSF_AR.inverse runs (spline_flow.py:218-235), through force_generic = 2; then the
    same with log_det accumulated onto a non-zero start, as NormalizingFlow's loop uses it."""
    fx = golden("g12_nsf_ar")
    dim, K, n_h, gain = G12_CASES[tag]
    sd = recipes.nsf_ar_params(1200 + dim + K, dim, K, n_h, gain=gain)
    layer = make(amd, dim, K, n_h, sd=sd)
    x = torch.from_numpy(fx[f"{tag}.x"]).to(DEV)
    z, ld = run(layer, x)
    widening = None if gain != 1.0 else 5e-5  # (d16_k8 is the stress fixture: tests/test_hip_round2.py)
    assert_parity(z, fx[f"{tag}.inv"], fx[f"{tag}.inv64"], f"nsf_ar_rt G12 {tag} z", max_widening=widening)
    # (the fixture carries the reference's fp32 log-det only: the float64 side comes from the oracle, as in test_hip_round2)
    _, ld64 = O.nsf_ar(x.cpu().double(), {k: v.double() for k, v in sd.items()}, K, B, True)
    assert_parity(ld, fx[f"{tag}.ld_inv"], ld64.numpy(), f"nsf_ar_rt G12 {tag} log_det", max_widening=widening)
    acc = torch.full((x.shape[0],), 0.25, device=DEV)
    with torch.no_grad():
        z2, none = layer._run(x, True, acc)
    assert layer_kernel() == KERNEL
    assert none is None and torch.equal(z2, z)
    assert torch.equal(acc, ld + 0.25)  # one fp32 add of the same sum


# ---------------------------------------------------------------------------------------------------------------------
# 2. shapes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,K,n_h,rows", SHAPES)
def test_shapes_vs_oracle(amd, dim, K, n_h, rows):
    x, (z32, ld32), (z64, ld64) = oracle_values(dim, K, n_h, rows)
    z, ld = run(make(amd, dim, K, n_h), x)
    what = f"nsf_ar_rt d={dim} K={K} n_h={n_h} rows={rows}"
    assert_parity(z, z32, z64, what=what)
    assert_parity(ld, ld32, ld64, what=what + " log_det")
    if (dim, K, n_h, rows) == MANY_BLOCKS:  # the persistent grid is smaller than the row blocks: workgroups loop
        from torch_mnf_amd import _lib

        grid = _lib.load().mnf_nsf_ar_rt_grid(rows, dim, K, 3, _lib.int_array((n_h,) * 3))
        assert 0 < grid and 2 * grid <= (rows + 127) // 128, grid  # (fewer workgroups than blocks of 8 waves x 2 tiles x 16 rows)


# ---------------------------------------------------------------------------------------------------------------------
# 3. inputs on the interval's ends and outside it
# ---------------------------------------------------------------------------------------------------------------------
def test_inputs_at_the_tail_bound_and_outside(amd, O):
    """Elements at exactly +-B and outside [-B, B] (identity, log-det contribution 0) in the first, a middle and the last
    position -- the conditioners of the later elements read them."""
    dim, K, n_h, rows = 6, 5, 8, 130
    sd = params(dim, K, n_h)
    x = recipes.gaussian(3600 + dim, rows, dim, scale=1.4).clone()
    for i, col in enumerate((0, 3, dim - 1)):
        x[4 * i + 0, col] = B
        x[4 * i + 1, col] = -B
        x[4 * i + 2, col] = 7.5
        x[4 * i + 3, col] = -4.25
    x[12] = torch.tensor([3.5, -3.0, 3.0, -6.0, 0.1, 9.0])  # several in one row
    x[129, dim - 1] = 5.0  # in the ragged last tile
    (z32, ld32), (z64, ld64) = oracle_pair(O, x, sd, K)
    z, ld = run(make(amd, dim, K, n_h), x)
    assert_parity(z, z32, z64, what="nsf_ar_rt edge inputs")
    assert_parity(ld, ld32, ld64, what="nsf_ar_rt edge inputs log_det")
    outside = (x.abs() > B).to(DEV)
    assert torch.equal(z[outside], x.to(DEV)[outside])  # the identity, bit for bit
    row = torch.tensor([3.5, -3.25, 4.0, -6.0, 3.125, 9.0]).repeat(3, 1)  # every element outside: log-det exactly 0
    z_out, ld_out = run(make(amd, dim, K, n_h), row)
    assert torch.equal(z_out.cpu(), row) and float(ld_out.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# 4. rows do not see each other
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,K,n_h,rows", [(6, 3, 5, 257), (37, 5, 8, 145)])
def test_rows_do_not_see_each_other(amd, dim, K, n_h, rows):
    """A row alone in a one-row batch, at the end of a ragged tile (a 130-row prefix) and in the full batch: the same bits."""
    x = oracle_values(dim, K, n_h, rows)[0].to(DEV)
    layer = make(amd, dim, K, n_h)
    z, ld = run(layer, x)
    z_head, ld_head = run(layer, x[:130].contiguous())
    assert torch.equal(z_head, z[:130]) and torch.equal(ld_head, ld[:130])
    for r in (0, 129, rows - 1):
        z_one, ld_one = run(layer, x[r:r + 1].contiguous())
        assert torch.equal(z_one, z[r:r + 1]) and torch.equal(ld_one, ld[r:r + 1]), r


# ---------------------------------------------------------------------------------------------------------------------
# 5. the autoregressive structure
# ---------------------------------------------------------------------------------------------------------------------
def test_an_element_depends_on_the_elements_before_it_only(amd):
    """Changing x[:, i] leaves z[:, :i] bit for bit unchanged (and changes z[:, i:])."""
    dim, K, n_h, rows = 13, 16, 4, 145
    x = oracle_values(dim, K, n_h, rows)[0].to(DEV)
    layer = make(amd, dim, K, n_h)
    z, _ = run(layer, x)
    for i in (0, 1, 3, 4, 7, 12):
        x2 = x.clone()
        x2[:, i] = (0.5 * x2[:, i] + 0.3).clamp(-2.5, 2.5)
        z2, _ = run(layer, x2)
        assert torch.equal(z2[:, :i], z[:, :i]), i
        assert not torch.equal(z2[:, i], z[:, i]), i
        if i + 1 < dim:
            assert not torch.equal(z2[:, i + 1:], z[:, i + 1:]), i


@pytest.mark.parametrize("small,large", [(5, 7), (4, 9), (2, 3)])
def test_a_narrower_layer_from_the_same_parameter_prefix(amd, small, large):
    """The layout has no weight a net never reads; what stands in for a masked-out weight is a net beyond the layer's dim.  A
    dim-`small` layer built from the prefix of a dim-`large` layer's parameters gives the first `small` columns of the
    larger layer's result bit for bit -- the nets 4 g + q' >= dim of the last group are staged as zeros and touch nothing."""
    K, n_h, rows = 5, 8, 97
    sd = params(large, K, n_h)
    sd_small = {k: v for k, v in sd.items() if k == "init_param" or int(k.split(".")[1]) < small - 1}
    x = recipes.gaussian(3600 + large, rows, large, scale=1.4)
    z_large, _ = run(make(amd, large, K, n_h, sd=sd), x)
    z_small, ld_small = run(make(amd, small, K, n_h, sd=sd_small), x[:, :small].contiguous())
    assert torch.equal(z_small, z_large[:, :small])
    assert bool(torch.isfinite(ld_small).all())


# ---------------------------------------------------------------------------------------------------------------------
# 6. round trip
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,K,n_h,rows", [(6, 3, 5, 257), (33, 10, 12, 129)])
def test_round_trip_through_the_valu_forward(amd, dim, K, n_h, rows):
    """NSF_AR.forward (the sequential direction, VALU kernel) after the new inverse returns x, and the log-dets cancel --
    what test_g12_nsf_ar_vs_reference demands of the VALU pair."""
    x = oracle_values(dim, K, n_h, rows)[0].to(DEV)
    layer = make(amd, dim, K, n_h)
    z, ld = run(layer, x)
    with torch.no_grad():
        back, ld_b = layer.forward(z)
    assert layer_kernel() == "nsf_ar_generic"
    assert float((back - x).abs().max()) <= 2e-4 * float(x.abs().max())
    assert float((ld + ld_b).abs().max()) <= 2e-4 * max(float(ld.abs().max()), 1.0)


# ---------------------------------------------------------------------------------------------------------------------
# 7. autograd through the new forward
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,K,n_h", [(5, 5, 8), (9, 8, 6)])
def test_autograd_through_the_new_forward(amd, O, dim, K, n_h):
    """forward on nsf_ar_rt, backward on nsf_ar_bwd_generic (it recomputes from x); gradients against autograd through the
    oracle, as test_nsf_ar_gradients_vs_autograd_through_the_oracle."""
    sd = recipes.nsf_ar_params(70 + dim, dim, K, n_h)
    rows = 97
    x = recipes.gaussian(71 + dim, rows, dim, scale=1.2)
    w, v = recipes.gaussian(72, rows, dim), recipes.gaussian(73, rows, 1)[:, 0]
    og = OracleGrads(cot_loss(lambda xx, p: O.nsf_ar(xx, p, K, B, True), w, v), x, sd)
    layer = make(amd, dim, K, n_h, sd=sd)
    xg = x.clone().to(DEV).requires_grad_(True)
    z, ld = layer.inverse(xg)
    assert layer_kernel() == KERNEL
    ((w.to(DEV) * z).sum() + (v.to(DEV) * ld).sum()).backward()
    assert layer_kernel() == "nsf_ar_bwd_generic"
    got = {"x": xg.grad, **{name: prm.grad for name, prm in layer.named_parameters()}}
    og.check_all(got, f"nsf_ar_rt forward + nsf_ar_bwd_generic d={dim} K={K}")


# ---------------------------------------------------------------------------------------------------------------------
# 8. a model
# ---------------------------------------------------------------------------------------------------------------------
def test_two_layer_model_inverse(amd, O):
    """NormalizingFlow([NSF_AR, NSF_AR]).inverse (log_det += in the kernel) against the oracle's stack at the existing stack
    test's budget (two splines deep: the reference's own fp32 noise)."""
    dim, K, n_h, rows = 12, 8, 4, 333
    sds = [recipes.nsf_ar_params(3300 + i, dim, K, n_h) for i in range(2)]
    flow = amd.NormalizingFlow([make(amd, dim, K, n_h, sd=sd) for sd in sds])
    x = recipes.gaussian(3301, rows, dim, scale=1.4)
    with torch.no_grad():
        zs, ld = flow.inverse(x.to(DEV))
    assert layer_kernel() == KERNEL
    ref_zs, ref_ld = O.flow_stack(x, [{"kind": "nsf_ar", "K": K, "B": B, "params": sd} for sd in sds], True)
    assert len(zs) == 3
    assert_close(zs[-1], ref_zs[-1], 1e-4, "2 x nsf_ar_rt stack z")
    assert_close(ld, ref_ld, 1e-4, "2 x nsf_ar_rt stack log_det")


# ---------------------------------------------------------------------------------------------------------------------
# 9. routes
# ---------------------------------------------------------------------------------------------------------------------
def test_the_shipped_route_is_opt_in_and_switches_at_the_threshold(amd, monkeypatch):
    """With the shipped None, 4,099 rows run the VALU kernel; with NSF_AR_RT_MIN_ROWS = 2048 they run nsf_ar_rt and 2,047
    rows do not; the sequential direction never does."""
    from torch_mnf_amd import _dispatch

    assert _dispatch.NSF_AR_RT_MIN_ROWS is None
    dim, K, n_h = 6, 8, 8
    layer = make(amd, dim, K, n_h, force=0)
    x = recipes.gaussian(3600 + dim, 4099, dim, scale=1.4).to(DEV)
    run(layer, x, kernel="nsf_ar_generic")
    monkeypatch.setattr(_dispatch, "NSF_AR_RT_MIN_ROWS", 2048)
    run(layer, x)
    run(layer, x[:2047].contiguous(), kernel="nsf_ar_generic")
    run(layer, x[:2048].contiguous())
    with torch.no_grad():
        layer.forward(x)
    assert layer_kernel() == "nsf_ar_generic"
    layer.force_generic = 1
    run(layer, x, kernel="nsf_ar_generic")


@pytest.mark.parametrize("dim,K,n_h", [(6, 5, 20), (1, 5, 8)])
def test_fallback_for_a_shape_without_a_plan(amd, O, dim, K, n_h):
    """Nets wider than 16 units and dim = 1 (no net at all) fall back to the VALU kernel under force_generic = 2."""
    rows = 100
    sd = params(dim, K, n_h)
    x = recipes.gaussian(3600 + dim, rows, dim, scale=1.4)
    z, ld = run(make(amd, dim, K, n_h), x, kernel="nsf_ar_generic")
    (z32, ld32), (z64, ld64) = oracle_pair(O, x, sd, K)
    assert_parity(z, z32, z64, what=f"nsf_ar_generic fallback of nsf_ar_rt d={dim} n_h={n_h}")
    assert_parity(ld, ld32, ld64, what=f"nsf_ar_generic fallback of nsf_ar_rt d={dim} n_h={n_h} log_det")
