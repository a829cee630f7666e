"""GPU tests of NSF_AR's element-by-element direction on the matrix cores (``mnf_nsf_ar_seq_rt`` behind ``NSF_AR.forward``,
kernel family ``nsf_ar_seq_rt``): the reference's own ``NSF_AR.forward`` runs (fixture G12), shapes on every path of the
kernel against the oracle, the autoregressive structure, independence of the rows, the parameter prefix, inputs on and
outside the spline's interval, a NaN in the input, the round trip through both ``inverse`` kernels, autograd through the new
forward (the backward stays ``nsf_ar_bwd_generic``), a two-layer model and ``sample``, and the routes.

The route is opt-in as shipped: every case sets ``_dispatch.NSF_AR_SEQ_RT_MIN_ROWS`` (monkeypatch) and names the kernel
it ran (``last_kernel()``).  Tolerances are the project's: ``helpers.assert_parity`` for values (1e-5 normwise plus twice
the fp32 oracle's distance from the float64 oracle, that widening capped at 5e-5), ``OracleGrads.check_all`` for
gradients; both are recorded for tests/test_zz_audit.py."""
import functools

import pytest
import torch

import recipes
from helpers import assert_close, assert_parity
from test_hip_autograd import OracleGrads, cot_loss

pytestmark = pytest.mark.gpu
DEV = "cuda"
KERNEL, VALU = "nsf_ar_seq_rt", "nsf_ar_generic"
B = 3.0
NOT_SHIPPED_K, MAX_DIM = 10, 128  # csrc/mnf_nsf_ar_seq_rt.hip: ar_seq_has_k, kArSeqMaxDim
G12_CASES = {"d2_k8": (2, 8, 16, 1.0), "d6_k5": (6, 5, 8, 1.0), "d16_k8": (16, 8, 8, 1.5)}  # dim, K, n_h, gain (fixture G12)

# (dim, K, n_h, rows): the reference's shape: element 0 and one net | . | odd width, rows not a multiple of 64, ragged last
# tile | the narrowest width, dim % 4 = 1 | two K-steps of input | . | the widest net | many row blocks | a persistent grid
# smaller than the row blocks whatever the tiles per wave (a workgroup of 8 waves takes 256 rows: 1,172 blocks)
SHAPES = [(2, 8, 16, 17), (3, 5, 8, 130), (6, 5, 5, 257), (13, 8, 4, 145), (37, 5, 8, 145), (33, 8, 12, 129), (64, 8, 16, 33),
          (6, 8, 8, 70003), (6, 5, 8, 300007)]
MANY_BLOCKS = (6, 5, 8, 300007)


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


@pytest.fixture(autouse=True)
def opted_in(monkeypatch):
    """The route opted in from the first row on; a layer's force_generic = 2 lifts wants_rt's 2,048-row floor as well."""
    from torch_mnf_amd import _dispatch

    assert _dispatch.NSF_AR_SEQ_RT_MIN_ROWS is None  # as shipped
    monkeypatch.setattr(_dispatch, "NSF_AR_SEQ_RT_MIN_ROWS", 1)


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


def run(layer, z, kernel=KERNEL):
    with torch.no_grad():
        x, ld = layer.forward(z.to(DEV) if z.device.type == "cpu" else z)
    assert layer_kernel() == kernel
    return x, ld


def oracle_pair(O, z, sd, K):
    """fp32 and float64 (x, log_det) of NSF_AR.forward as numpy arrays"""
    x32, ld32 = O.nsf_ar(z, sd, K, B, False)
    x64, ld64 = O.nsf_ar(z.double(), {k: v.double() for k, v in sd.items()}, K, B, False)
    return (x32.numpy(), ld32.numpy()), (x64.numpy(), ld64.numpy())


@functools.lru_cache(maxsize=None)
def oracle_values(dim, K, n_h, rows):
    """(z, fp32 (x, log_det), fp64 (x, log_det)) of a shape-matrix case: computed once, shared, never written"""
    from oracle import flow_oracle as O

    z = recipes.gaussian(3700 + dim, rows, dim, scale=1.4)
    return (z, *oracle_pair(O, z, params(dim, K, n_h), K))


# ---------------------------------------------------------------------------------------------------------------------
# 1. the reference's own runs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", sorted(G12_CASES))
def test_g12_reference_runs_on_the_seq_rt_kernel(amd, O, golden, tag):
    """Fixture G12, the reference's own NSF_AR.forward runs (spline_flow.py:199-216); then the same with log_det accumulated
    onto a non-zero start, as NormalizingFlow's loop uses it."""
    fx = golden("g12_nsf_ar")
    dim, K, n_h, gain = G12_CASES[tag]
    sd = recipes.nsf_ar_params(1200 + dim + K, dim, K, n_h, gain=gain)
    layer = make(amd, dim, K, n_h, sd=sd)
    z = torch.from_numpy(fx[f"{tag}.x"]).to(DEV)
    x, ld = run(layer, z)
    widening = None if gain != 1.0 else 5e-5  # (d16_k8 is the stress fixture: tests/test_hip_round2.py)
    assert_parity(x, fx[f"{tag}.fwd"], fx[f"{tag}.fwd64"], f"nsf_ar_seq_rt G12 {tag} x", max_widening=widening)
    # (the fixture carries the reference's fp32 log-det only: the float64 side comes from the oracle, as in test_hip_round2)
    _, ld64 = O.nsf_ar(z.cpu().double(), {k: v.double() for k, v in sd.items()}, K, B, False)
    assert_parity(ld, fx[f"{tag}.ld_fwd"], ld64.numpy(), f"nsf_ar_seq_rt G12 {tag} log_det", max_widening=widening)
    acc = torch.full((z.shape[0],), 0.25, device=DEV)
    with torch.no_grad():
        x2, none = layer._run(z, False, acc)
    assert layer_kernel() == KERNEL
    assert none is None and torch.equal(x2, x)
    assert torch.equal(acc, ld + 0.25)  # one fp32 add of the same sum


# ---------------------------------------------------------------------------------------------------------------------
# 2. shapes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,K,n_h,rows", SHAPES)
def test_shapes_vs_oracle(amd, dim, K, n_h, rows):
    z, (x32, ld32), (x64, ld64) = oracle_values(dim, K, n_h, rows)
    if rows * dim >= 1000:
        assert 0.005 < float((z.abs() > B).float().mean()) < 0.08  # some elements on the identity tails
    x, ld = run(make(amd, dim, K, n_h), z)
    what = f"nsf_ar_seq_rt d={dim} K={K} n_h={n_h} rows={rows}"
    assert_parity(x, x32, x64, what=what)
    assert_parity(ld, ld32, ld64, what=what + " log_det")
    if (dim, K, n_h, rows) == MANY_BLOCKS:  # the persistent grid is smaller than the row blocks: workgroups loop
        from torch_mnf_amd import _lib

        grid = _lib.load().mnf_nsf_ar_seq_rt_grid(rows, dim, K, 3, _lib.int_array((n_h,) * 3))
        assert 0 < grid < (rows + 511) // 512, grid  # (fewer workgroups than blocks of 512 rows, and so than those of 8 waves x 32)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the autoregressive structure
# ---------------------------------------------------------------------------------------------------------------------
def test_an_element_depends_on_the_elements_before_it_only(amd):
    """Changing z[:, i] leaves x[:, :i] bit for bit unchanged and changes x[:, i] (and what follows it)."""
    dim, K, n_h, rows = 13, 8, 4, 145
    z = oracle_values(dim, K, n_h, rows)[0].to(DEV)
    layer = make(amd, dim, K, n_h)
    x, _ = run(layer, z)
    for i in (0, 1, 3, 4, 7, 12):
        z2 = z.clone()
        z2[:, i] = (0.5 * z2[:, i] + 0.3).clamp(-2.5, 2.5)
        x2, _ = run(layer, z2)
        assert torch.equal(x2[:, :i], x[:, :i]), i
        assert not torch.equal(x2[:, i], x[:, i]), i
        if i + 1 < dim:
            assert not torch.equal(x2[:, i + 1:], x[:, i + 1:]), i


# ---------------------------------------------------------------------------------------------------------------------
# 4. rows do not see each other
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,K,n_h,rows", [(6, 5, 5, 257), (37, 5, 8, 145)])
def test_rows_do_not_see_each_other(amd, dim, K, n_h, rows):
    """A row alone in a one-row batch, at the end of a ragged tile (a 130-row prefix) and in the full batch: the same bits."""
    z = oracle_values(dim, K, n_h, rows)[0].to(DEV)
    layer = make(amd, dim, K, n_h)
    x, ld = run(layer, z)
    x_head, ld_head = run(layer, z[:130].contiguous())
    assert torch.equal(x_head, x[:130]) and torch.equal(ld_head, ld[:130])
    for r in (0, 129, rows - 1):
        x_one, ld_one = run(layer, z[r:r + 1].contiguous())
        assert torch.equal(x_one, x[r:r + 1]) and torch.equal(ld_one, ld[r:r + 1]), r


# ---------------------------------------------------------------------------------------------------------------------
# 5. a narrower layer from the same parameter prefix
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("small,large", [(5, 7), (4, 9), (2, 3)])
def test_a_narrower_layer_from_the_same_parameter_prefix(amd, small, large):
    """A dim-`small` layer built from the prefix of a dim-`large` layer's parameters gives the first `small` columns of the
    larger layer's result bit for bit: net e reads nothing but its own parameters and the columns before it."""
    K, n_h, rows = 5, 8, 97
    sd = params(large, K, n_h)
    sd_small = {k: v for k, v in sd.items() if k == "init_param" or int(k.split(".")[1]) < small - 1}
    z = recipes.gaussian(3700 + large, rows, large, scale=1.4)
    x_large, _ = run(make(amd, large, K, n_h, sd=sd), z)
    x_small, ld_small = run(make(amd, small, K, n_h, sd=sd_small), z[:, :small].contiguous())
    assert torch.equal(x_small, x_large[:, :small])
    assert bool(torch.isfinite(ld_small).all())


# ---------------------------------------------------------------------------------------------------------------------
# 6. inputs on the interval's ends and outside it
# ---------------------------------------------------------------------------------------------------------------------
def test_inputs_at_the_tail_bound_and_outside(amd, O):
    """Elements at exactly +-B and outside [-B, B] (identity, log-det contribution 0) in the first, a middle and the last
    position -- the conditioners of the later elements read them."""
    dim, K, n_h, rows = 6, 5, 8, 130
    sd = params(dim, K, n_h)
    z = recipes.gaussian(3700 + dim, rows, dim, scale=1.4).clone()
    for i, col in enumerate((0, 3, dim - 1)):
        z[4 * i + 0, col] = B
        z[4 * i + 1, col] = -B
        z[4 * i + 2, col] = 7.5
        z[4 * i + 3, col] = -4.25
    z[12] = torch.tensor([3.5, -3.0, 3.0, -6.0, 0.1, 9.0])  # several in one row
    z[129, dim - 1] = 5.0  # in the ragged last tile
    (x32, ld32), (x64, ld64) = oracle_pair(O, z, sd, K)
    x, ld = run(make(amd, dim, K, n_h), z)
    assert_parity(x, x32, x64, what="nsf_ar_seq_rt edge inputs")
    assert_parity(ld, ld32, ld64, what="nsf_ar_seq_rt edge inputs log_det")
    outside = (z.abs() > B).to(DEV)
    assert torch.equal(x[outside], z.to(DEV)[outside])  # the identity, bit for bit
    row = torch.tensor([3.5, -3.25, 4.0, -6.0, 3.125, 9.0]).repeat(3, 1)  # every element outside: log-det exactly 0
    x_out, ld_out = run(make(amd, dim, K, n_h), row)
    assert torch.equal(x_out.cpu(), row) and float(ld_out.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# 7. a NaN in the input
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,K,n_h,rows", [(13, 8, 4, 145), (37, 5, 8, 145)])
def test_a_nan_stays_in_its_row_and_behind_its_column(amd, dim, K, n_h, rows):
    """A NaN in z[r, i]: x[r, :i] as in the clean run (decoded before), x[r, i:] NaN (the spline hands it through and every
    later net reads it; only a later element outside the tail bound stays the identity), every other row -- those of its 16-row tile and of its wave included -- bit for bit the clean run."""
    z = oracle_values(dim, K, n_h, rows)[0].to(DEV)
    layer = make(amd, dim, K, n_h)
    x, ld = run(layer, z)
    hits = {3: 0, 20: 5, 70: dim - 1, 144: 2}  # row -> column: first tile, second tile of a wave, a later wave, ragged tile
    z2 = z.clone()
    for r, i in hits.items():
        z2[r, i] = float("nan")
    x2, ld2 = run(layer, z2)
    clean = torch.ones(rows, dtype=torch.bool, device=DEV)
    for r, i in hits.items():
        clean[r] = False
        assert torch.equal(x2[r, :i], x[r, :i]), (r, i)
        tail = z2[r, i:].abs() > B  # (an element outside [-B, B] is the identity whatever its parameters, as in the reference)
        assert bool(torch.isnan(x2[r, i:][~tail]).all()) and torch.equal(x2[r, i:][tail], z2[r, i:][tail]), (r, i)
        assert int((~tail).sum()) >= (dim - i + 1) // 2, (r, i)
    assert torch.equal(x2[clean], x[clean]) and torch.equal(ld2[clean], ld[clean])


# ---------------------------------------------------------------------------------------------------------------------
# 8. round trip
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inverse_kernel,force", [("nsf_ar_generic", 1), ("nsf_ar_rt", 2)])
@pytest.mark.parametrize("dim,K,n_h,rows", [(6, 5, 5, 257), (33, 8, 12, 129)])
def test_round_trip_through_both_inverse_kernels(amd, dim, K, n_h, rows, inverse_kernel, force):
    """NSF_AR.inverse (the one-pass direction: VALU kernel, then nsf_ar_rt) after the new forward returns z, and the log-dets
    cancel -- the budget of test_round_trip_through_the_valu_forward."""
    z = oracle_values(dim, K, n_h, rows)[0].to(DEV)
    x, ld = run(make(amd, dim, K, n_h), z)
    with torch.no_grad():
        back, ld_b = make(amd, dim, K, n_h, force=force).inverse(x)
    assert layer_kernel() == inverse_kernel
    assert float((back - z).abs().max()) <= 2e-4 * float(z.abs().max())
    assert float((ld + ld_b).abs().max()) <= 2e-4 * max(float(ld.abs().max()), 1.0)


# ---------------------------------------------------------------------------------------------------------------------
# 9. autograd through the new forward
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,K,n_h", [(5, 5, 8), (9, 8, 6)])
def test_autograd_through_the_new_forward(amd, O, dim, K, n_h):
    """forward on nsf_ar_seq_rt, backward on nsf_ar_bwd_generic (it recomputes from z); gradients against autograd through
    the oracle, as test_nsf_ar_gradients_vs_autograd_through_the_oracle."""
    sd = recipes.nsf_ar_params(70 + dim, dim, K, n_h)
    rows = 97
    z = recipes.gaussian(71 + dim, rows, dim, scale=1.2)
    w, v = recipes.gaussian(72, rows, dim), recipes.gaussian(73, rows, 1)[:, 0]
    og = OracleGrads(cot_loss(lambda zz, p: O.nsf_ar(zz, p, K, B, False), w, v), z, sd)
    layer = make(amd, dim, K, n_h, sd=sd)
    zg = z.clone().to(DEV).requires_grad_(True)
    x, ld = layer.forward(zg)
    assert layer_kernel() == KERNEL
    ((w.to(DEV) * x).sum() + (v.to(DEV) * ld).sum()).backward()
    assert layer_kernel() == "nsf_ar_bwd_generic"
    got = {"x": zg.grad, **{name: prm.grad for name, prm in layer.named_parameters()}}
    og.check_all(got, f"nsf_ar_seq_rt forward + nsf_ar_bwd_generic d={dim} K={K}")


# ---------------------------------------------------------------------------------------------------------------------
# 10. a model
# ---------------------------------------------------------------------------------------------------------------------
def test_two_layer_model_forward_and_sample(amd, O):
    """NormalizingFlow([NSF_AR, NSF_AR]).forward (log_det += in the kernel) against the oracle's stack at the existing stack
    test's budget (two splines deep: the reference's own fp32 noise); NormalizingFlowModel.sample runs the same kernel."""
    dim, K, n_h, rows = 12, 8, 4, 333
    sds = [recipes.nsf_ar_params(3300 + i, dim, K, n_h) for i in range(2)]
    flow = amd.NormalizingFlowModel(amd.StandardNormal(dim, DEV), [make(amd, dim, K, n_h, sd=sd) for sd in sds])
    z = recipes.gaussian(3301, rows, dim, scale=1.4)
    with torch.no_grad():
        xs, ld = flow.forward(z.to(DEV))
    assert layer_kernel() == KERNEL
    ref_xs, ref_ld = O.flow_stack(z, [{"kind": "nsf_ar", "K": K, "B": B, "params": sd} for sd in sds], False)
    assert len(xs) == 3
    assert_close(xs[-1], ref_xs[-1], 1e-4, "2 x nsf_ar_seq_rt stack x")
    assert_close(ld, ref_ld, 1e-4, "2 x nsf_ar_seq_rt stack log_det")
    flow.flows[0].force_generic = 1
    run(flow.flows[0], z, kernel=VALU)  # another family's name in last_kernel() ...
    flow.flows[0].force_generic = 2
    with torch.no_grad():
        samples = flow.sample(300)
    assert layer_kernel() == KERNEL  # ... which sample() replaces
    assert samples.shape == (300, dim) and bool(torch.isfinite(samples).all())
    assert amd._dispatch.tier_of_kernel(KERNEL) == "rt"


# ---------------------------------------------------------------------------------------------------------------------
# 11. routes
# ---------------------------------------------------------------------------------------------------------------------
def test_the_shipped_route_is_opt_in_and_switches_at_the_threshold(amd, monkeypatch):
    """With the shipped None, 4,099 rows and force_generic = 2 both run the VALU kernel; with NSF_AR_SEQ_RT_MIN_ROWS = 2048
    4,099 and 2,048 rows run nsf_ar_seq_rt and 2,047 rows do not; force_generic = 1 and an fp32 request veto; the one-pass
    direction never takes it."""
    from torch_mnf_amd import _dispatch

    monkeypatch.setattr(_dispatch, "NSF_AR_SEQ_RT_MIN_ROWS", None)  # as shipped
    dim, K, n_h = 6, 8, 8
    layer = make(amd, dim, K, n_h, force=0)
    z = recipes.gaussian(3700 + dim, 4099, dim, scale=1.4).to(DEV)
    run(layer, z, kernel=VALU)
    layer.force_generic = 2
    run(layer, z, kernel=VALU)
    layer.force_generic = 0
    monkeypatch.setattr(_dispatch, "NSF_AR_SEQ_RT_MIN_ROWS", 2048)
    x, ld = run(layer, z)
    run(layer, z[:2047].contiguous(), kernel=VALU)
    x_head, ld_head = run(layer, z[:2048].contiguous())
    assert torch.equal(x_head, x[:2048]) and torch.equal(ld_head, ld[:2048])
    with torch.no_grad():
        layer.inverse(z)
    assert layer_kernel() == "nsf_ar_generic"  # NSF_AR.inverse is unaffected ...
    layer.force_generic = 2
    with torch.no_grad():
        layer.inverse(z)
    assert layer_kernel() == "nsf_ar_rt"       # ... under either setting
    layer.force_generic = 1
    run(layer, z, kernel=VALU)
    layer.force_generic = 0
    layer.force_fp32_mfma = True
    run(layer, z, kernel=VALU)
    layer.force_generic = 2
    run(layer, z, kernel=VALU)
    layer.force_fp32_mfma = False
    run(layer, z)


@pytest.mark.parametrize("dim,K,n_h", [(6, 5, 20), (1, 5, 8), (6, NOT_SHIPPED_K, 8), (MAX_DIM + 1, 5, 4)])
def test_fallback_for_a_shape_without_a_plan(amd, O, dim, K, n_h):
    """Nets wider than 16 units, dim = 1 (no net at all), a K that did not ship and a dim above the slab's bound fall back
    to the VALU kernel with the route opted in and force_generic = 2."""
    rows = 100
    sd = params(dim, K, n_h)
    z = recipes.gaussian(3700 + dim, rows, dim, scale=1.4)
    x, ld = run(make(amd, dim, K, n_h), z, kernel=VALU)
    (x32, ld32), (x64, ld64) = oracle_pair(O, z, sd, K)
    assert_parity(x, x32, x64, what=f"nsf_ar_generic fallback of nsf_ar_seq_rt d={dim} K={K} n_h={n_h}")
    assert_parity(ld, ld32, ld64, what=f"nsf_ar_generic fallback of nsf_ar_seq_rt d={dim} K={K} n_h={n_h} log_det")
