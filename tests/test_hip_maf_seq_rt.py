"""GPU tests of the element-by-element direction of MAF / IAF on the matrix cores (``mnf_maf_seq_rt`` behind ``MAF.forward``
/ ``IAF.inverse``, kernel family ``maf_seq_rt``): the reference's own ``MAF.forward`` runs (fixture G15), shapes on every
path of the kernel against the oracle, independence of the rows, unaligned rows, masked-out weights, a permuted MADE,
autograd through the new forward (the backward stays ``maf_bwd_generic``), a 3-layer model, the fallback and the default
route's threshold.

Every case names the kernel it ran (``last_kernel()``).  Tolerances are the project's: ``helpers.assert_parity`` for values
(1e-5 normwise plus twice the fp32 oracle's distance from the float64 oracle, that widening capped at 5e-5),
``OracleGrads.check`` for gradients; both are recorded for tests/test_zz_audit.py."""
import functools

import numpy as np
import pytest
import torch

import recipes
from helpers import RTOL, assert_parity, normwise_err
from test_hip_autograd import OracleGrads, cot_loss
from test_oracle_golden import G15_CASES, g15_params

pytestmark = pytest.mark.gpu
DEV = "cuda"
KERNEL = "maf_seq_rt"

# (dim, h_sizes, rows): the reference's shape | odd dim, unaligned rows, two row blocks with a ragged last tile | odd widths |
# one wide layer | several output tiles, two K-steps of input | four layers, dim > 64 | the widest class near the LDS limit
# (four waves per workgroup) | dim > 128: nine output tiles, two waves per workgroup | a persistent grid smaller than the
# row blocks
SEQ_SHAPES = [(2, (24, 24, 24), 17), (3, (5,), 130), (37, (20, 7, 33), 257), (40, (64,), 129), (64, (24, 24, 24), 145),
              (100, (16,) * 4, 33), (33, (128, 128), 145), (130, (64, 64), 33), (6, (8,), 70003)]
MANY_BLOCKS = (6, (8,), 70003)


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


def params(dim, h_sizes):
    return recipes.maf_params(2100 + dim + len(h_sizes), dim, h_sizes, gain=1.2, last_gain=0.5)


def make(amd, dim, h_sizes, parity, cls=None, force=2, sd=None):
    layer = (cls or amd.MAF)(dim, parity=parity, h_sizes=h_sizes)
    missing = layer.load_state_dict(sd if sd is not None else params(dim, h_sizes), strict=False)
    assert all(k.endswith(".mask") for k in missing.missing_keys) and not missing.unexpected_keys
    layer.force_generic = force
    return layer.to(DEV)


def sequential(layer, x):
    """the element-by-element direction of either class: MAF.forward, IAF.inverse"""
    return layer.inverse(x) if type(layer).__name__ == "IAF" else layer.forward(x)


def layer_kernel():
    import torch_mnf_amd

    torch.cuda.synchronize()
    return torch_mnf_amd.last_kernel()


@functools.lru_cache(maxsize=None)
def oracle_values(dim, h_sizes, rows, parity):
    """(z, fp32 (y, log_det), fp64 (y, log_det)) of the element-by-element direction: computed once, shared, never written"""
    from oracle import flow_oracle as O

    sd, masks = params(dim, h_sizes), O.made_masks(dim, h_sizes, 2 * dim)
    z = recipes.gaussian(2600 + dim, rows, dim)
    y32, ld32 = O.maf(z, sd, masks, parity, False)
    y64, ld64 = O.maf(z.double(), {k: v.double() for k, v in sd.items()}, masks, parity, False)
    return z, (y32.numpy(), ld32.numpy()), (y64.numpy(), ld64.numpy())


def run(layer, z):
    with torch.no_grad():
        y, ld = sequential(layer, z.to(DEV) if z.device.type == "cpu" else z)
    assert layer_kernel() == KERNEL
    return y, ld


# ---------------------------------------------------------------------------------------------------------------------
# 1. the reference's own runs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parity", [False, True])
@pytest.mark.parametrize("tag", sorted(G15_CASES))
def test_g15_reference_runs_on_the_seq_rt_kernel(amd, O, golden, tag, parity):
    """Fixture G15, the reference's own MAF.forward runs (flows/maf.py:39-51), through force_generic = 2; IAF.inverse is
    the same launch: bit for bit.  log_det accumulation as NormalizingFlow's loop uses it."""
    fx = golden("g15_maf_iaf")
    dim, h_sizes, _ = G15_CASES[tag]
    x = torch.from_numpy(fx[f"{tag}.x"]).to(DEV)
    key = f"{tag}.p{int(parity)}"
    maf = make(amd, dim, h_sizes, parity, sd=g15_params(tag, parity))
    iaf = make(amd, dim, h_sizes, parity, cls=amd.IAF, sd=g15_params(tag, parity))
    for i, m in enumerate(maf._masked()):
        assert np.array_equal(m.mask.cpu().numpy().astype(np.uint8), fx[f"{tag}.mask{i}"])
    with torch.no_grad():
        y, ld = maf.forward(x)
        assert layer_kernel() == KERNEL
        yi, ldi = iaf.inverse(x)
        assert layer_kernel() == KERNEL
    assert_parity(y, fx[f"{key}.fwd"], fx[f"{key}.fwd64"], what=f"maf_seq_rt G15 {key}")
    # (the reference's float64 forward allocates a float32 log-det: the float64 side comes from the oracle, as in
    # tests/test_hip_maf.py)
    _, ld64 = O.maf(x.cpu().double(), g15_params(tag, parity, torch.float64), O.made_masks(dim, h_sizes, 2 * dim), parity, False)
    assert_parity(ld, fx[f"{key}.ld_fwd"], ld64.numpy(), what=f"maf_seq_rt G15 log_det {key}")
    assert torch.equal(yi, y) and torch.equal(ldi, ld)
    acc = torch.full((x.shape[0],), 0.25, device=DEV)
    with torch.no_grad():
        y2, none = maf._run(x, False, acc)
        assert layer_kernel() == KERNEL
    assert none is None and torch.equal(y2, y)
    assert torch.equal(acc, ld + 0.25)  # one fp32 add of the same sum


# ---------------------------------------------------------------------------------------------------------------------
# 2. shapes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parity", [False, True])
@pytest.mark.parametrize("dim,h_sizes,rows", SEQ_SHAPES)
def test_shapes_vs_oracle(amd, dim, h_sizes, rows, parity):
    z, (y32, ld32), (y64, ld64) = oracle_values(dim, h_sizes, rows, parity)
    y, ld = run(make(amd, dim, h_sizes, parity), z)
    what = f"maf_seq_rt d={dim} h={h_sizes} rows={rows} parity={parity}"
    assert_parity(y, y32, y64, what=what)
    assert_parity(ld, ld32, ld64, what=what + " log_det")
    if (dim, h_sizes, rows) == MANY_BLOCKS:  # the persistent grid is smaller than the row blocks: workgroups loop
        from torch_mnf_amd import _lib

        grid = _lib.load().mnf_maf_seq_rt_grid(rows, dim, len(h_sizes), _lib.int_array(h_sizes))
        blocks = (rows + 127) // 128
        assert 0 < grid and 2 * grid <= blocks, (grid, blocks)


# ---------------------------------------------------------------------------------------------------------------------
# 3. rows do not see each other
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,h_sizes,rows", [(37, (20, 7, 33), 257), (64, (24, 24, 24), 145)])
def test_rows_do_not_see_each_other(amd, dim, h_sizes, rows):
    """The first 130 rows alone (a ragged last tile whose dead lanes read the clamped last row) give the full call's first
    130 rows bit for bit."""
    z = oracle_values(dim, h_sizes, rows, True)[0].to(DEV)
    layer = make(amd, dim, h_sizes, True)
    y, ld = run(layer, z)
    y_head, ld_head = run(layer, z[:130].contiguous())
    assert torch.equal(y_head, y[:130]) and torch.equal(ld_head, ld[:130])


# ---------------------------------------------------------------------------------------------------------------------
# 4. unaligned rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,h_sizes,rows", [(64, (24, 24, 24), 145), (3, (5,), 130), (40, (64,), 129)])
def test_rows_at_a_four_byte_odd_offset(amd, dim, h_sizes, rows):
    """Input and output starting 4 bytes past a 16-byte boundary (the element-by-element row accesses): the aligned call's
    numbers bit for bit."""
    from torch_mnf_amd import _lib

    layer = make(amd, dim, h_sizes, True)
    z = oracle_values(dim, h_sizes, rows, True)[0].to(DEV)
    y, ld = run(layer, z)
    zbuf, ybuf = torch.empty(rows * dim + 1, device=DEV), torch.zeros(rows * dim + 1, device=DEV)
    z_odd, y_odd = zbuf[1:].view(rows, dim), ybuf[1:].view(rows, dim)
    z_odd.copy_(z)
    assert z_odd.data_ptr() % 16 == 4 and y_odd.data_ptr() % 16 == 4
    ld_odd = torch.empty(rows, device=DEV)
    flat, masks = layer._packed(z.device)[0], layer._mask_bytes(z.device)
    layer._launch(z_odd, y_odd, ld_odd, 0, flat, masks, True)
    assert layer_kernel() == KERNEL
    assert torch.equal(y_odd, y) and torch.equal(ld_odd, ld)
    assert float(ybuf[0]) == 0.0  # nothing in front of the first row was written
    y_in, _ = run(layer, z_odd)   # the layer's own call on the odd input (its output is aligned)
    assert torch.equal(y_in, y)
    assert _lib.load().mnf_maf_seq_rt_supported(dim, len(h_sizes), _lib.int_array(h_sizes)) == 1


# ---------------------------------------------------------------------------------------------------------------------
# 5. masked-out weights
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,h_sizes,rows", [(37, (20, 7, 33), 257), (6, (16, 16), 300)])
def test_masked_out_weights_take_no_part(amd, dim, h_sizes, rows):
    """Every masked-out weight set to 0, 1e30, inf: finite outputs, bit for bit the same -- the weight is staged by a select,
    not a multiply, and does not set the staging exponent."""
    z = recipes.gaussian(2600 + dim, rows, dim)
    clean = make(amd, dim, h_sizes, False)
    results = []
    for fill in (0.0, 1e30, float("inf")):
        layer = make(amd, dim, h_sizes, False, sd={k: v.detach().cpu() for k, v in clean.state_dict().items()})
        with torch.no_grad():
            for m in layer._masked():
                assert int((m.mask.T == 0).sum()) > 0
                m.weight.masked_fill_(m.mask.T == 0, fill)
        results.append(run(layer, z))
    y0, ld0 = results[0]
    assert bool(torch.isfinite(y0).all()) and bool(torch.isfinite(ld0).all())
    for y, ld in results[1:]:
        assert torch.equal(y, y0) and torch.equal(ld, ld0)


# ---------------------------------------------------------------------------------------------------------------------
# 6. a permuted MADE
# ---------------------------------------------------------------------------------------------------------------------
def test_a_permuted_made(amd, O):
    """natural_ordering=False: element i's s, t see elements decoded LATER in index order too, which are exactly 0 at step i
    (flows/maf.py:43-50) -- the values are the oracle's with the layer's own masks; gradients of this direction are
    refused as before."""
    from torch_mnf_amd.flows import MADE

    dim, rows = 6, 200
    torch.manual_seed(4)
    net = MADE(dim, (16, 16), 2 * dim, natural_ordering=False)
    flow = amd.MAF(dim, True, net=net)
    flow.force_generic = 2
    flow.to(DEV)
    assert not flow._autoregressive_in_index_order()
    z = 0.5 * recipes.gaussian(31, rows, dim)
    sd = {k: v.detach().cpu() for k, v in flow.state_dict().items()}
    masks = [m.mask.detach().cpu() for m in flow._masked()]
    y, ld = run(flow, z)
    y32, ld32 = O.maf(z, sd, masks, True, False)
    y64, ld64 = O.maf(z.double(), {k: v.double() for k, v in sd.items()}, masks, True, False)
    assert_parity(y, y32.numpy(), y64.numpy(), what="maf_seq_rt permuted MADE")
    assert_parity(ld, ld32.numpy(), ld64.numpy(), what="maf_seq_rt permuted MADE log_det")
    with pytest.raises(NotImplementedError, match="natural_ordering"):
        flow.forward(z.to(DEV).requires_grad_(True))


# ---------------------------------------------------------------------------------------------------------------------
# 7. autograd through the new forward
# ---------------------------------------------------------------------------------------------------------------------
def _grad_case(name):
    if name == "d12":
        dim, h_sizes, rows = G15_CASES["d12"]
        return dim, h_sizes, rows, g15_params("d12", True)
    return 6, (16, 16), 200, params(6, (16, 16))


@pytest.mark.parametrize("name", ["d6", "d12"])
def test_autograd_through_the_new_forward(amd, O, golden, name):
    """forward on maf_seq_rt, backward on maf_bwd_generic (it needs x and y only); gradients against autograd through the
    float64 oracle; masked-out weights get exactly zero."""
    dim, h_sizes, rows, sd = _grad_case(name)
    z = torch.from_numpy(golden("g15_maf_iaf")["d12.x"]) if name == "d12" else recipes.gaussian(2600 + dim, rows, dim)
    masks = O.made_masks(dim, h_sizes, 2 * dim)
    w_y, w_l = recipes.gaussian(2700 + dim, rows, dim), recipes.gaussian(2701 + dim, rows, 1)[:, 0]
    layer = make(amd, dim, h_sizes, True, sd=sd)
    zz = z.to(DEV).requires_grad_(True)
    y, ld = layer.forward(zz)
    assert layer_kernel() == KERNEL
    ((y * w_y.to(DEV)).sum() + (ld * w_l.to(DEV)).sum()).backward()
    assert layer_kernel() == "maf_bwd_generic"
    got = {"x": zz.grad, **{n: p.grad for n, p in layer.named_parameters()}}
    ref = OracleGrads(cot_loss(lambda xx, p: O.maf(xx, p, masks, True, False), w_y, w_l), z, sd)
    ref.check_all(got, f"maf_seq_rt forward + maf_bwd_generic {name}")
    for m in layer._masked():
        assert float((m.weight.grad * (m.mask.T == 0)).abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# 8. a model
# ---------------------------------------------------------------------------------------------------------------------
def test_three_layer_model_forward_and_sample(amd, O):
    """3 MAF layers of alternating parity in a NormalizingFlowModel, 2,049 rows: model.forward's last output and summed
    log_det against oracle.apply_layer looped; model.sample runs the kernel."""
    dim, h_sizes, rows = 6, (16, 16), 2049
    sds = [recipes.maf_params(2800 + i, dim, h_sizes, gain=1.2, last_gain=0.5) for i in range(3)]
    masks = O.made_masks(dim, h_sizes, 2 * dim)
    flows = [make(amd, dim, h_sizes, i % 2 == 0, sd=sds[i]) for i in range(3)]
    model = amd.NormalizingFlowModel(amd.StandardNormal(dim, DEV), flows).to(DEV)
    z = recipes.gaussian(2801, rows, dim)
    with torch.no_grad():
        xs, ld = model.forward(z.to(DEV))
    assert layer_kernel() == KERNEL
    ref = {}
    for dt in (torch.float32, torch.float64):
        x, total = z.to(dt), torch.zeros(rows, dtype=dt)
        for i in range(3):
            spec = {"kind": "maf", "parity": i % 2 == 0, "masks": masks, "params": {k: v.to(dt) for k, v in sds[i].items()}}
            x, step = O.apply_layer(spec, x, False)
            total = total + step
        ref[dt] = (x.numpy(), total.numpy())
    assert_parity(xs[-1], ref[torch.float32][0], ref[torch.float64][0], what="3 x maf_seq_rt forward, 2,049 rows")
    assert_parity(ld, ref[torch.float32][1], ref[torch.float64][1], what="3 x maf_seq_rt log_det, 2,049 rows")
    with torch.no_grad():
        s = model.sample(64)
    assert layer_kernel() == KERNEL
    assert s.shape == (64, dim) and bool(torch.isfinite(s).all())


# ---------------------------------------------------------------------------------------------------------------------
# 9. / 10. routes
# ---------------------------------------------------------------------------------------------------------------------
def test_fallback_for_a_shape_without_a_plan(amd, O):
    dim, h_sizes, rows = 6, (3,), 100
    sd, masks = params(dim, h_sizes), O.made_masks(dim, h_sizes, 2 * dim)
    z = recipes.gaussian(2600 + dim, rows, dim)
    layer = make(amd, dim, h_sizes, True)
    with torch.no_grad():
        y, ld = layer.forward(z.to(DEV))
    assert layer_kernel() == "maf_generic"
    y32, ld32 = O.maf(z, sd, masks, True, False)
    y64, ld64 = O.maf(z.double(), {k: v.double() for k, v in sd.items()}, masks, True, False)
    assert_parity(y, y32.numpy(), y64.numpy(), what="maf_generic fallback of maf_seq_rt")
    assert_parity(ld, ld32.numpy(), ld64.numpy(), what="maf_generic fallback of maf_seq_rt log_det")


def test_default_route_switches_at_the_threshold(amd, O, monkeypatch):
    """At MAF_SEQ_RT_MIN_ROWS rows: maf_seq_rt; one row below: maf_generic; an fp32 request and force_generic = 1 stay on it.
    (With the default None -- opt-in -- the threshold under test is RT_MIN_ROWS, the lowest it may ever be.)  The two
    kernels' outputs on the shared rows agree within the sum of the budgets assert_parity gives each against the oracle."""
    from torch_mnf_amd import _dispatch

    if _dispatch.MAF_SEQ_RT_MIN_ROWS is None:
        monkeypatch.setattr(_dispatch, "MAF_SEQ_RT_MIN_ROWS", _dispatch.RT_MIN_ROWS)
    n = _dispatch.MAF_SEQ_RT_MIN_ROWS
    assert n >= _dispatch.RT_MIN_ROWS
    dim, h_sizes = 6, (16, 16)
    sd, masks = params(dim, h_sizes), O.made_masks(dim, h_sizes, 2 * dim)
    layer = make(amd, dim, h_sizes, True, force=0)
    z = recipes.gaussian(2900, n, dim)
    with torch.no_grad():
        y_at, ld_at = layer.forward(z.to(DEV))
        assert layer_kernel() == KERNEL
        y_below, ld_below = layer.forward(z[:n - 1].to(DEV))
        assert layer_kernel() == "maf_generic"
    y32, ld32 = O.maf(z, sd, masks, True, False)
    y64, ld64 = O.maf(z.double(), {k: v.double() for k, v in sd.items()}, masks, True, False)
    for got_at, got_below, r32, r64, what in ((y_at, y_below, y32, y64, "y"), (ld_at, ld_below, ld32, ld64, "log_det")):
        r32, r64 = r32.numpy(), r64.numpy()
        assert_parity(got_at, r32, r64, what=f"maf_seq_rt at the threshold {what}")
        assert_parity(got_below, r32[:n - 1], r64[:n - 1], what=f"maf_generic below the threshold {what}")
        budget = (RTOL + 2 * normwise_err(r32, r64)) + (RTOL + 2 * normwise_err(r32[:n - 1], r64[:n - 1]))
        assert normwise_err(got_below.cpu().numpy(), got_at[:n - 1].cpu().numpy()) <= budget, what
    layer.force_fp32_mfma = True
    with torch.no_grad():
        layer.forward(z.to(DEV))
    assert layer_kernel() == "maf_generic"
    layer.force_fp32_mfma = False
    layer.force_generic = 1
    with torch.no_grad():
        layer.forward(z.to(DEV))
    assert layer_kernel() == "maf_generic"
