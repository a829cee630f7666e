"""GPU tests of the one-pass direction of MAF / IAF on the matrix cores (``mnf_maf_rt`` / ``mnf_maf_bwd_rt`` behind
``flows.MAF`` / ``flows.IAF``, kernel families ``maf_rt`` / ``maf_bwd_rt``): the reference's own runs (fixture G15), shapes
on every path of the kernels against the oracle, masked-out weights, gradients against autograd through the float64
oracle, the default route's threshold, fixed-order sums in a child process and a 3-layer model's log-prob.

Every case names the kernel it ran (``last_kernel()``).  Tolerances are the project's: ``helpers.assert_parity`` for values
(1e-5 normwise plus twice the fp32 oracle's distance from the float64 oracle), ``OracleGrads.check`` for gradients (1e-5
plus twice the fp32 oracle gradients' distance from the float64 ones); both are recorded for tests/test_zz_audit.py."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import recipes
from helpers import RTOL, assert_close, assert_parity
from test_hip_autograd import OracleGrads, cot_loss
from test_oracle_golden import G15_CASES, g15_params

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (dim, h_sizes, rows): the reference's shape | odd dim, unaligned rows, two row blocks with a ragged end | odd widths, three
# row blocks | one wide layer, dim % 4 == 0 with an odd row count | resident, several blocks | four layers, dim > 64 |
# streaming (144 blocks of weights do not fit LDS) | a workgroup takes several row blocks
SHAPES = [(2, (24, 24, 24), 17), (3, (5,), 130), (37, (20, 7, 33), 257), (40, (64,), 129), (64, (24, 24, 24), 2065),
          (100, (16,) * 4, 33), (130, (128, 128), 145), (6, (8,), 70003)]
GRAD_SHAPES = [s for s in SHAPES if max(s[1]) <= 64] + [(130, (64, 64), 145)]
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


def make(amd, dim, h_sizes, parity, cls=None, force=2, sd=None):
    layer = (cls or amd.MAF)(dim, parity=parity, h_sizes=h_sizes)
    sd = sd if sd is not None else params(dim, h_sizes)
    missing = layer.load_state_dict(sd, strict=False)
    assert all(k.endswith(".mask") for k in missing.missing_keys) and not missing.unexpected_keys
    layer.force_generic = force
    return layer.to(DEV)


def params(dim, h_sizes):
    return recipes.maf_params(2100 + dim + len(h_sizes), dim, h_sizes, gain=1.2, last_gain=0.5)


def one_pass(layer, x):
    """the one-pass direction of either class: MAF.inverse, IAF.forward"""
    return layer.forward(x) if type(layer).__name__ == "IAF" else layer.inverse(x)


@functools.lru_cache(maxsize=None)
def oracle_values(dim, h_sizes, rows, parity):
    """(x, fp32 (y, log_det), fp64 (y, log_det)) of the one-pass direction: computed once, shared, never written to"""
    from oracle import flow_oracle as O

    sd, masks = params(dim, h_sizes), O.made_masks(dim, h_sizes, 2 * dim)
    x = recipes.gaussian(2200 + dim, rows, dim)
    y32, ld32 = O.maf(x, sd, masks, parity, True)
    y64, ld64 = O.maf(x.double(), {k: v.double() for k, v in sd.items()}, masks, parity, True)
    return x, (y32.numpy(), ld32.numpy()), (y64.numpy(), ld64.numpy())


@functools.lru_cache(maxsize=None)
def oracle_grads(dim, h_sizes, rows, parity, which="both"):
    from oracle import flow_oracle as O

    masks = O.made_masks(dim, h_sizes, 2 * dim)
    x = oracle_values(dim, h_sizes, rows, parity)[0]
    w_y, w_l = cotangents(dim, rows, which)
    return OracleGrads(cot_loss(lambda xx, p: O.maf(xx, p, masks, parity, True), w_y, w_l), x, params(dim, h_sizes))


def cotangents(dim, rows, which="both"):
    w_y, w_l = recipes.gaussian(2300 + dim, rows, dim), recipes.gaussian(2301 + dim, rows, 1)[:, 0]
    return (w_y if which != "ld" else torch.zeros_like(w_y)), (w_l if which != "y" else torch.zeros_like(w_l))


def backward(layer, x_cpu, w_y, w_l, which="both"):
    """loss = sum(y w_y) + sum(log_det w_l) through the layer; which = "y" / "ld": the other output takes no part at all
    (its cotangent reaches the kernel as None)"""
    for p in layer.parameters():  # (in place: a FlatParameters home keeps its views)
        if p.grad is not None:
            p.grad.zero_()
    x = x_cpu.to(DEV).requires_grad_(True)
    y, ld = one_pass(layer, x)
    fwd_kernel = layer_kernel()
    loss = 0
    if which != "ld":
        loss = loss + (y * w_y.to(DEV)).sum()
    if which != "y":
        loss = loss + (ld * w_l.to(DEV)).sum()
    loss.backward()
    torch.cuda.synchronize()
    got = {"x": x.grad, **{n: p.grad for n, p in layer.named_parameters()}}
    return got, fwd_kernel, layer_kernel(), (y.detach(), ld.detach())


def layer_kernel():
    import torch_mnf_amd

    torch.cuda.synchronize()
    return torch_mnf_amd.last_kernel()


# ---------------------------------------------------------------------------------------------------------------------
# values
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parity", [False, True])
@pytest.mark.parametrize("tag", sorted(G15_CASES))
def test_g15_reference_runs_on_the_rt_kernel(amd, golden, tag, parity):
    """Fixture G15, the reference's own MAF.inverse runs (flows/maf.py:53-62), through force_generic = 2; IAF.forward is the
    same launch: bit for bit.  log_det accumulation as NormalizingFlow's loop uses it."""
    fx = golden("g15_maf_iaf")
    dim, h_sizes, _ = G15_CASES[tag]
    x = torch.from_numpy(fx[f"{tag}.x"]).to(DEV)
    key = f"{tag}.p{int(parity)}"
    maf = make(amd, dim, h_sizes, parity, sd=g15_params(tag, parity))
    iaf = make(amd, dim, h_sizes, parity, cls=amd.IAF, sd=g15_params(tag, parity))
    for i, m in enumerate(maf._masked()):
        assert np.array_equal(m.mask.cpu().numpy().astype(np.uint8), fx[f"{tag}.mask{i}"])
    with torch.no_grad():
        y, ld = maf.inverse(x)
        assert layer_kernel() == "maf_rt"
        yi, ldi = iaf.forward(x)
        assert layer_kernel() == "maf_rt"
    assert_parity(y, fx[f"{key}.inv"], fx[f"{key}.inv64"], what=f"maf_rt G15 {key}")
    assert_parity(ld, fx[f"{key}.ld_inv"], fx[f"{key}.ld_inv64"], what=f"maf_rt G15 log_det {key}")
    assert torch.equal(yi, y) and torch.equal(ldi, ld)
    acc = torch.full((x.shape[0],), 0.25, device=DEV)
    with torch.no_grad():
        y2, none = maf._run(x, True, acc)
        assert layer_kernel() == "maf_rt"
    assert none is None and torch.equal(y2, y)
    assert torch.equal(acc, ld + 0.25)  # one fp32 add of the same sum
    assert_close(acc, fx[f"{key}.ld_inv"] + 0.25, RTOL, "accumulated log_det")


@pytest.mark.parametrize("parity", [False, True])
@pytest.mark.parametrize("dim,h_sizes,rows", SHAPES)
def test_forward_shapes_vs_oracle(amd, dim, h_sizes, rows, parity):
    x, (y32, ld32), (y64, ld64) = oracle_values(dim, h_sizes, rows, parity)
    layer = make(amd, dim, h_sizes, parity)
    with torch.no_grad():
        y, ld = layer.inverse(x.to(DEV))
    assert layer_kernel() == "maf_rt"
    what = f"maf_rt d={dim} h={h_sizes} rows={rows} parity={parity}"
    assert_parity(y, y32, y64, what=what)
    assert_parity(ld, ld32, ld64, what=what + " log_det")
    if (dim, h_sizes, rows) == MANY_BLOCKS:  # the persistent grid is smaller than the row blocks: workgroups loop
        from torch_mnf_amd import _lib

        grid = _lib.load().mnf_maf_rt_grid(rows, dim, len(h_sizes), _lib.int_array(h_sizes))
        blocks = (rows + 127) // 128
        assert 0 < grid and 2 * grid <= blocks, (grid, blocks)


@pytest.mark.parametrize("dim,h_sizes,rows", [(64, (24, 24, 24), 2065), (3, (5,), 130), (40, (64,), 129)])
def test_rows_at_a_four_byte_odd_offset(amd, dim, h_sizes, rows):
    """An input (and, in the gradient pass, a cotangent) that starts 4 bytes past a 16-byte boundary: the element-by-element
    variant, the same numbers as the aligned call bit for bit."""
    x_cpu = oracle_values(dim, h_sizes, rows, True)[0]
    layer = make(amd, dim, h_sizes, True)
    x = x_cpu.to(DEV)
    buf = torch.empty(rows * dim + 1, device=DEV)
    odd = buf[1:].view(rows, dim)
    odd.copy_(x)
    assert odd.data_ptr() % 16 == 4 and odd.is_contiguous()
    with torch.no_grad():
        y, ld = layer.inverse(x)
        y_odd, ld_odd = layer.inverse(odd)
    assert layer_kernel() == "maf_rt"
    assert torch.equal(y_odd, y) and torch.equal(ld_odd, ld)
    if max(h_sizes) <= 64:
        w_y, w_l = cotangents(dim, rows)
        ref = backward(layer, x_cpu, w_y, w_l)[0]
        ref = {k: v.clone() for k, v in ref.items()}
        for p in layer.parameters():
            p.grad = None
        xg = odd.detach().requires_grad_(True)
        yy, ll = layer.inverse(xg)
        wbuf = torch.empty(rows * dim + 1, device=DEV)
        wbuf[1:].copy_(w_y.to(DEV).reshape(-1))
        torch.autograd.backward([yy, ll], [wbuf[1:].view(rows, dim), w_l.to(DEV)])
        assert layer_kernel() == "maf_bwd_rt"
        assert torch.equal(xg.grad, ref["x"])
        for n, p in layer.named_parameters():  # (atomic sums: the order of the adds differs run to run)
            assert_close(p.grad, ref[n], 2e-6, f"{n} at an odd offset")


def test_a_permuted_made(amd, O):
    """natural_ordering=False (made.py's default): the masks are no longer triangular in index order; the one-pass direction
    takes them as they are."""
    from torch_mnf_amd.flows import MADE

    dim, rows = 6, 200
    torch.manual_seed(4)
    net = MADE(dim, (16, 16), 2 * dim, natural_ordering=False)
    flow = amd.MAF(dim, True, net=net)
    flow.force_generic = 2
    flow.to(DEV)
    assert not flow._autoregressive_in_index_order()
    x = 0.5 * recipes.gaussian(31, rows, dim)
    sd = {k: v.detach().cpu() for k, v in flow.state_dict().items()}
    masks = [m.mask.detach().cpu() for m in flow._masked()]
    w_y, w_l = cotangents(dim, rows)
    got, fwd_kernel, bwd_kernel, (y, ld) = backward(flow, x, w_y, w_l)
    assert (fwd_kernel, bwd_kernel) == ("maf_rt", "maf_bwd_rt")
    y32, ld32 = O.maf(x, sd, masks, True, True)
    y64, ld64 = O.maf(x.double(), {k: v.double() for k, v in sd.items()}, masks, True, True)
    assert_parity(y, y32.numpy(), y64.numpy(), what="maf_rt permuted MADE")
    assert_parity(ld, ld32.numpy(), ld64.numpy(), what="maf_rt permuted MADE log_det")
    psd = {k: v for k, v in sd.items() if not k.endswith("mask")}
    ref = OracleGrads(cot_loss(lambda xx, p: O.maf(xx, p, masks, True, True), w_y, w_l), x, psd)
    ref.check_all(got, "maf_bwd_rt permuted MADE")


# ---------------------------------------------------------------------------------------------------------------------
# masked-out weights
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,h_sizes,rows", [(37, (20, 7, 33), 257), (6, (16, 16), 2065)])
def test_masked_out_weights_take_no_part(amd, dim, h_sizes, rows):
    """Every masked-out weight set to 1e30 (then to inf): outputs and gradients bit for bit those with zeros there -- the
    weight is staged by a select, not a multiply, and does not set the staging exponent --; their gradient entries
    receive no add at all."""
    x = oracle_values(dim, h_sizes, rows, False)[0]
    w_y, w_l = cotangents(dim, rows)
    clean = make(amd, dim, h_sizes, False)
    with torch.no_grad():
        for m in clean._masked():
            m.weight.mul_(m.mask.T != 0)  # exact zeros in the masked-out slots
    results = []
    for fill in (0.0, 1e30, float("inf")):
        layer = make(amd, dim, h_sizes, False, sd={k: v.detach().cpu() for k, v in clean.state_dict().items()})
        with torch.no_grad():
            for m in layer._masked():
                m.weight.masked_fill_(m.mask.T == 0, fill)
        got, fwd_kernel, bwd_kernel, (y, ld) = backward(layer, x, w_y, w_l)
        assert (fwd_kernel, bwd_kernel) == ("maf_rt", "maf_bwd_rt")
        for m in layer._masked():
            dead = m.weight.grad[m.mask.T == 0]
            assert dead.numel() > 0 and bool((dead.view(torch.int32) == 0).all()), "a masked-out weight received an add"
        results.append((y, ld, got["x"]))
    y0, ld0, gx0 = results[0]
    assert bool(torch.isfinite(y0).all()) and bool(torch.isfinite(gx0).all())
    for y, ld, gx in results[1:]:
        assert torch.equal(y, y0) and torch.equal(ld, ld0) and torch.equal(gx, gx0)


# ---------------------------------------------------------------------------------------------------------------------
# gradients
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parity", [False, True])
@pytest.mark.parametrize("dim,h_sizes,rows", GRAD_SHAPES)
def test_gradients_vs_float64_oracle(amd, dim, h_sizes, rows, parity):
    x = oracle_values(dim, h_sizes, rows, parity)[0]
    w_y, w_l = cotangents(dim, rows)
    layer = make(amd, dim, h_sizes, parity)
    got, fwd_kernel, bwd_kernel, _ = backward(layer, x, w_y, w_l)
    assert (fwd_kernel, bwd_kernel) == ("maf_rt", "maf_bwd_rt")
    oracle_grads(dim, h_sizes, rows, parity).check_all(got, f"maf_bwd_rt d={dim} h={h_sizes} rows={rows} parity={parity}")
    for m in layer._masked():
        assert float((m.weight.grad * (m.mask.T == 0)).abs().max()) == 0.0


@pytest.mark.parametrize("which", ["y", "ld"])
@pytest.mark.parametrize("dim,h_sizes,rows", [(37, (20, 7, 33), 257), (64, (24, 24, 24), 2065)])
def test_gradients_with_one_cotangent_missing(amd, dim, h_sizes, rows, which):
    x = oracle_values(dim, h_sizes, rows, True)[0]
    w_y, w_l = cotangents(dim, rows, which)
    layer = make(amd, dim, h_sizes, True)
    got, _, bwd_kernel, _ = backward(layer, x, w_y, w_l, which)
    assert bwd_kernel == "maf_bwd_rt"
    oracle_grads(dim, h_sizes, rows, True, which).check_all(got, f"maf_bwd_rt d={dim} h={h_sizes} grad_{which} only")


def test_a_layer_homed_in_flat_parameters(amd):
    """The gradient launch adds into the FlatParameters buffer in place: the same sums as the un-homed layer's (float
    atomics: the order of the adds differs), and p.grad stays the buffer's view."""
    dim, h_sizes, rows = 37, (20, 7, 33), 257
    x = oracle_values(dim, h_sizes, rows, True)[0]
    w_y, w_l = cotangents(dim, rows)
    plain, homed = make(amd, dim, h_sizes, True), make(amd, dim, h_sizes, True)
    flat = amd.FlatParameters(homed)
    g_plain, _, k_plain, _ = backward(plain, x, w_y, w_l)
    g_homed, _, k_homed, _ = backward(homed, x, w_y, w_l)
    assert k_plain == k_homed == "maf_bwd_rt"
    assert torch.equal(g_homed["x"], g_plain["x"])
    for (n, p0), (_, p1) in zip(plain.named_parameters(), homed.named_parameters()):
        assert_close(p1.grad, p0.grad, 2e-6, n)
    assert all(p.grad is v for p, v in zip(flat.params, flat._grad_views))


# ---------------------------------------------------------------------------------------------------------------------
# routes
# ---------------------------------------------------------------------------------------------------------------------
def test_default_route_switches_at_the_threshold(amd, monkeypatch):
    """At MAF_RT_MIN_ROWS rows: maf_rt / maf_bwd_rt; one row below: the VALU kernels; an fp32 request stays on them.  (Were
    the default None -- opt-in -- the threshold under test would be RT_MIN_ROWS, the lowest it may ever be.)"""
    from torch_mnf_amd import _dispatch

    if _dispatch.MAF_RT_MIN_ROWS is None:
        monkeypatch.setattr(_dispatch, "MAF_RT_MIN_ROWS", _dispatch.RT_MIN_ROWS)
    n = _dispatch.MAF_RT_MIN_ROWS
    assert n >= _dispatch.RT_MIN_ROWS
    dim, h_sizes = 6, (16, 16)
    layer = make(amd, dim, h_sizes, True, force=0)
    w_y, w_l = cotangents(dim, n)
    x = recipes.gaussian(2400, n, dim)
    at, k_fwd, k_bwd, (y_at, _) = backward(layer, x, w_y, w_l)
    assert (k_fwd, k_bwd) == ("maf_rt", "maf_bwd_rt")
    at = {k: v.clone() for k, v in at.items()}
    below, k_fwd, k_bwd, (y_below, _) = backward(layer, x[:n - 1], w_y[:n - 1], w_l[:n - 1])
    assert (k_fwd, k_bwd) == ("maf_generic", "maf_bwd_generic")
    assert_close(y_below, y_at[:n - 1], 2e-6, "the two kernels' outputs")
    assert_close(below["x"], at["x"][:n - 1], 2e-5, "the two kernels' grad_x")
    layer.force_fp32_mfma = True
    _, k_fwd, k_bwd, _ = backward(layer, x, w_y, w_l)
    assert (k_fwd, k_bwd) == ("maf_generic", "maf_bwd_generic")
    layer.force_fp32_mfma = False
    with torch.no_grad():  # the element-by-element direction: never
        layer.forward(x[:64].to(DEV))
    assert layer_kernel() == "maf_generic"
    layer.force_generic = 1
    _, k_fwd, k_bwd, _ = backward(layer, x, w_y, w_l)
    assert (k_fwd, k_bwd) == ("maf_generic", "maf_bwd_generic")


def test_fixed_order_sums_in_a_child_process(amd):
    """MNF_DETERMINISTIC=1 is read once per process: a fresh child runs two backward passes of one shape on the fixed-order
    form (bit-identical grad_flat, no atomic-sums warning) -- tests/maf_rt_deterministic_child.py; without the switch
    (this process) the atomic entry runs and the fixed-order one is not asked for."""
    assert not amd.deterministic()
    from torch_mnf_amd import _lib

    dim, h_sizes, rows = 37, (20, 7, 33), 257
    lib, hid = _lib.load(), _lib.int_array(h_sizes)
    calls = []
    real = lib.mnf_maf_bwd_rt_det
    x = oracle_values(dim, h_sizes, rows, False)[0]
    w_y, w_l = cotangents(dim, rows)
    layer = make(amd, dim, h_sizes, False)
    try:
        lib.mnf_maf_bwd_rt_det = lambda *a: calls.append(a) or real(*a)
        _, _, k_bwd, _ = backward(layer, x, w_y, w_l)
    finally:
        lib.mnf_maf_bwd_rt_det = real
    assert k_bwd == "maf_bwd_rt" and not calls
    assert lib.mnf_maf_bwd_rt_det_workspace(rows, dim, len(h_sizes), hid) > 0
    env = dict(os.environ, MNF_DETERMINISTIC="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "maf_rt_deterministic_child.py")], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    tail = "\n".join((p.stdout + p.stderr).splitlines()[-30:])
    assert p.returncode == 0, tail
    assert "maf rt deterministic child ok" in p.stdout, tail


def test_three_layer_model_log_prob(amd, O):
    """NormalizingFlowModel.log_prob of 3 MAF layers of alternating parity at 2,065 rows against oracle.flow_stack: log_det
    accumulated across the launches."""
    dim, h_sizes, rows = 6, (16, 16), 2065
    sds = [recipes.maf_params(2500 + i, dim, h_sizes, gain=1.2, last_gain=0.5) for i in range(3)]
    masks = O.made_masks(dim, h_sizes, 2 * dim)
    flows = [make(amd, dim, h_sizes, i % 2 == 0, sd=sds[i]) for i in range(3)]
    model = amd.NormalizingFlowModel(amd.StandardNormal(dim, DEV), flows).to(DEV)
    x = recipes.gaussian(2501, rows, dim)
    with torch.no_grad():
        lp = model.log_prob(x.to(DEV))
    assert layer_kernel() == "maf_rt"
    ref = {}
    for dt in (torch.float32, torch.float64):
        layers = [{"kind": "maf", "parity": i % 2 == 0, "masks": masks, "params": {k: v.to(dt) for k, v in sds[i].items()}}
                  for i in range(3)]
        ref[dt] = O.mean_log_prob(x.to(dt), layers)[1].numpy()
    assert_parity(lp, ref[torch.float32], ref[torch.float64], what="3 x maf_rt log_prob, 2,065 rows")
