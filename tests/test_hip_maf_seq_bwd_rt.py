"""GPU tests of the gradients of the element-by-element direction of MAF / IAF on the matrix cores (``mnf_maf_seq_bwd_rt``
behind ``MAF.forward`` / ``IAF.inverse`` under ``backward()``, kernel family ``maf_seq_bwd_rt``): shapes on
every path of the solve kernel against autograd through the float64 oracle, the reference's own case (fixture G15), single
cotangents, mean-loss magnitudes, independence of the rows, unaligned rows, masked-out weights, the parent's route, the
fallbacks, a 3-layer IAF model's ``-log_prob.mean()`` and the fixed-order form in a child process.

The route is opt-in: every test sets ``_dispatch.MAF_SEQ_BWD_RT_MIN_ROWS`` (0 unless said otherwise) and uses
``force_generic = 2``.  Every case names the kernel it ran.  Tolerance: the project's own rule, ``OracleGrads.check_all`` /
``check_vs_float64`` (1e-5 normwise plus twice the fp32 oracle gradients' distance from the float64 ones), recorded for
tests/test_zz_audit.py."""
import functools
import math
import os
import subprocess
import sys

import pytest
import torch

import recipes
from helpers import normwise_err
from test_hip_autograd import GBASE, OracleGrads, check_vs_float64, cot_loss
from test_oracle_golden import G15_CASES, g15_params

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL, PARENT = "maf_seq_bwd_rt", "maf_bwd_generic"

# (dim, h_sizes, rows): the reference's shape, one ragged tile | odd dim and width, two row blocks | two layers, three row
# blocks | odd widths, three layers, dim % 4 != 0 | one wide layer, dim % 4 == 0 | four input tiles, narrow layers | the
# largest plan (four waves per workgroup) | four hidden layers, seven input tiles (dim > 64)
SHAPES = [(2, (24, 24, 24), 17), (3, (5,), 130), (6, (16, 16), 300), (37, (20, 7, 33), 257), (40, (64,), 129),
          (64, (24, 24, 24), 145), (64, (64, 64), 145), (100, (16,) * 4, 33)]
ODD = (37, (20, 7, 33), 257)
WIDE = (64, (24, 24, 24), 145)


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
    from torch_mnf_amd import _dispatch

    monkeypatch.setattr(_dispatch, "MAF_SEQ_BWD_RT_MIN_ROWS", 0)


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


def inputs(dim, rows):
    return (recipes.gaussian(2600 + dim, rows, dim), recipes.gaussian(2700 + dim, rows, dim),
            recipes.gaussian(2701 + dim, rows, 1)[:, 0])


@functools.lru_cache(maxsize=None)
def oracle(dim, h_sizes, rows, parity, which="both"):
    """autograd through the oracle's element-by-element pass, fp32 and fp64: computed once, shared, never written"""
    from oracle import flow_oracle as O

    z, w_y, w_l = inputs(dim, rows)
    masks = O.made_masks(dim, h_sizes, 2 * dim)
    fn = lambda xx, p: O.maf(xx, p, masks, parity, False)  # noqa: E731
    if which == "both":
        loss = cot_loss(fn, w_y, w_l)
    elif which == "y":
        loss = lambda x, p, dt: (fn(x, p)[0] * w_y.to(dt)).sum()  # noqa: E731
    else:
        loss = lambda x, p, dt: (fn(x, p)[1] * w_l.to(dt)).sum()  # noqa: E731
    return OracleGrads(loss, z, params(dim, h_sizes))


def backward(layer, z, w_y, w_l, expect=KERNEL):
    """gradients of sum(y w_y) + sum(log_det w_l) through the layer's element-by-element direction"""
    layer.zero_grad()
    zz = z.to(DEV).requires_grad_(True)
    y, ld = sequential(layer, zz)
    ((y * w_y.to(DEV)).sum() + (ld * w_l.to(DEV)).sum()).backward()
    assert layer_kernel() == expect
    return {"x": zz.grad, **{n: p.grad.clone() for n, p in layer.named_parameters()}}


def masked_entries_are_zero(layer, got):
    for i, m in enumerate(layer._masked()):
        g = got[f"net.{2 * i}.weight"]
        assert float((g * (m.mask.T == 0)).abs().max()) == 0.0


def raw_call(layer, y, gy, gl, gx=None, det=False):
    """mnf_maf_seq_bwd_rt (det: mnf_maf_seq_bwd_rt_det, the fixed-order form, which any process may call) itself on device
    tensors (grad_y / grad_ld may be None: NULL): (grad_x, grad_flat)"""
    from torch_mnf_amd import _lib
    from torch_mnf_amd.flows import _grad_scale

    lib = _lib.load()
    rows, dim = y.shape
    flat, masks = layer._packed(y.device)[0], layer._mask_bytes(y.device)
    gx = torch.empty(rows, dim, device=DEV) if gx is None else gx
    gf = torch.zeros_like(flat)
    scale = _grad_scale(gy, gl, rows, dim, y.device)
    n_ws = (lib.mnf_maf_seq_bwd_rt_det_workspace(rows, dim, len(layer.h_sizes), layer._hid) if det
            else lib.mnf_maf_seq_bwd_rt_workspace(rows, dim))
    ws = torch.empty(n_ws, device=DEV)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    entry = lib.mnf_maf_seq_bwd_rt_det if det else lib.mnf_maf_seq_bwd_rt
    rc = entry(y.data_ptr(), ptr(gy), ptr(gl), gx.data_ptr(), gf.data_ptr(), flat.data_ptr(), masks.data_ptr(),
               scale.data_ptr(), rows, dim, int(bool(layer.parity)), len(layer.h_sizes), layer._hid, ws.data_ptr(), n_ws, None)
    assert rc == 0, rc
    assert layer_kernel() == KERNEL
    return gx, gf


def flat_grads(layer, gf):
    """grad_flat -> the layer's named parameters (state_dict order: weight, bias per MaskedLinear)"""
    out, off = {}, 0
    for i, m in enumerate(layer._masked()):
        for name, p in ((f"net.{2 * i}.weight", m.weight), (f"net.{2 * i}.bias", m.bias)):
            out[name] = gf[off:off + p.numel()].view(p.shape)
            off += p.numel()
    assert off == gf.numel()
    return out


# ---------------------------------------------------------------------------------------------------------------------
# 1. shapes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parity", [False, True])
@pytest.mark.parametrize("dim,h_sizes,rows", SHAPES)
def test_shapes_vs_float64_oracle(amd, dim, h_sizes, rows, parity):
    from torch_mnf_amd import _lib

    assert _lib.load().mnf_maf_seq_bwd_rt_supported(dim, len(h_sizes), _lib.int_array(h_sizes)) == 1
    layer = make(amd, dim, h_sizes, parity)
    got = backward(layer, *inputs(dim, rows))
    oracle(dim, h_sizes, rows, parity).check_all(got, f"maf_seq_bwd_rt d={dim} h={h_sizes} rows={rows} parity={parity}")
    masked_entries_are_zero(layer, got)


@pytest.mark.parametrize("dim,h_sizes,rows", [SHAPES[2], ODD])
def test_iaf_inverse_is_the_same_pass(amd, dim, h_sizes, rows):
    layer = make(amd, dim, h_sizes, True, cls=amd.IAF)
    got = backward(layer, *inputs(dim, rows))
    oracle(dim, h_sizes, rows, True).check_all(got, f"maf_seq_bwd_rt IAF.inverse d={dim} h={h_sizes} rows={rows}")
    masked_entries_are_zero(layer, got)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the reference's own case
# ---------------------------------------------------------------------------------------------------------------------
def test_g15_d12(amd, O, golden):
    dim, h_sizes, rows = G15_CASES["d12"]
    sd = g15_params("d12", True)
    z = torch.from_numpy(golden("g15_maf_iaf")["d12.x"])
    masks = O.made_masks(dim, h_sizes, 2 * dim)
    w_y, w_l = recipes.gaussian(2700 + dim, rows, dim), recipes.gaussian(2701 + dim, rows, 1)[:, 0]
    layer = make(amd, dim, h_sizes, True, sd=sd)
    got = backward(layer, z, w_y, w_l)
    ref = OracleGrads(cot_loss(lambda xx, p: O.maf(xx, p, masks, True, False), w_y, w_l), z, sd)
    ref.check_all(got, "maf_seq_bwd_rt G15 d12")
    masked_entries_are_zero(layer, got)


# ---------------------------------------------------------------------------------------------------------------------
# 3. single cotangents: the other one reaches the kernel as NULL
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["y", "ld"])
def test_single_cotangents(amd, which):
    dim, h_sizes, rows = ODD
    layer = make(amd, dim, h_sizes, True)
    z, w_y, w_l = inputs(dim, rows)
    with torch.no_grad():
        y, _ = layer.forward(z.to(DEV))
    gx, gf = raw_call(layer, y, w_y.to(DEV) if which == "y" else None, w_l.to(DEV) if which == "ld" else None)
    got = {"x": gx, **flat_grads(layer, gf)}
    oracle(dim, h_sizes, rows, True, which).check_all(got, f"maf_seq_bwd_rt grad_{which} only d={dim}")
    masked_entries_are_zero(layer, got)


# ---------------------------------------------------------------------------------------------------------------------
# 4. mean-loss magnitude
# ---------------------------------------------------------------------------------------------------------------------
def test_cotangents_of_a_mean_loss_magnitude(amd):
    """The cotangents times 2^-17 (a mean over 131,072 rows): every gradient is 2^-17 of the full-size one -- scaled back by
    the same power of two (exact) and held to the same budget; the normwise error is scale-free."""
    dim, h_sizes, rows = WIDE
    z, w_y, w_l = inputs(dim, rows)
    layer = make(amd, dim, h_sizes, True)
    got = backward(layer, z, w_y * 2.0 ** -17, w_l * 2.0 ** -17)
    got = {k: v * 2.0 ** 17 for k, v in got.items()}
    oracle(dim, h_sizes, rows, True).check_all(got, f"maf_seq_bwd_rt cotangents x 2^-17 d={dim} h={h_sizes}")


# ---------------------------------------------------------------------------------------------------------------------
# 5. rows do not see each other; unaligned rows
# ---------------------------------------------------------------------------------------------------------------------
def test_rows_do_not_see_each_other(amd):
    """grad_x of the first 129 of 257 rows = that of a 129-row call (a ragged last tile whose dead lanes read the clamped
    last row), bit for bit."""
    dim, h_sizes, rows = ODD
    z, w_y, w_l = inputs(dim, rows)
    layer = make(amd, dim, h_sizes, True)
    full = backward(layer, z, w_y, w_l)["x"]
    head = backward(layer, z[:129].contiguous(), w_y[:129].contiguous(), w_l[:129].contiguous())["x"]
    assert torch.equal(head.view(torch.int32), full[:129].view(torch.int32))


def test_rows_at_a_four_byte_odd_offset(amd):
    """y, grad_y and grad_x starting 4 bytes past a 16-byte boundary (element-by-element row accesses where the aligned call
    uses 16-byte ones, dim % 4 == 0): the aligned call's grad_x bit for bit, nothing written in front of the first row."""
    dim, h_sizes, rows = 40, (64,), 129
    z, w_y, w_l = inputs(dim, rows)
    layer = make(amd, dim, h_sizes, True)
    with torch.no_grad():
        y, _ = layer.forward(z.to(DEV))
    gy, gl = w_y.to(DEV), w_l.to(DEV)
    gx, gf = raw_call(layer, y, gy, gl)

    def odd(t=None):
        buf = torch.zeros(rows * dim + 1, device=DEV)
        view = buf[1:].view(rows, dim)
        if t is not None:
            view.copy_(t)
        assert view.data_ptr() % 16 == 4
        return buf, view

    (_, y_odd), (_, gy_odd), (gx_buf, gx_odd) = odd(y), odd(gy), odd()
    gx2, gf2 = raw_call(layer, y_odd, gy_odd, gl, gx=gx_odd)
    assert torch.equal(gx2.view(torch.int32), gx.view(torch.int32))
    assert float(gx_buf[0]) == 0.0
    oracle(dim, h_sizes, rows, True).check_all({"x": gx2, **flat_grads(layer, gf2)}, "maf_seq_bwd_rt rows at an odd offset")


# ---------------------------------------------------------------------------------------------------------------------
# 6. masked-out weights
# ---------------------------------------------------------------------------------------------------------------------
def test_masked_out_weights_take_no_part(amd):
    """NaN and inf parked in every masked-out weight: staged by a select, left out of the staging exponent, no add.  Through
    the fixed-order entry every gradient is bit for bit that of the run with zeros parked (the atomic entry's parameter sums
    over several workgroups differ in their last bits run to run with ANY weights, so only its grad_x can be held to bits;
    its parameter gradients are held to the oracle); those entries' own gradients are exactly 0.0 on both."""
    dim, h_sizes, rows = ODD
    z, w_y, w_l = inputs(dim, rows)
    clean = make(amd, dim, h_sizes, False)
    atomic, fixed = [], []
    for fill in (0.0, float("nan"), float("inf")):
        layer = make(amd, dim, h_sizes, False, sd={k: v.detach().cpu() for k, v in clean.state_dict().items()})
        with torch.no_grad():
            for m in layer._masked():
                assert int((m.mask.T == 0).sum()) > 0
                m.weight.masked_fill_(m.mask.T == 0, fill)
        atomic.append(backward(layer, z, w_y, w_l))
        with torch.no_grad():
            y, _ = layer.forward(z.to(DEV))
        gx, gf = raw_call(layer, y, w_y.to(DEV), w_l.to(DEV), det=True)
        fixed.append({"x": gx, **flat_grads(layer, gf)})
        for got in (atomic[-1], fixed[-1]):
            assert all(bool(torch.isfinite(v).all()) for v in got.values())
            masked_entries_are_zero(layer, got)
            oracle(dim, h_sizes, rows, False).check_all(got, f"maf_seq_bwd_rt masked-out weights = {fill}")
    for other in fixed[1:]:
        for k, v in other.items():
            assert torch.equal(v.view(torch.int32), fixed[0][k].view(torch.int32)), k
    for other in atomic[1:]:
        assert torch.equal(other["x"].view(torch.int32), atomic[0]["x"].view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------------
# 7. against the parent's route
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,h_sizes,rows", [SHAPES[2], ODD])
def test_against_the_parents_route(amd, monkeypatch, dim, h_sizes, rows):
    """The same call with the constant None runs maf_bwd_generic: the two agree within the sum of the budgets each has
    against the float64 oracle."""
    from torch_mnf_amd import _dispatch

    layer = make(amd, dim, h_sizes, True)
    new = backward(layer, *inputs(dim, rows))
    monkeypatch.setattr(_dispatch, "MAF_SEQ_BWD_RT_MIN_ROWS", None)
    old = backward(layer, *inputs(dim, rows), expect=PARENT)
    ref = oracle(dim, h_sizes, rows, True)
    for k in new:
        r32, r64 = ref.g[torch.float32][k].numpy(), ref.g[torch.float64][k].numpy()
        budget = 2 * (GBASE + 2.0 * normwise_err(r32, r64))
        err = normwise_err(new[k].cpu().numpy(), old[k].cpu().numpy())
        print(f"maf_seq_bwd_rt vs maf_bwd_generic d={dim} {k}: {err:.3e} (budget {budget:.3e})")
        assert err <= budget, (k, err, budget)


# ---------------------------------------------------------------------------------------------------------------------
# 8. fallbacks
# ---------------------------------------------------------------------------------------------------------------------
def test_without_the_constant_the_parents_kernel_runs(amd, monkeypatch):
    from torch_mnf_amd import _dispatch

    monkeypatch.setattr(_dispatch, "MAF_SEQ_BWD_RT_MIN_ROWS", None)
    dim, h_sizes, rows = SHAPES[2]
    got = backward(make(amd, dim, h_sizes, True), *inputs(dim, rows), expect=PARENT)
    oracle(dim, h_sizes, rows, True).check_all(got, "maf_bwd_generic with the route not opted in")


def test_fallback_for_a_shape_without_a_plan(amd):
    dim, h_sizes, rows = 6, (128,), 100
    layer = make(amd, dim, h_sizes, True)
    assert not layer._rt_seq_bwd(rows)
    got = backward(layer, *inputs(dim, rows), expect=PARENT)
    oracle(dim, h_sizes, rows, True).check_all(got, "maf_bwd_generic fallback of maf_seq_bwd_rt")


def test_a_permuted_made_is_still_refused(amd):
    from torch_mnf_amd.flows import MADE

    dim = 6
    torch.manual_seed(4)
    flow = amd.MAF(dim, True, net=MADE(dim, (16, 16), 2 * dim, natural_ordering=False))
    flow.force_generic = 2
    flow.to(DEV)
    assert not flow._autoregressive_in_index_order() and flow._rt_seq_bwd(200)
    with pytest.raises(NotImplementedError, match="natural_ordering"):
        flow.forward((0.5 * recipes.gaussian(31, 200, dim)).to(DEV).requires_grad_(True))


# ---------------------------------------------------------------------------------------------------------------------
# 9. a model
# ---------------------------------------------------------------------------------------------------------------------
def test_three_layer_iaf_model_trains_through_the_route(amd, O):
    """3 IAF layers of alternating parity under StandardNormal, 2,049 rows, -model.log_prob(x).mean().backward(): every
    parameter gradient against autograd through the oracle's maf calls composed here (IAF.inverse is the element-by-element
    pass; log_prob walks the layers backwards); once more with the parameters in a FlatParameters buffer: the same
    gradients, added in place (a second backward pass doubles them)."""
    dim, h_sizes, rows, n = 6, (16, 16), 2049, 3
    sds = [recipes.maf_params(2800 + i, dim, h_sizes, gain=1.2, last_gain=0.5) for i in range(n)]
    masks = O.made_masks(dim, h_sizes, 2 * dim)
    x = recipes.gaussian(2801, rows, dim)
    ref = {}
    for dt in (torch.float32, torch.float64):
        ps = [{k: v.to(dt).clone().requires_grad_(True) for k, v in sd.items()} for sd in sds]
        z, total = x.to(dt), torch.zeros(rows, dtype=dt)
        for i in reversed(range(n)):
            z, ld = O.maf(z, ps[i], masks, i % 2 == 0, False)
            total = total + ld
        lp = -0.5 * (z * z).sum(1) - 0.5 * dim * math.log(2 * math.pi) + total
        (-lp.mean()).backward()
        ref[dt] = {f"flows.{i}.{k}": v.grad for i in range(n) for k, v in ps[i].items()}

    def build():
        flows = [make(amd, dim, h_sizes, i % 2 == 0, cls=amd.IAF, sd=sds[i]) for i in range(n)]
        return amd.NormalizingFlowModel(amd.StandardNormal(dim, DEV), flows).to(DEV)

    model = build()
    (-model.log_prob(x.to(DEV)).mean()).backward()
    assert layer_kernel() == KERNEL
    plain = {k: p.grad.clone() for k, p in model.named_parameters()}
    assert set(plain) == set(ref[torch.float32])
    for k, g in plain.items():
        check_vs_float64(g, ref[torch.float32][k], ref[torch.float64][k], f"3 x IAF -log_prob.mean() grad {k}")

    model = build()
    flat = amd.FlatParameters(model)
    for passes in (1, 2):  # the second pass adds to what the first left in the buffer: twice the gradient (the halving is exact)
        (-model.log_prob(x.to(DEV)).mean()).backward()
        assert layer_kernel() == KERNEL
        for k, p in model.named_parameters():
            assert flat.grad.data_ptr() <= p.grad.data_ptr() < flat.grad.data_ptr() + 4 * flat.grad.numel()
            check_vs_float64(p.grad / passes, ref[torch.float32][k], ref[torch.float64][k],
                             f"3 x IAF in FlatParameters, {passes} pass(es), grad {k}")


# ---------------------------------------------------------------------------------------------------------------------
# 10. fixed order
# ---------------------------------------------------------------------------------------------------------------------
def test_fixed_order_sums_in_a_child_process(amd):
    env = dict(os.environ, MNF_DETERMINISTIC="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "maf_seq_bwd_rt_deterministic_child.py")], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=300)
    tail = "\n".join((p.stdout + p.stderr).splitlines()[-30:])
    assert p.returncode == 0, tail
    assert "maf seq bwd rt deterministic child ok" in p.stdout, tail
