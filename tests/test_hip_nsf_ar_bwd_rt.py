"""GPU tests of the gradients of NSF_AR's one-pass direction on the matrix cores (``mnf_nsf_ar_bwd_rt`` behind
``_NsfArFn.backward`` for ``NSF_AR.inverse``, kernel family ``nsf_ar_bwd_rt``): the reference's own autograd gradients
(fixture G18), one shape per path of the kernel against autograd through the float64 oracle, the cotangent conventions and
magnitudes, the autoregressive structure (exact), inputs on and outside the spline's interval, the routes, a three-layer
model under ``-log_prob.mean()`` and the fixed-order form in a child process.

Every case runs ``force_generic = 2`` with ``NSF_AR_BWD_RT_MIN_ROWS = 0`` and names the kernel it ran (``last_kernel()``).
Tolerance: the project's own rule, ``OracleGrads.check_all`` / ``check_vs_float64`` (1e-5 normwise plus twice the fp32
gradients' distance from the float64 ones), ``GTOL`` kernel against kernel; recorded for tests/test_zz_audit.py."""
import functools
import math
import os
import subprocess
import sys

import pytest
import torch

import g18_cases as G18
import recipes
from helpers import budgeted, normwise_err
from test_hip_autograd import GTOL, OracleGrads, check_vs_float64, cot_loss

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL, FORWARD, PARENT = "nsf_ar_bwd_rt", "nsf_ar_rt", "nsf_ar_bwd_generic"
B = 3.0

# (dim, K, n_h, rows): one group, element 0 plus one net, a ragged tile | . | odd width, rows not 16-byte aligned | the
# narrowest width, a last group of one element | two K-steps of input, dim % 4 = 1 | three K-steps, the widest class | more
# row blocks than workgroups
SHAPES = [(2, 8, 16, 17), (3, 5, 8, 130), (6, 5, 5, 257), (13, 8, 4, 145), (37, 5, 8, 145), (70, 8, 16, 33), (6, 8, 8, 70003)]
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


@pytest.fixture(autouse=True)
def _route_opted_in(monkeypatch):
    from torch_mnf_amd import _dispatch

    assert _dispatch.NSF_AR_BWD_RT_MIN_ROWS is None  # shipped: opt-in
    monkeypatch.setattr(_dispatch, "NSF_AR_BWD_RT_MIN_ROWS", 0)


def params(dim, K, n_h):
    return recipes.nsf_ar_params(4100 + dim + K, dim, K, n_h)


def make(amd, dim, K, n_h, sd=None, force=2, net_class=None):
    layer = amd.NSF_AR(dim, K=K, B=3, n_h=n_h) if net_class is None else amd.NSF_AR(dim, K=K, B=3, n_h=n_h, net_class=net_class)
    if sd is not None:
        layer.load_state_dict(sd)
    layer.force_generic = force
    return layer.to(DEV)


def layer_kernel():
    import torch_mnf_amd

    torch.cuda.synchronize()
    return torch_mnf_amd.last_kernel()


def layer_grads(layer, x, w, v, kernel=KERNEL, forward=FORWARD):
    """{"x": ..., name: ...} of sum(z * w) + sum(log_det * v) through layer.inverse (w or v None: that cotangent is zero)"""
    layer.zero_grad()
    xg = x.clone().to(DEV).requires_grad_(True)
    z, ld = layer.inverse(xg)
    assert layer_kernel() == forward
    loss = 0.0
    if w is not None:
        loss = loss + (w.to(DEV) * z).sum()
    if v is not None:
        loss = loss + (v.to(DEV) * ld).sum()
    loss.backward()
    assert layer_kernel() == kernel
    return {"x": xg.grad, **{name: prm.grad for name, prm in layer.named_parameters()}}


def raw_call(layer, x, gy, gl, want_flat=True):
    """mnf_nsf_ar_bwd_rt at the C ABI: (grad_x, grad_flat); grad_x starts as NaN, grad_flat as zeros"""
    from torch_mnf_amd import _lib

    lib, rows, dim = _lib.load(), x.shape[0], x.shape[1]
    flat = torch.cat([p.detach().reshape(-1) for p in layer._packed_params()]).contiguous()
    gx = torch.full((rows, dim), float("nan"), device=DEV)
    gf = torch.zeros_like(flat) if want_flat else None
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    args = (x.data_ptr(), ptr(gy), ptr(gl), gx.data_ptr(), ptr(gf), flat.data_ptr(), rows, dim, layer.K, float(layer.B),
            len(layer.h_sizes), layer._hid)
    rc = lib.mnf_nsf_ar_bwd_rt(*args, None)
    assert rc == 0, rc
    assert layer_kernel() == KERNEL
    return gx, gf


def oracle_loss(O, K, w, v):
    return cot_loss(lambda xx, p: O.nsf_ar(xx, p, K, B, True), w, v)


def kink_rows(x, sd):
    """Rows in which the gradient is not determined at fp32 accuracy: some hidden unit's pre-activation p = b + sum_k w_k h_k
    (float64) lies within 2^-20 (|b| + sum_k |w_k h_k|) of zero.  LeakyReLU's slope jumps there (1 against 0.2), and the sign of
    such a p is below what ANY fp32 evaluation resolves: the fp32 oracle's own sum carries n 2^-24 of the terms, the split-f16
    products 2^-22 (csrc/mnf_split.h) -- 2^-20 leaves a factor of four.  (Measured on the 70,003-row case as first drawn: one
    row with p = 1.03e-7 next to terms of 3.1, i.e. 2^-25 of them; the kernel took the other slope than the fp32 oracle, which
    moved that row's grad_x by the size of the jump, 1.2e-3 of the tensor's maximum, and nothing else.)"""
    from oracle import flow_oracle as O

    bad = torch.zeros(x.shape[0], dtype=torch.bool)
    for i in range(1, x.shape[1]):
        h = x[:, :i].double()
        for l in O.linear_indices(sd, f"layers.{i - 1}")[:-1]:
            W, b = sd[f"layers.{i - 1}.{l}.weight"].double(), sd[f"layers.{i - 1}.{l}.bias"].double()
            pre, size = h @ W.T + b, h.abs() @ W.abs().T + b.abs()
            bad |= (pre.abs() < 2.0 ** -20 * size).any(1)
            h = torch.nn.functional.leaky_relu(pre, 0.2)
    return bad


def well_posed(x, sd):
    """x with every kink row redrawn (scaled by 15/16 until no unit sits on its kink): no row of the small cases, 8
    rows of the 70,003-row one"""
    x = x.clone()
    for _ in range(8):
        bad = kink_rows(x, sd)
        if not bool(bad.any()):
            return x
        x[bad] = x[bad] * 0.9375
    raise AssertionError("kink rows left")


@functools.lru_cache(maxsize=None)
def shape_case(dim, K, n_h, rows):
    """(sd, x, w, v, OracleGrads) of a shape-matrix case: computed once, shared, never written"""
    from oracle import flow_oracle as O

    sd = params(dim, K, n_h)
    x = well_posed(recipes.gaussian(4600 + dim, rows, dim, scale=1.4), sd)
    w, v = recipes.gaussian(4700 + dim, rows, dim), recipes.gaussian(4701 + dim, rows, 1)[:, 0]
    return sd, x, w, v, OracleGrads(oracle_loss(O, K, w, v), x, sd)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the reference's own gradients
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", sorted(G18.CASES))
def test_g18_reference_gradients(amd, golden, tag):
    """Fixture G18: the reference's own autograd gradients through NSF_AR.inverse, fp32 and .double(), for x and every
    parameter."""
    fx = golden("g18_nsf_ar_grads")
    dim, K, n_h, rows = G18.CASES[tag]
    sd, x, w, v = G18.inputs(tag)
    g32, g64 = G18.split(tag, fx[f"{tag}.g32"]), G18.split(tag, fx[f"{tag}.g64"])
    got = layer_grads(make(amd, dim, K, n_h, sd=sd), x, w, v)
    assert set(got) == set(g32)
    for k in G18.grad_names(tag):
        check_vs_float64(got[k], torch.from_numpy(g32[k]), torch.from_numpy(g64[k]), f"nsf_ar_bwd_rt G18 {tag} grad {k}")


# ---------------------------------------------------------------------------------------------------------------------
# 2. shapes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,K,n_h,rows", SHAPES)
def test_shapes_vs_oracle(amd, dim, K, n_h, rows):
    sd, x, w, v, og = shape_case(dim, K, n_h, rows)
    got = layer_grads(make(amd, dim, K, n_h, sd=sd), x, w, v)
    og.check_all(got, f"nsf_ar_bwd_rt d={dim} K={K} n_h={n_h} rows={rows}")
    if (dim, K, n_h, rows) == MANY_BLOCKS:  # the persistent grid is smaller than the row blocks: workgroups loop
        from torch_mnf_amd import _lib

        hid = _lib.int_array((n_h,) * 3)
        n_params = _lib.load().mnf_nsf_ar_flat_floats(dim, K, 3, hid)
        slots, rest = divmod(_lib.load().mnf_nsf_ar_bwd_rt_det_workspace(rows, dim, K, 3, hid), (n_params + 63) // 64 * 64)
        assert rest == 0 and 0 < slots and 2 * slots <= (rows + 127) // 128, slots  # (a row block is at most 8 waves x 16 rows)


@pytest.mark.parametrize("K,widths", [(5, (4, 16, 9)), (8, (8,)), (5, (5, 12)), (8, (4, 6, 8, 16))])
def test_unequal_widths_and_layer_counts_vs_the_parent_kernel(amd, monkeypatch, K, widths):
    """Nets of 1, 2, 3 and 4 hidden layers of unequal widths (through net_class): the route against the parent kernel on the
    same layer, kernel against kernel."""
    from torch_mnf_amd import _dispatch

    dim, rows = 7, 150
    layer = make(amd, dim, K, 8, net_class=lambda i, a, b, c, out: amd.MLP(i, *widths, out))
    assert layer.h_sizes == widths
    x = recipes.gaussian(4800 + len(widths), rows, dim, scale=1.4)
    w, v = recipes.gaussian(4801, rows, dim), recipes.gaussian(4802, rows, 1)[:, 0]
    got = {k: g.clone() for k, g in layer_grads(layer, x, w, v).items()}
    monkeypatch.setattr(_dispatch, "NSF_AR_BWD_RT_MIN_ROWS", None)
    ref = layer_grads(layer, x, w, v, kernel=PARENT)
    for k in ref:
        assert float(ref[k].abs().max()) > 0, k
        budgeted(normwise_err(got[k].cpu().numpy(), ref[k].cpu().numpy()), GTOL, f"nsf_ar_bwd_rt vs parent K={K} hidden={widths} grad {k}")


# ---------------------------------------------------------------------------------------------------------------------
# 3. cotangents
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["grad_y", "grad_ld"])
def test_one_cotangent_alone(amd, O, which):
    dim, K, n_h, rows = 6, 5, 8, 130
    sd = params(dim, K, n_h)
    x = recipes.gaussian(4900, rows, dim, scale=1.4)
    w = recipes.gaussian(4901, rows, dim) if which == "grad_y" else None
    v = recipes.gaussian(4902, rows, 1)[:, 0] if which == "grad_ld" else None
    zero_w, zero_v = torch.zeros(rows, dim), torch.zeros(rows)
    og = OracleGrads(oracle_loss(O, K, w if w is not None else zero_w, v if v is not None else zero_v), x, sd)
    og.check_all(layer_grads(make(amd, dim, K, n_h, sd=sd), x, w, v), f"nsf_ar_bwd_rt {which} alone")
    # the same at the C ABI with the other pointer NULL
    layer = make(amd, dim, K, n_h, sd=sd)
    gx, gf = raw_call(layer, x.to(DEV), None if w is None else w.to(DEV), None if v is None else v.to(DEV))
    check_vs_float64(gx, og.ref("x"), og.ref("x", torch.float64), f"nsf_ar_bwd_rt {which} alone, C ABI, grad x")
    assert bool(torch.isfinite(gf).all()) and float(gf.abs().max()) > 0


def test_null_cotangents_and_null_grad_flat(amd):
    dim, K, n_h, rows = 6, 8, 8, 130
    layer = make(amd, dim, K, n_h, sd=params(dim, K, n_h))
    x = recipes.gaussian(4910, rows, dim, scale=1.4).to(DEV)
    gx, gf = raw_call(layer, x, None, None)
    assert float(gx.abs().max()) == 0.0 and float(gf.abs().max()) == 0.0  # (NaN-filled before the call: every entry written)
    gy, gl = recipes.gaussian(4911, rows, dim).to(DEV), recipes.gaussian(4912, rows, 1)[:, 0].contiguous().to(DEV)
    gx_full, gf_full = raw_call(layer, x, gy, gl)
    gx_only, none = raw_call(layer, x, gy, gl, want_flat=False)
    assert none is None and torch.equal(gx_only.view(torch.int32), gx_full.view(torch.int32))
    assert float(gf_full.abs().max()) > 0
    gf_twice = gf_full.clone()  # grad_flat is ADDED to
    from torch_mnf_amd import _lib

    flat = torch.cat([p.detach().reshape(-1) for p in layer._packed_params()]).contiguous()
    gx2 = torch.empty_like(x)
    rc = _lib.load().mnf_nsf_ar_bwd_rt(x.data_ptr(), gy.data_ptr(), gl.data_ptr(), gx2.data_ptr(), gf_twice.data_ptr(),
                                       flat.data_ptr(), rows, dim, K, B, 3, layer._hid, None)
    assert rc == 0 and layer_kernel() == KERNEL
    budgeted(normwise_err(gf_twice.cpu().numpy(), (2 * gf_full).cpu().numpy()), GTOL, "nsf_ar_bwd_rt adds to grad_flat")


@pytest.mark.parametrize("log2_scale", [-20, 10])
def test_cotangent_magnitudes(amd, O, log2_scale):
    """Cotangents of a mean() loss over 10^6 rows (2^-20) and of a summed, weighted one (2^10): the launch's cotangent scale
    keeps them in the split-f16 range -- the same relative accuracy as at magnitude 1."""
    dim, K, n_h, rows = 13, 8, 4, 145
    sd, x, w, v, _ = shape_case(dim, K, n_h, rows)
    s = 2.0 ** log2_scale
    og = OracleGrads(oracle_loss(O, K, w * s, v * s), x, sd)
    og.check_all(layer_grads(make(amd, dim, K, n_h, sd=sd), x, w * s, v * s), f"nsf_ar_bwd_rt cotangents x 2^{log2_scale}")


# ---------------------------------------------------------------------------------------------------------------------
# 4. structure, exact
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [0, 1, 4, 6, 8])
def test_a_cotangent_on_one_column_reaches_its_own_net_only(amd, i):
    """w one-hot in column i, v = 0: grad_x[:, j > i] is exactly 0 and every net but element i's (init_param for i = 0) gets
    an exactly zero gradient -- an off-diagonal product is dropped, not added as a computed 0."""
    dim, K, n_h, rows = 9, 8, 6, 97
    layer = make(amd, dim, K, n_h, sd=params(dim, K, n_h))
    x = recipes.gaussian(4920, rows, dim, scale=1.2)
    w = torch.zeros(rows, dim)
    w[:, i] = recipes.gaussian(4921, rows, 1)[:, 0]
    got = layer_grads(layer, x, w, None)
    assert float(got["x"][:, i + 1:].abs().max() if i + 1 < dim else 0.0) == 0.0
    assert float(got["x"][:, :i + 1].abs().max()) > 0
    own = "init_param" if i == 0 else f"layers.{i - 1}."
    for name, g in got.items():
        if name == "x":
            continue
        if name.startswith(own):
            assert float(g.abs().max()) > 0, name
        else:
            assert float(g.abs().max()) == 0.0, name


@pytest.mark.parametrize("dim,K,n_h,rows", [(6, 5, 5, 257), (37, 5, 8, 145)])
def test_rows_do_not_see_each_other(amd, dim, K, n_h, rows):
    """A row alone, at the end of a ragged tile (a 130-row prefix) and in the full batch: bit-equal grad_x rows."""
    sd, x, w, v, _ = shape_case(dim, K, n_h, rows)
    layer = make(amd, dim, K, n_h, sd=sd)
    full = layer_grads(layer, x, w, v)["x"].clone()
    head = layer_grads(layer, x[:130], w[:130], v[:130])["x"]
    assert torch.equal(head.view(torch.int32), full[:130].view(torch.int32))
    for r in (0, 129, rows - 1):
        one = layer_grads(layer, x[r:r + 1], w[r:r + 1], v[r:r + 1])["x"]
        assert torch.equal(one.view(torch.int32), full[r:r + 1].view(torch.int32)), r


# ---------------------------------------------------------------------------------------------------------------------
# 5. inputs on the interval's ends and outside it
# ---------------------------------------------------------------------------------------------------------------------
def test_inputs_at_the_tail_bound_and_outside(amd, O):
    """Elements at exactly +-B and outside [-B, B]: the spline is the identity there -- the direct term is the output
    cotangent itself, and those elements send nothing to their nets."""
    dim, K, n_h, rows = 6, 5, 8, 130
    sd = params(dim, K, n_h)
    x = recipes.gaussian(4930, rows, dim, scale=1.4).clone()
    for i, col in enumerate((0, 3, dim - 1)):
        x[4 * i + 0, col] = B
        x[4 * i + 1, col] = -B
        x[4 * i + 2, col] = 7.5
        x[4 * i + 3, col] = -4.25
    x[12] = torch.tensor([3.5, -3.0, 3.0, -6.0, 0.1, 9.0])
    x[129, dim - 1] = 5.0  # in the ragged last tile
    w, v = recipes.gaussian(4931, rows, dim), recipes.gaussian(4932, rows, 1)[:, 0]
    og = OracleGrads(oracle_loss(O, K, w, v), x, sd)
    layer = make(amd, dim, K, n_h, sd=sd)
    og.check_all(layer_grads(layer, x, w, v), "nsf_ar_bwd_rt edge inputs")
    # every element of the LAST column outside: g_v = g_out bit for bit (nothing is added to the last column), and the last
    # net's gradient is exactly zero
    x_out = recipes.gaussian(4933, rows, dim, scale=1.2).clone()
    x_out[:, dim - 1] = torch.where(torch.arange(rows) % 2 == 0, torch.tensor(3.25), torch.tensor(-7.0))
    got = layer_grads(layer, x_out, w, v)
    assert torch.equal(got["x"][:, dim - 1].cpu(), w[:, dim - 1])
    for name, g in got.items():
        if name.startswith(f"layers.{dim - 2}."):
            assert float(g.abs().max()) == 0.0, name


# ---------------------------------------------------------------------------------------------------------------------
# 6. routes
# ---------------------------------------------------------------------------------------------------------------------
def test_the_shipped_route_is_opt_in_and_switches_at_the_threshold(amd, monkeypatch):
    from torch_mnf_amd import _dispatch

    dim, K, n_h = 6, 8, 8
    x = recipes.gaussian(4940, 4099, dim, scale=1.4)
    w, v = recipes.gaussian(4941, 4099, dim), recipes.gaussian(4942, 4099, 1)[:, 0]
    layer = make(amd, dim, K, n_h, sd=params(dim, K, n_h))
    monkeypatch.setattr(_dispatch, "NSF_AR_BWD_RT_MIN_ROWS", None)  # shipped: the parent, force_generic = 2 included
    layer_grads(layer, x, w, v, kernel=PARENT)
    layer.force_generic = 0
    monkeypatch.setattr(_dispatch, "NSF_AR_BWD_RT_MIN_ROWS", 2048)
    layer_grads(layer, x, w, v, forward="nsf_ar_generic")
    layer_grads(layer, x[:2047], w[:2047], v[:2047], kernel=PARENT, forward="nsf_ar_generic")
    layer_grads(layer, x[:2048], w[:2048], v[:2048], forward="nsf_ar_generic")
    layer.force_generic = 1
    layer_grads(layer, x, w, v, kernel=PARENT, forward="nsf_ar_generic")
    layer.force_generic = 2
    # the sequential direction's gradients stay on the parent
    layer.zero_grad()
    zg = x[:130].clone().to(DEV).requires_grad_(True)
    y, ld = layer.forward(zg)
    ((w[:130].to(DEV) * y).sum() + (v[:130].to(DEV) * ld).sum()).backward()
    assert layer_kernel() == PARENT


@pytest.mark.parametrize("dim,K,n_h", [(6, 10, 8), (6, 5, 20)])
def test_fallback_for_a_shape_without_a_plan(amd, O, dim, K, n_h):
    """A K without an instantiation and nets wider than 16 units fall back to the parent kernel under force_generic = 2."""
    rows = 100
    sd = params(dim, K, n_h)
    x = recipes.gaussian(4950 + K, rows, dim, scale=1.4)
    w, v = recipes.gaussian(4951, rows, dim), recipes.gaussian(4952, rows, 1)[:, 0]
    forward = FORWARD if n_h <= 16 else "nsf_ar_generic"
    got = layer_grads(make(amd, dim, K, n_h, sd=sd), x, w, v, kernel=PARENT, forward=forward)
    OracleGrads(oracle_loss(O, K, w, v), x, sd).check_all(got, f"parent fallback of nsf_ar_bwd_rt d={dim} K={K} n_h={n_h}")


# ---------------------------------------------------------------------------------------------------------------------
# 7. a model
# ---------------------------------------------------------------------------------------------------------------------
def test_three_layer_model_under_the_mean_log_prob(amd, O):
    """NormalizingFlowModel of three NSF_AR layers under -log_prob.mean(): forward on nsf_ar_rt, backward on nsf_ar_bwd_rt,
    against autograd through the oracle's stack (cotangents of 1 / 333 and of the layers behind)."""
    dim, K, n_h, rows = 12, 8, 4, 333
    sds = [recipes.nsf_ar_params(4960 + i, dim, K, n_h) for i in range(3)]
    x = recipes.gaussian(4963, rows, dim, scale=1.2)
    ref = {}
    for dt in (torch.float32, torch.float64):
        ps = [{k: t.to(dt).clone().requires_grad_(True) for k, t in sd.items()} for sd in sds]
        z, total = x.to(dt), torch.zeros(rows, dtype=dt)
        for i in reversed(range(3)):  # (log_prob walks the layers backwards)
            z, ld = O.nsf_ar(z, ps[i], K, B, True)
            total = total + ld
        lp = -0.5 * (z * z).sum(1) - 0.5 * dim * math.log(2 * math.pi) + total
        (-lp.mean()).backward()
        ref[dt] = {f"flows.{i}.{k}": t.grad for i in range(3) for k, t in ps[i].items()}
    model = amd.NormalizingFlowModel(amd.StandardNormal(dim, DEV), [make(amd, dim, K, n_h, sd=sd) for sd in sds]).to(DEV)
    (-model.log_prob(x.to(DEV)).mean()).backward()
    assert layer_kernel() == KERNEL
    got = {k: p.grad for k, p in model.named_parameters()}
    assert set(got) == set(ref[torch.float32])
    for k, g in got.items():
        check_vs_float64(g, ref[torch.float32][k], ref[torch.float64][k], f"3 x NSF_AR -log_prob.mean() grad {k}")


# ---------------------------------------------------------------------------------------------------------------------
# 8. fixed order
# ---------------------------------------------------------------------------------------------------------------------
def test_fixed_order_sums_in_a_child_process(amd):
    env = dict(os.environ, MNF_DETERMINISTIC="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "nsf_ar_bwd_rt_deterministic_child.py")], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=300)
    tail = "\n".join((p.stdout + p.stderr).splitlines()[-30:])
    assert p.returncode == 0, tail
    assert "nsf ar bwd rt deterministic child ok" in p.stdout, tail
