"""AffineHalfFlow gradients for conditioners whose widest hidden layer has 65 .. 128 units on the matrix cores: the second
size class of ahf_bwd_rt (csrc/mnf_ahf_bwd_rt.hip, the mnf_affine_half_bwd_rt_wide* entries), reached through the layer with
_dispatch.AHF_BWD_RT_WIDE_MIN_ROWS set (the route is opt-in: None as shipped).

Against the float64 oracle on the audited budget (test_hip_autograd.OracleGrads: GBASE + twice the fp32 oracle's own
distance from float64), in the form of test_hip_round6.py::test_affine_half_rt_gradients, with that test's recipes and
seeds.  Rows: 300 has a partial tile, 2,100 several row blocks at every wave count the plan can choose (16 .. 128 rows
per block)."""
import os
import subprocess
import sys
import warnings

import pytest
import torch

import recipes
from helpers import assert_close
from test_hip_autograd import GBASE, OracleGrads, cot_loss

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def amd():
    import torch_mnf_amd

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch_mnf_amd


@pytest.fixture(scope="module")
def O():
    from oracle import flow_oracle

    return flow_oracle


@pytest.fixture
def wide_on(monkeypatch):
    """The route opted in from the first row on (a layer's force_generic = 2 then lifts wants_rt's own floor)."""
    from torch_mnf_amd import _dispatch

    monkeypatch.setattr(_dispatch, "AHF_BWD_RT_WIDE_MIN_ROWS", 0)
    return _dispatch


def bits(a):
    return a.contiguous().view(torch.int32)


def same_bits(a, b, what=""):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert torch.equal(bits(a), bits(b)), f"{what}: {int((bits(a) != bits(b)).sum())} of {a.numel()} elements differ"


def layer_of(amd, dim, parity, hs, kw, sd, force=2):
    f = amd.AffineHalfFlow(dim, parity, h_sizes=hs, **kw)
    f.load_state_dict(sd)
    f.force_generic = force
    return f.to(DEV)


def backward(f, x_cpu, inverse, w_y, w_l):
    """-> (gradients {"x", parameter names}, the gradient kernel's family)"""
    import torch_mnf_amd

    x = x_cpu.detach().to(DEV).requires_grad_(True)
    y, ld = f.forward(x, inverse=inverse)
    ((y * w_y.to(DEV)).sum() + (ld * w_l.to(DEV)).sum()).backward()
    torch.cuda.synchronize()
    return {"x": x.grad, **{n: q.grad for n, q in f.named_parameters()}}, torch_mnf_amd.last_kernel()


def inputs(dim, rows):
    """the recipes and seeds of test_hip_round6.py::test_affine_half_rt_gradients (seed 232 + dim: see the remark there)"""
    return recipes.gaussian(232 + dim, rows, dim), recipes.gaussian(33, rows, dim), recipes.gaussian(34, rows, 1)[:, 0]


def params(dim, hs, kw):
    return recipes.affine_half_params(31 + dim, dim, h_sizes=hs, s_last_gain=2.0, **kw)


# each the smallest that reaches a distinct branch of the kernel or its plan
SHAPES = [
    (64, (128,), {}),                  # one layer, full tiles
    (64, (65,), {}),                   # five tiles, 15 padding units
    (10, (100, 72), {}),               # a half narrower than a tile, two wide layers
    (64, (128, 128, 128), {}),         # the shape the route is for
    (64, (128,) * 4, {}),              # 32 exchange tiles: 32 rows per workgroup
    (64, (24, 128), {}),               # mixed widths: the chunk sizes differ per layer
    (64, (128, 24), {}),
    (512, (96,), {}),                  # many first-layer input chunks
    (64, (128,), {"scale": False}),    # one net absent
    (64, (128,), {"shift": False}),
    (6, (128,), {}),                   # rows that are not 16-byte aligned
]


@pytest.mark.parametrize("dim,hs,kw", SHAPES, ids=lambda v: str(v).replace(" ", ""))
@pytest.mark.parametrize("inverse", [False, True])
def test_gradients(amd, O, wide_on, dim, hs, kw, inverse):
    for rows, parity in ((300, True), (2100, False)):
        sd = params(dim, hs, kw)
        x_cpu, w_y, w_l = inputs(dim, rows)
        ref = OracleGrads(cot_loss(lambda x, p: O.affine_half(x, p, parity, inverse, **kw), w_y, w_l), x_cpu, sd)
        got, kernel = backward(layer_of(amd, dim, parity, hs, kw, sd), x_cpu, inverse, w_y, w_l)
        assert kernel == "ahf_bwd_rt", kernel
        ref.check_all(got, f"ahf_bwd_rt wide d={dim} h={hs} {kw} rows={rows} inv={inverse}")


def test_fixed_order_sums_in_a_child_process(amd):
    env = dict(os.environ, MNF_DETERMINISTIC="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ahf_bwd_rt_wide_deterministic_child.py")], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=300)
    tail = "\n".join((p.stdout + p.stderr).splitlines()[-30:])
    assert p.returncode == 0, tail
    assert "ahf bwd rt wide deterministic child ok" in p.stdout, tail


# ------------------------------------------------------------------------------------------------- a run as one node
RUN_DIM, RUN_HS, RUN_LAYERS, RUN_ROWS = 64, (96, 96), 3, 2100


def run_state_dicts():
    return [recipes.affine_half_params(31 + RUN_DIM + i, RUN_DIM, h_sizes=RUN_HS, s_last_gain=2.0) for i in range(RUN_LAYERS)]


def run_model(amd, sds, switch):
    flows = []
    for i, sd in enumerate(sds):
        f = amd.AffineHalfFlow(RUN_DIM, parity=bool(i % 2), h_sizes=RUN_HS)
        f.load_state_dict(sd)
        flows.append(f)
    model = amd.NormalizingFlowModel(amd.StandardNormal(RUN_DIM, DEV), flows).to(DEV)
    model.fuse_rt_training = switch
    return model


def run_step(amd, model, x_cpu, loss, w):
    x = x_cpu.to(DEV).requires_grad_(True)
    if loss == "nll":
        out = model.log_prob(x)
        k_fwd = amd.last_kernel()
        (-out.mean()).backward()
    else:
        zs, ld = model.inverse(x)
        k_fwd = amd.last_kernel()
        ((zs[-1] * w[0].to(DEV)).sum() + (ld * w[1].to(DEV)).sum()).backward()
    torch.cuda.synchronize()
    return k_fwd, amd.last_kernel(), {"x": x.grad, **{k: q.grad for k, q in model.named_parameters()}}


@pytest.mark.parametrize("loss", ["nll", "inverse"])
def test_a_run_trains_as_one_node(amd, O, wide_on, loss):
    """fuse_rt_training on: ahf_stack_rt forward, ONE ahf_bwd_stack_rt launch backward (the wide stack entries); off: the
    layers one by one through the wide route.  x.grad of the two bit for bit; the parameter gradients bit for bit under
    MNF_DETERMINISTIC=1 (fixed-order sums), else 1e-6 normwise (two orders of float atomics) -- what
    tests/test_hip_rt_train_run.py::test_the_route holds for the narrow shapes; test_one_launch_equals_n_launches below
    holds the fixed-order forms bit for bit in either mode.  -log_prob(x).mean() also against the float64 oracle."""
    sds = run_state_dicts()
    x_cpu, w_y, w_l = inputs(RUN_DIM, RUN_ROWS)
    got = {}
    for switch in (True, False):
        k_fwd, k_bwd, got[switch] = run_step(amd, run_model(amd, sds, switch), x_cpu, loss, (w_y, w_l))
        want = ("ahf_stack_rt", "ahf_bwd_stack_rt") if switch else ("ahf_rt", "ahf_bwd_rt")
        assert (k_fwd, k_bwd) == want, (switch, k_fwd, k_bwd)
    same_bits(got[True]["x"], got[False]["x"], "x.grad")
    for k in got[False]:
        if amd.deterministic():
            same_bits(got[True][k], got[False][k], k)
        else:
            assert_close(got[True][k], got[False][k], 1e-6, k)
    if loss == "nll":
        sd_all = {f"flows.{i}.{k}": v for i, sd in enumerate(sds) for k, v in sd.items()}

        def nll(x, p, dt):
            ld = 0
            for i in reversed(range(RUN_LAYERS)):
                x, l1 = O.affine_half(x, {k: p[f"flows.{i}.{k}"] for k in sds[i]}, bool(i % 2), True)
                ld = ld + l1
            return -(ld + O.std_normal_log_prob(x)).mean()

        OracleGrads(nll, x_cpu, sd_all).check_all(got[True], "wide run, -log_prob.mean()")


def test_the_run_stays_layer_by_layer_without_the_constant(amd):
    """As shipped a run of such layers does not train as one node, whatever fuse_rt_training says."""
    sds = run_state_dicts()
    x_cpu, w_y, w_l = inputs(RUN_DIM, RUN_ROWS)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        k_fwd, k_bwd, _ = run_step(amd, run_model(amd, sds, True), x_cpu, "nll", None)
    assert (k_fwd, k_bwd) == ("ahf_rt", "ahf_bwd_generic"), (k_fwd, k_bwd)


@pytest.mark.parametrize("inverse", [False, True])
def test_one_launch_equals_n_launches(amd, inverse):
    """The C ABI: mnf_affine_half_bwd_rt_wide_stack_det on three layers against three calls of
    mnf_affine_half_bwd_rt_wide_det on the same inputs and scales -- grad_x and grad_flats bit for bit (the cotangent
    hand-over between layers: each lane reads the grad_x it stored), the lp form against its materialised cotangent."""
    from torch_mnf_amd import _lib
    from torch_mnf_amd.flows import _grad_scale

    lib = _lib.load()
    n, rows, dim = RUN_LAYERS, RUN_ROWS, RUN_DIM
    hid, flags = (len(RUN_HS), _lib.int_array(list(RUN_HS))), (1, 1)
    parities = [0, 1, 1]
    flats = []
    for sd in run_state_dicts():
        f = amd.AffineHalfFlow(dim, parity=False, h_sizes=RUN_HS)
        f.load_state_dict(sd)
        flats.append(torch.cat([p.detach().reshape(-1) for p in f.parameters()]))
    n_params = flats[0].numel()
    flats = torch.cat(flats).to(DEV).contiguous()
    par = _lib.int_array(parities)
    stream = torch.cuda.current_stream().cuda_stream
    x = recipes.gaussian(600 + dim + rows, rows, dim, scale=0.5).to(DEV)
    outs, ld = torch.empty((n, rows, dim), device=DEV), torch.empty(rows, device=DEV)
    assert lib.mnf_affine_half_rt_stack(x.data_ptr(), outs[-1].data_ptr(), outs.data_ptr(), ld.data_ptr(), None, None, None, 0,
                                        flats.data_ptr(), par, n, rows, dim, int(inverse), *hid, *flags, stream) == _lib.MNF_OK
    g = torch.Generator(device=DEV).manual_seed(700 + rows + dim)
    gy, gl = torch.randn(rows, dim, device=DEV, generator=g) / rows, torch.randn(rows, device=DEV, generator=g) / rows
    a = (rows, dim, *hid, *flags)
    n_run, n_one = lib.mnf_affine_half_bwd_rt_wide_stack_det_workspace(*a, n), lib.mnf_affine_half_bwd_rt_wide_det_workspace(*a)
    assert n_run > 0 and n_one > 0
    ws = torch.empty(max(n_run, n_one), device=DEV)

    def layer_by_layer(gy, gl, sc):
        gf, g_in = torch.zeros_like(flats), gy
        for i in range(n - 1, -1, -1):
            k = n - 1 - i if inverse else i
            gx = torch.full_like(x, float("nan"))
            rc = lib.mnf_affine_half_bwd_rt_wide_det(
                (x if i == 0 else outs[i - 1]).data_ptr(), outs[i].data_ptr(), g_in.data_ptr(), gl.data_ptr(), gx.data_ptr(),
                gf.data_ptr() + 4 * n_params * k, flats.data_ptr() + 4 * n_params * k, sc.data_ptr(), rows, dim, parities[k],
                int(inverse), *hid, *flags, ws.data_ptr(), n_one, stream)
            assert rc == _lib.MNF_OK, rc
            g_in = gx
        return g_in, gf

    def one_launch(gy, lp, gl, sc):
        gx, work, gf = torch.full_like(x, float("nan")), torch.full_like(x, float("nan")), torch.zeros_like(flats)
        ptr = lambda t: None if t is None else t.data_ptr()
        rc = lib.mnf_affine_half_bwd_rt_wide_stack_det(
            x.data_ptr(), outs.data_ptr(), ptr(gy), ptr(lp), ptr(gl), gx.data_ptr(), work.data_ptr(), gf.data_ptr(),
            flats.data_ptr(), sc.expand(n).contiguous().data_ptr(), par, n, rows, dim, int(inverse), *hid, *flags,
            ws.data_ptr(), n_run, stream)
        assert rc == _lib.MNF_OK and amd.last_kernel() == "ahf_bwd_stack_rt", (rc, amd.last_kernel())
        return gx, gf

    sc = _grad_scale(gy, gl, rows, dim, x.device)
    ref_gx, ref_gf = layer_by_layer(gy, gl, sc)
    assert bool(torch.isfinite(ref_gx).all()) and bool(torch.isfinite(ref_gf).all()) and float(ref_gf.abs().max()) > 0
    gx, gf = one_launch(gy, None, gl, sc)
    same_bits(gx, ref_gx, "grad_x")
    same_bits(gf, ref_gf, "grad_flats")
    sc = _grad_scale(None, gl, rows, dim, x.device)
    gx_a, gf_a = one_launch(-outs[n - 1] * gl.unsqueeze(1), None, gl, sc)
    gx_b, gf_b = one_launch(None, gl, None, sc)
    same_bits(gx_b, gx_a, "lp form grad_x")
    same_bits(gf_b, gf_a, "lp form grad_flats")


# ------------------------------------------------------------------------------------------------------------ routes
def test_routes(amd, O, monkeypatch):
    from torch_mnf_amd import _dispatch

    dim, hs = 64, (128,)
    sd = params(dim, hs, {})

    def kernel(rows, force=0, fp32=False):
        f = layer_of(amd, dim, False, hs, {}, sd, force)
        f.force_fp32_mfma = fp32
        x_cpu, w_y, w_l = inputs(dim, rows)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # (the any-shape kernel's note at 4,096 rows)
            return backward(f, x_cpu, True, w_y, w_l)

    assert _dispatch.AHF_BWD_RT_WIDE_MIN_ROWS is None  # as shipped
    assert kernel(4096)[1] == "ahf_bwd_generic" and kernel(4096, force=2)[1] == "ahf_bwd_generic"
    monkeypatch.setattr(_dispatch, "AHF_BWD_RT_WIDE_MIN_ROWS", 2048)
    assert kernel(4096)[1] == "ahf_bwd_rt" and kernel(200)[1] == "ahf_bwd_generic"
    assert kernel(200, force=2)[1] == "ahf_bwd_generic"  # below the constant, whatever lifts wants_rt's floor
    assert kernel(4096, force=1)[1] == "ahf_bwd_generic" and kernel(4096, fp32=True)[1] == "ahf_bwd_generic"
    monkeypatch.undo()
    # the narrow kernel's shapes: the same launch and the same bits, whatever the constant says
    hs = (64, 64, 64)
    sd = params(dim, hs, {})
    x_cpu, w_y, w_l = inputs(dim, 2100)
    got = {}
    for value in (None, 0):
        monkeypatch.setattr(_dispatch, "AHF_BWD_RT_WIDE_MIN_ROWS", value)
        got[value], k = backward(layer_of(amd, dim, False, hs, {}, sd), x_cpu, True, w_y, w_l)
        assert k == "ahf_bwd_rt", k
    same_bits(got[0]["x"], got[None]["x"], "narrow shape x.grad")
    for k in got[None]:
        if amd.deterministic():
            same_bits(got[0][k], got[None][k], k)
        else:  # (two runs of the same atomic sums)
            assert_close(got[0][k], got[None][k], 1e-6, k)


# ------------------------------------------------------------------------------------------------------------- range
def scaled(sd, factors):
    return {k: (v * factors[k] if k in factors else v) for k, v in sd.items()}


@pytest.mark.parametrize("family", ["weights_2^-12", "weights_2^6", "cot_mean"])
@pytest.mark.parametrize("inverse", [False, True])
def test_range(amd, O, wide_on, family, inverse):
    """Outside the unit-scale fixtures, at (64, (128,)) and 2,100 rows, on the budget of tests/rt_bwd_range_cases.py's cot_*
    and weight families (GBASE + widening: no stress allowance).

    weights_2^-12: every weight matrix x 2^-12 -- the staged weights' common exponent (weight_exponent) far below 1, both
    nets' outputs ~1e-4.  weights_2^6: the first Linear (weights and bias) x 2^6 and the output Linear's weights x 2^-6 --
    LeakyReLU is homogeneous, so s and t are what they were (all weights x 2^6 would put s at 2^12 times its value and
    e^s beyond fp32), while the kernel stages first-layer weights up to ~8 beside output weights of ~1e-3 under ONE common
    exponent and carries a hidden vector of ~64.  cot_mean: cotangents x 1 / rows, the mean loss of a training step."""
    dim, hs, rows = 64, (128,), 2100
    sd = params(dim, hs, {})
    x_cpu, w_y, w_l = inputs(dim, rows)
    nets = ("s_net", "t_net")
    if family == "weights_2^-12":
        sd = scaled(sd, {k: 2.0 ** -12 for k in sd if k.endswith(".weight")})
    elif family == "weights_2^6":
        sd = scaled(sd, {**{f"{n}.0.{p}": 2.0 ** 6 for n in nets for p in ("weight", "bias")},
                         **{f"{n}.2.weight": 2.0 ** -6 for n in nets}})
    else:
        w_y, w_l = w_y / rows, w_l / rows
    ref = OracleGrads(cot_loss(lambda x, p: O.affine_half(x, p, False, inverse), w_y, w_l), x_cpu, sd)
    got, kernel = backward(layer_of(amd, dim, False, hs, {}, sd), x_cpu, inverse, w_y, w_l)
    assert kernel == "ahf_bwd_rt", kernel
    ref.check_all(got, f"ahf_bwd_rt wide range {family} inv={inverse}", base=GBASE)


# --------------------------------------------------------------------------------------------------------- dead rows
@pytest.mark.parametrize("inverse", [False, True])
def test_dead_rows(amd, O, wide_on, inverse):
    """17 rows: one live row in the second tile, 15 rows past the end beside it (they read the last row's addresses and
    are kept out of every sum and every store).  grad_x holds exactly the live rows' values: bit for bit the first 17 rows
    of a 32-row batch whose other rows repeat row 16 with zero cotangents (the same gradient scale, a full tile); the
    parameter gradients are finite and within the budget."""
    dim, hs, rows = 64, (128,), 17
    sd = params(dim, hs, {})
    x_cpu, w_y, w_l = inputs(dim, rows)
    ref = OracleGrads(cot_loss(lambda x, p: O.affine_half(x, p, True, inverse), w_y, w_l), x_cpu, sd)
    got, kernel = backward(layer_of(amd, dim, True, hs, {}, sd), x_cpu, inverse, w_y, w_l)
    assert kernel == "ahf_bwd_rt", kernel
    assert got["x"].shape == (rows, dim) and all(bool(torch.isfinite(v).all()) for v in got.values())
    ref.check_all(got, f"ahf_bwd_rt wide 17 rows inv={inverse}")
    pad = 32 - rows
    x_full = torch.cat([x_cpu, x_cpu[-1:].expand(pad, dim)])
    wy_full, wl_full = torch.cat([w_y, torch.zeros(pad, dim)]), torch.cat([w_l, torch.zeros(pad)])
    full, kernel = backward(layer_of(amd, dim, True, hs, {}, sd), x_full, inverse, wy_full, wl_full)
    assert kernel == "ahf_bwd_rt", kernel
    same_bits(got["x"], full["x"][:rows].contiguous(), "grad_x of the live rows")
