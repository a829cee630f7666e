"""Glow's row transform x @ W and its gradients on the run-time-shaped fp32 matrix-core kernels (kernel families
"linear_rows_rt" and "linear_rows_bwd_weight_rt", csrc/mnf_linear_mfma.hip), any 2 <= dim <= 1024.

Every output element of linear_rows_rt is ONE accumulator over k = 0 .. dim-1 in ascending order, and the fp32 MFMA is a
k-ordered fmaf chain, so forward, inverse and grad_x are compared with the VALU kernel's (``force_generic = 1``) WITHOUT a
tolerance -- by value, so that -0 equals +0: a zero-padded k-step turns an accumulator of -0 into +0.  The weight
gradient sums rows four at a time in a fixed order: it is held to the float64 oracle by OracleGrads' own rule, and two
runs must give the same bits."""
import os
import subprocess
import sys

import pytest
import torch

import recipes
from helpers import assert_parity
from test_hip_autograd import OracleGrads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"


@pytest.fixture(scope="module")
def amd():
    import torch_mnf_amd

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch_mnf_amd


@pytest.fixture(scope="module")
def O():
    from oracle import flow_oracle

    return flow_oracle


def glow(amd, dim, force, seed=None):
    gp = recipes.glow_params(900 + dim if seed is None else seed, dim)
    f = amd.Glow(dim)
    f.P = gp["P"]
    f.load_state_dict({k: gp[k] for k in "LSU"})
    f.force_generic = force
    return f.to(DEV), gp


# (dim, rows): fewer rows than a tile and partial row tiles; rows that are not 16-byte aligned and more row blocks than a
# persistent grid has workgroups; a partial column tile; dim % 4 != 0 (scalar stores); a per-shape dim, forced; several
# column groups; several K-chunks with streamed staging; the envelope's edge
FWD_CASES = [(2, 1), (2, 15), (2, 17), (6, 40003), (17, 100), (50, 4099), (64, 4099), (100, 2049), (300, 777), (520, 130),
             (1024, 33)]


def both_routes(amd, dim, x):
    """{inverse: (y on the rt kernel, y on the VALU kernel)} for one layer and input, kernel names checked"""
    f_rt, _ = glow(amd, dim, 2)
    f_valu, _ = glow(amd, dim, 1)
    out = {}
    with torch.no_grad():
        for inverse in (False, True):
            y_rt, ld_rt = (f_rt.inverse if inverse else f_rt.forward)(x)
            assert amd.last_kernel() == "linear_rows_rt", amd.last_kernel()
            y_valu, ld_valu = (f_valu.inverse if inverse else f_valu.forward)(x)
            assert amd.last_kernel() == "linear_rows_generic", amd.last_kernel()
            assert torch.equal(ld_rt, ld_valu)
            out[inverse] = (y_rt, y_valu)
    return out


@pytest.mark.parametrize("dim,rows", FWD_CASES, ids=lambda v: str(v))
def test_forward_and_inverse_equal_the_valu_kernel(amd, dim, rows):
    x = recipes.gaussian(910 + dim, rows, dim, scale=1.2).to(DEV)
    for inverse, (y_rt, y_valu) in both_routes(amd, dim, x).items():
        assert y_rt.shape == y_valu.shape == x.shape
        assert bool(torch.isfinite(y_valu).all())
        differ = int((y_rt != y_valu).sum())
        assert torch.equal(y_rt, y_valu), f"d={dim} rows={rows} inv={inverse}: {differ} of {y_rt.numel()} elements differ"


@pytest.mark.parametrize("dim,rows", [(48, 1031), (100, 517)], ids=lambda v: str(v))
def test_a_view_at_an_odd_storage_offset(amd, dim, rows):
    """dim % 4 == 0 but the rows start 4 bytes past a 16-byte boundary: the 16-byte stores must turn off"""
    buf = torch.zeros(rows * dim + 1, device=DEV)
    buf[1:] = recipes.gaussian(911 + dim, rows, dim).to(DEV).reshape(-1)
    x = buf[1:].view(rows, dim)
    assert x.data_ptr() % 16 == 4 and x.is_contiguous()
    for inverse, (y_rt, y_valu) in both_routes(amd, dim, x).items():
        assert torch.equal(y_rt, y_valu), (dim, rows, inverse)


@pytest.fixture
def rt_at(monkeypatch):
    """rt_at(rows): default dispatch with the row threshold out of the way for a case below it (the threshold is a
    measured latency trade, tests/test_glow_rt_host.py holds tier() to it; the kernels are correct at any row count)"""
    from torch_mnf_amd import _dispatch

    def patch(rows):
        if rows < _dispatch.GLOW_RT_MIN_ROWS:
            monkeypatch.setattr(_dispatch, "GLOW_RT_MIN_ROWS", 0)
    return patch


def backward(f, x_cpu, w_y, inverse, rows):
    x = x_cpu.to(DEV).requires_grad_(True)
    f.zero_grad()
    y, ld = (f.inverse if inverse else f.forward)(x)
    ((y * w_y.to(DEV)).sum() + ld.sum() * rows).backward()
    torch.cuda.synchronize()
    return {"x": x.grad, **{k: getattr(f, k).grad for k in "LSU"}}


@pytest.mark.parametrize("dim,rows", [(6, 3001), (50, 1027), (100, 517), (520, 130)], ids=lambda v: str(v))
@pytest.mark.parametrize("inverse", [False, True])
def test_grad_x_equals_the_valu_route(amd, dim, rows, inverse):
    """grad_x = grad_y @ W^T: the same chain, W read transposed by the kernel (trans = 1) against the VALU kernel on a
    transposed copy"""
    import torch_mnf_amd

    x_cpu, w_y = recipes.gaussian(920 + dim, rows, dim, scale=1.2), recipes.gaussian(921, rows, dim)
    f_rt, _ = glow(amd, dim, 2)
    f_valu, _ = glow(amd, dim, 1)
    g_rt = backward(f_rt, x_cpu, w_y, inverse, rows)
    assert torch_mnf_amd.last_kernel() == "linear_rows_bwd_weight_rt", torch_mnf_amd.last_kernel()
    g_valu = backward(f_valu, x_cpu, w_y, inverse, rows)
    differ = int((g_rt["x"] != g_valu["x"]).sum())
    assert torch.equal(g_rt["x"], g_valu["x"]), f"{differ} of {g_rt['x'].numel()} elements differ"


# (dim, rows, force_generic): default dispatch (rt_at: the row threshold aside), and a dim with a per-shape forward
# kernel forced onto the rt kernels
ORACLE_CASES = [(6, 70001, 0), (50, 30001, 0), (100, 2049, 0), (64, 4099, 2), (300, 2049, 0)]


@pytest.mark.parametrize("dim,rows,force", ORACLE_CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("inverse", [False, True])
def test_gradients_against_the_float64_oracle(amd, O, rt_at, dim, rows, force, inverse):
    rt_at(rows)
    f, gp = glow(amd, dim, force, seed=504 + dim)
    x_cpu = recipes.gaussian(505 + dim, rows, dim, scale=1.2)
    w_y = recipes.gaussian(506, rows, dim)
    got = backward(f, x_cpu, w_y, inverse, rows)
    assert amd.last_kernel() == "linear_rows_bwd_weight_rt", amd.last_kernel()

    def loss_fn(xc, p, dt):
        yc, l2 = O.glow(xc, gp["P"].to(dt), p["L"], p["S"], p["U"], inverse)
        return (yc * w_y.to(dt)).sum() + l2.sum() * rows

    ref = OracleGrads(loss_fn, x_cpu, {k: gp[k] for k in "LSU"})
    ref.check_all(got, f"glow rt d={dim} rows={rows} force={force} inv={inverse}")


@pytest.mark.parametrize("dim,rows", [(6, 70001), (100, 30001), (520, 2049)], ids=lambda v: str(v))
def test_the_weight_gradient_has_the_same_bits_every_run(amd, rt_at, dim, rows):
    rt_at(rows)
    f, _ = glow(amd, dim, 0)
    x_cpu, w_y = recipes.gaussian(930 + dim, rows, dim, scale=1.2), recipes.gaussian(931, rows, dim)
    runs = []
    for _ in range(2):
        got = backward(f, x_cpu, w_y, False, rows)
        assert amd.last_kernel() == "linear_rows_bwd_weight_rt", amd.last_kernel()
        runs.append({k: v.clone() for k, v in got.items()})
    for k in "LSU":
        a, b = runs[0][k].contiguous().view(torch.int32), runs[1][k].contiguous().view(torch.int32)
        assert torch.equal(a, b), f"grad {k}: {int((a != b).sum())} of {a.numel()} elements differ between two runs"
        assert float(runs[0][k].abs().max()) > 0


def test_a_spline_model_with_glow_on_the_rt_kernels(amd, O, monkeypatch):
    """[ActNormFlow, Glow, NSF_CL(K = 8, n_h = 8)] x 2 at dim = 48 and 4,096 rows, Glow on the rt kernels: log_prob
    against the oracle by the parity rule (float64 head-room as the spline needs it near a knot)."""
    from glow_rt_model_child import DIM, ROWS, build_layers
    from test_hip_parity import _layers_f64
    from torch_mnf_amd import _dispatch

    monkeypatch.setattr(_dispatch, "GLOW_RT_MIN_ROWS", 0)
    flows, specs = build_layers()
    model = amd.NormalizingFlowModel(amd.StandardNormal(DIM), flows).to(DEV)
    x_cpu = recipes.gaussian(970, ROWS, DIM)
    with torch.no_grad():
        flows[1].forward(x_cpu.to(DEV))
        assert amd.last_kernel() == "linear_rows_rt", amd.last_kernel()
        lp = model.log_prob(x_cpu.to(DEV))
    _, ref = O.mean_log_prob(x_cpu, specs)
    _, ref64 = O.mean_log_prob(x_cpu.double(), _layers_f64(specs))
    assert_parity(lp, ref.numpy(), ref64.float().numpy(), "glow rt spline model d=48 log_prob")


def test_a_graphed_training_step_of_that_model_replays_identically():
    """One GraphedStep of -log_prob.mean() captured and replayed for 3 steps, twice: identical parameters under
    MNF_DETERMINISTIC=1 (the switch is read once per process: a child, started fresh)."""
    env = dict(os.environ, MNF_DETERMINISTIC="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "glow_rt_model_child.py")], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    tail = "\n".join((p.stdout + p.stderr).splitlines()[-30:])
    assert p.returncode == 0, tail
    assert "glow rt model child ok" in p.stdout, tail
