"""Glow.inverse followed by ActNormFlow.inverse at any 2 <= dim <= 1024 as one launch each way (kernel families
"glow_actnorm_inv_rt" and "glow_actnorm_inv_bwd_rt", csrc/mnf_linear_mfma.hip), with the log-prob epilogue.

The forward kernel keeps mnf_linear_rows_rt's k-ascending fmaf chain and applies mnf_affine_const's expression to its own
columns; the grad_u kernel applies mnf_affine_const_bwd's product to its row loads and reads M transposed.  So z, the
pair's log|det J| and grad_u are compared with the layer-by-layer kernels WITHOUT a tolerance (by value: a zero-padded
k-step turns an accumulator of -0 into +0).  The sums over the rows have an order of their own: they are held to the
float64 oracle with tests/test_hip_round4.py's budgets for the per-shape pair, and two runs must give the same bits."""
import math

import pytest
import torch

import recipes
from helpers import normwise_err
from test_hip_round4 import _pair_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
# 184: the largest dim whose M stays resident in LDS next to the staged t and e^-s (188 x 208 floats + 8 KB > 160 KB)
RESIDENT_MAX = 184


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


def _err(a, b) -> float:
    return normwise_err(a.detach().cpu().numpy(), b.detach().cpu().numpy())


def _device_case(seed, rows, dim):
    """the float64 case and its fp32 copies on the device; s and t 4-byte aligned only, as views into a flat buffer are"""
    u, M, s, t, gz = _pair_case(seed, rows, dim)
    st = torch.cat((torch.zeros(1), s.float().reshape(-1), t.float().reshape(-1))).to(DEV)
    dev = dict(u=u.float().to(DEV), M=M.float().to(DEV).contiguous(), s=st[1:1 + dim], t=st[1 + dim:1 + 2 * dim],
               gz=gz.float().to(DEV))
    assert dev["s"].data_ptr() % 16 == 4
    return (u, M, s, t, gz), dev


def _fwd(amd, d, z, ld_glow, ld_out, ld_rows=None, lp=None, s=None, t=None):
    rows, dim = d["u"].shape
    amd._lib.check("mnf_glow_actnorm_inv_rt", amd._lib.load().mnf_glow_actnorm_inv_rt(
        d["u"].data_ptr(), d["M"].data_ptr(), (d["s"] if s is None else s).data_ptr(), (d["t"] if t is None else t).data_ptr(),
        None if z is None else z.data_ptr(), ld_glow.data_ptr(), ld_out.data_ptr(), None if ld_rows is None else ld_rows.data_ptr(),
        None if lp is None else lp.data_ptr(), rows, dim, None))
    assert amd.last_kernel() == "glow_actnorm_inv_rt", amd.last_kernel()


def _bwd(amd, d, z, gz, g_lp, gu, gM, gs, gt, g_ld, gld):
    lib = amd._lib.load()
    rows, dim = d["u"].shape
    n = lib.mnf_glow_actnorm_inv_bwd_rt_workspace(rows, dim)
    assert n > 0
    work = torch.empty(n, device=DEV)
    p = lambda a: None if a is None else a.data_ptr()  # noqa: E731
    amd._lib.check("mnf_glow_actnorm_inv_bwd_rt", lib.mnf_glow_actnorm_inv_bwd_rt(
        d["u"].data_ptr(), z.data_ptr(), p(gz), p(g_lp), d["M"].data_ptr(), d["s"].data_ptr(), d["t"].data_ptr(), gu.data_ptr(),
        gM.data_ptr(), p(gs), p(gt), p(g_ld), p(gld), rows, dim, work.data_ptr(), n, None))
    assert amd.last_kernel() == "glow_actnorm_inv_bwd_rt", amd.last_kernel()


# (dim, rows): one row; a partial tile; partial column tiles over many row tiles; dim % 4 != 0 (scalar stores); the
# largest resident dim and the first streamed one; several column groups, streamed; the envelope's edge
BIT_CASES = [(2, 1), (6, 17), (48, 1031), (50, 4099), (100, 517), (RESIDENT_MAX, 130), (RESIDENT_MAX + 1, 130), (520, 130),
             (1024, 33)]


@pytest.mark.parametrize("dim,rows", BIT_CASES, ids=lambda v: str(v))
def test_z_log_det_and_grad_u_are_the_layer_by_layer_kernels_bit_for_bit(amd, dim, rows):
    lib = amd._lib.load()
    _, d = _device_case(2000 + dim, rows, dim)
    u, M, s, t, gz = (d[k] for k in ("u", "M", "s", "t", "gz"))
    # layer by layer: mnf_linear_rows_rt, then mnf_affine_const inverse (its log|det J| = -sum s from sum_vec_kernel)
    v, z_ref, ld_an = torch.empty_like(u), torch.empty_like(u), torch.empty(1, device=DEV)
    amd._lib.check("mnf_linear_rows_rt", lib.mnf_linear_rows_rt(u.data_ptr(), M.data_ptr(), v.data_ptr(), rows, dim, 0, None))
    amd._lib.check("mnf_affine_const", lib.mnf_affine_const(v.data_ptr(), z_ref.data_ptr(), s.data_ptr(), t.data_ptr(), None, 0,
                                                            ld_an.data_ptr(), rows, dim, 1, None))
    ld_glow = torch.full((1,), 0.75, device=DEV)
    ld_ref = ld_glow + ld_an
    # ... and backward: grad_z * expf(-s) (mnf_affine_const_bwd), then mnf_linear_rows_rt on M transposed
    gv, gu_ref = torch.empty_like(u), torch.empty_like(u)
    amd._lib.check("mnf_affine_const_bwd", lib.mnf_affine_const_bwd(v.data_ptr(), z_ref.data_ptr(), gz.data_ptr(), s.data_ptr(),
                                                                    gv.data_ptr(), None, None, rows, dim, 1, None))
    amd._lib.check("mnf_linear_rows_rt", lib.mnf_linear_rows_rt(gv.data_ptr(), M.data_ptr(), gu_ref.data_ptr(), rows, dim, 1, None))

    z, ld = torch.full_like(u, float("nan")), torch.empty(1, device=DEV)
    _fwd(amd, d, z, ld_glow, ld)
    gu = torch.full_like(u, float("nan"))
    gM, gs, gt = torch.zeros(dim, dim, device=DEV), torch.zeros(dim, device=DEV), torch.zeros(dim, device=DEV)
    _bwd(amd, d, z, gz, None, gu, gM, gs, gt, None, None)
    # s = t = 0: the product alone
    zero = torch.zeros(2 * dim + 1, device=DEV)
    v_pair, ld0 = torch.full_like(u, float("nan")), torch.empty(1, device=DEV)
    _fwd(amd, d, v_pair, ld_glow, ld0, s=zero[1:1 + dim], t=zero[1 + dim:])
    torch.cuda.synchronize()
    assert torch.equal(v_pair, v), f"u @ M: {int((v_pair != v).sum())} of {v.numel()} elements differ from mnf_linear_rows_rt"
    assert float(ld0) == 0.75
    assert torch.equal(z, z_ref), f"z: {int((z != z_ref).sum())} of {z.numel()} elements differ"
    assert torch.equal(ld, ld_ref), (float(ld), float(ld_ref))
    assert torch.equal(gu, gu_ref), f"grad_u: {int((gu != gu_ref).sum())} of {gu.numel()} elements differ"
    assert bool(torch.isfinite(gM).all()) and float(gM.abs().max()) > 0


ORACLE_CASES = [(48, 1031), (100, 517), (520, 130), (50, 30001)]


@pytest.mark.parametrize("dim,rows", ORACLE_CASES, ids=lambda v: str(v))
def test_pair_kernels_vs_float64_oracle(amd, O, dim, rows):
    """The oracle's two layers composed in float64 and torch.autograd through them, with the budgets of
    test_hip_round4.py::test_glow_actnorm_inverse_pair_kernels_vs_float64_oracle: 2e-6 normwise on the rows, 2e-5 on the
    sums over the rows."""
    (u, M, s, t, gz), d = _device_case(100 + rows + dim, rows, dim)
    u64, M64, s64, t64 = (a.clone().requires_grad_(True) for a in (u, M, s, t))
    z64, _ = O.affine_const(u64 @ M64, s64, t64, inverse=True)
    z64.backward(gz)
    z, ld = torch.empty_like(d["u"]), torch.empty(1, device=DEV)
    _fwd(amd, d, z, torch.full((1,), 0.75, device=DEV), ld)
    gu = torch.full_like(d["u"], float("nan"))
    gM, gs, gt = torch.zeros(dim, dim, device=DEV), torch.zeros(dim, device=DEV), torch.zeros(dim, device=DEV)
    g_ld = torch.full((1,), -0.3, device=DEV)  # cotangent of the pair's log|det J| = 0.75 - sum s
    _bwd(amd, d, z, d["gz"], None, gu, gM, gs, gt, g_ld, None)
    torch.cuda.synchronize()
    # (fp32: s rounded once, then at most 9 + 6 + 1 adds per chain, each within 2^-24 of a partial sum <= 0.75 + sum |s|)
    assert abs(float(ld) - (0.75 - float(s.sum()))) <= 1.1e-6 * (0.75 + float(s.abs().sum()))
    errs = dict(z=_err(z.double(), z64), gu=_err(gu.double(), u64.grad), gM=_err(gM.double(), M64.grad),
                gs=_err((gs - 0.3).double(), s64.grad.reshape(-1)), gt=_err(gt.double(), t64.grad.reshape(-1)))
    print(f"pair rt d={dim} rows={rows}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert errs["z"] <= 2e-6 and errs["gu"] <= 2e-6
    assert errs["gM"] <= 2e-5 and errs["gs"] <= 2e-5 and errs["gt"] <= 2e-5   # (grad_ld entered grad_s: +0.3 per column)
    # the sums are ADDED to, and either column sum may be left out
    _bwd(amd, d, z, d["gz"], None, gu, gM, None, gt, None, None)
    gs_before = gs.clone()
    _bwd(amd, d, z, d["gz"], None, gu, gM, gs, None, None, None)
    torch.cuda.synchronize()
    assert _err(gM.double(), 3 * M64.grad) <= 2e-5 and _err(gt.double(), 2 * t64.grad.reshape(-1)) <= 2e-5
    assert _err((gs - gs_before).double(), s64.grad.reshape(-1)) <= 2e-5


@pytest.mark.parametrize("dim,rows", ORACLE_CASES, ids=lambda v: str(v))
def test_pair_logprob_kernels_vs_float64_oracle(amd, O, dim, rows):
    """The pair closing a density pass, with the budgets of
    test_hip_round4.py::test_glow_actnorm_inverse_pair_logprob_kernels_vs_float64_oracle.  The sums sit back to back here,
    as the autograd node keeps them: one reduction launch for all four."""
    (u, M, s, t, _), d = _device_case(500 + rows + dim, rows, dim)
    g = torch.Generator().manual_seed(9 + rows)
    ld_rows = torch.randn(rows, generator=g, dtype=torch.float64)
    g_lp = torch.randn(rows, generator=g, dtype=torch.float64) / rows
    u64, M64, s64, t64, ldr64 = (a.clone().requires_grad_(True) for a in (u, M, s, t, ld_rows))
    ldg64 = torch.tensor(0.75, dtype=torch.float64, requires_grad=True)
    z64, ld_an = O.affine_const(u64 @ M64, s64, t64, inverse=True)
    lp64 = ldr64 + ldg64 + ld_an + (-0.5 * z64 ** 2 - 0.5 * math.log(2 * math.pi)).sum(1)  # distributions: Normal(0, 1)
    lp64.backward(g_lp)
    ldg, ldr, gl = torch.full((1,), 0.75, device=DEV), ld_rows.float().to(DEV), g_lp.float().to(DEV)
    lp, lp_only, z, ld = (torch.empty(rows, device=DEV), torch.empty(rows, device=DEV), torch.empty_like(d["u"]),
                          torch.empty(1, device=DEV))
    _fwd(amd, d, z, ldg, ld, ldr, lp)
    _fwd(amd, d, None, ldg, ld, ldr, lp_only)  # z not wanted
    gu = torch.full_like(d["u"], float("nan"))
    sums = torch.zeros(dim * dim + 2 * dim + 1, device=DEV)
    gM, gs = sums[:dim * dim], sums[dim * dim:dim * dim + dim]
    gt, gld = sums[dim * dim + dim:dim * dim + 2 * dim], sums[dim * dim + 2 * dim:]
    _bwd(amd, d, z, None, gl, gu, gM, gs, gt, None, gld)
    torch.cuda.synchronize()
    errs = dict(lp=_err(lp.double(), lp64.detach()), z=_err(z.double(), z64), gu=_err(gu.double(), u64.grad),
                gM=_err(gM.view(dim, dim).double(), M64.grad), gs=_err(gs.double(), s64.grad.reshape(-1)),
                gt=_err(gt.double(), t64.grad.reshape(-1)), gld=abs(float(gld) - float(ldg64.grad)))
    print(f"pair rt logprob d={dim} rows={rows}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert torch.equal(lp, lp_only)
    assert errs["lp"] <= 2e-6 and errs["z"] <= 2e-6 and errs["gu"] <= 2e-6
    assert errs["gM"] <= 2e-5 and errs["gs"] <= 2e-5 and errs["gt"] <= 2e-5
    assert errs["gld"] <= 2e-5 * max(1.0, float(g_lp.abs().sum()))
    # separate buffers take the other reduction path: the same bits
    gM2, gs2, gt2, gld2 = (torch.zeros(n, device=DEV) for n in (dim * dim, dim, dim, 1))
    _bwd(amd, d, z, None, gl, gu, gM2, gs2, gt2, None, gld2)
    torch.cuda.synchronize()
    for a, b in ((gM, gM2), (gs, gs2), (gt, gt2), (gld, gld2)):
        assert torch.equal(a.contiguous().view(torch.int32), b.view(torch.int32))


def test_the_sums_have_the_same_bits_every_run(amd):
    """(100, 30001): more than 32 row slices, so the two-step reduction; no environment switch set."""
    dim, rows = 100, 30001
    _, d = _device_case(77, rows, dim)
    gl = (torch.randn(rows, generator=torch.Generator().manual_seed(78)) / rows).to(DEV)
    z, ld = torch.empty_like(d["u"]), torch.empty(1, device=DEV)
    _fwd(amd, d, z, torch.zeros(1, device=DEV), ld)
    runs = []
    for form in ("log-prob", "log-prob", "plain", "plain"):
        gu = torch.empty_like(d["u"])
        gM, gs, gt, gld = (torch.zeros(n, device=DEV) for n in (dim * dim, dim, dim, 1))
        if form == "plain":
            _bwd(amd, d, z, d["gz"], None, gu, gM, gs, gt, None, None)
        else:
            _bwd(amd, d, z, None, gl, gu, gM, gs, gt, None, gld)
        torch.cuda.synchronize()
        runs.append((gM, gs, gt, gld, gu))
    for a, b in ((runs[0], runs[1]), (runs[2], runs[3])):
        for name, x, y in zip(("grad_m", "grad_s", "grad_t", "grad_ld_glow", "grad_u"), a, b):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), name
        assert float(a[0].abs().max()) > 0 and float(a[1].abs().max()) > 0 and float(a[2].abs().max()) > 0
    assert float(runs[0][3].abs()) > 0


# ------------------------------------------------------------------------------------------------------- model level
def _spline_model(amd, dim, blocks=2):
    flows = []
    for i in range(blocks):
        ap, gp = recipes.actnorm_params(940 + i, dim), recipes.glow_params(950 + i, dim)
        an, gl, nsf = amd.ActNormFlow(dim), amd.Glow(dim), amd.NSF_CL(dim, K=8, B=3, n_h=8)
        an.load_state_dict(ap)
        an.data_dep_init_done = True
        gl.P = gp["P"]
        gl.load_state_dict({k: gp[k] for k in "LSU"})
        nsf.load_state_dict(recipes.nsf_cl_params(960 + i, dim, 8, 8))
        flows += [an, gl, nsf]
    return amd.NormalizingFlowModel(amd.StandardNormal(dim), flows).to(DEV)


@pytest.fixture
def families(amd, monkeypatch):
    """the kernel family behind every library call of the test, in order"""
    seen, check = [], amd._lib.check

    def recording_check(name, rc):
        seen.append(amd.last_kernel())
        return check(name, rc)

    monkeypatch.setattr(amd._lib, "check", recording_check)
    return seen


def _training_pass(amd, model, x_cpu, families, fused, backward=True):
    flows_mod = amd.flows
    for p in model.parameters():
        p.grad = None
    x = x_cpu.to(DEV).requires_grad_(True)
    del families[:]
    env, flows_mod._NO_PAIR_FUSION_ENV = flows_mod._NO_PAIR_FUSION_ENV, not fused
    try:
        loss = -model.log_prob(x).mean()
        if backward:
            loss.backward()
    finally:
        flows_mod._NO_PAIR_FUSION_ENV = env
    torch.cuda.synchronize()
    return (loss.detach().clone(), x.grad, {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None},
            set(families))


def test_spline_model_training_pass_with_the_fused_rt_pair_matches_layer_by_layer(amd, families, monkeypatch):
    """[ActNormFlow, Glow, NSF_CL(K = 8, n_h = 8)] x 2 at dim 48 and 4,096 rows: -mean log_prob and its gradients with
    the pair as one autograd node on the run-time-shaped kernels (both forms: the last pair closes the density pass)
    against the same pass layer by layer, with the budgets of
    test_hip_round4.py::test_spline_block_training_pass_with_the_fused_pair_matches_layer_by_layer."""
    from torch_mnf_amd import _dispatch

    monkeypatch.setattr(_dispatch, "GLOW_RT_MIN_ROWS", 0)
    monkeypatch.setattr(_dispatch, "GLOW_ACTNORM_RT", True)  # (the rt pair is opt-in)
    dim, rows = 48, 4096
    # the model of the test whose budgets these are: default-constructed layers, ActNorm initialised from the data (its
    # 4e-6 absolute budget on ActNorm's s is the fp32 error of O(1) sums that cancel to 1 / rows right after that step)
    torch.manual_seed(11)
    layers = []
    for _ in range(2):
        layers += [amd.ActNormFlow(dim), amd.Glow(dim), amd.NSF_CL(dim, K=8, B=3, n_h=8)]
    model = amd.NormalizingFlowModel(amd.StandardNormal(dim), layers).to(DEV)
    x_cpu = recipes.gaussian(970, rows, dim)
    with torch.no_grad():
        model.log_prob(x_cpu.to(DEV))  # ActNorm's data-dependent initialisation
    res = {fused: _training_pass(amd, model, x_cpu, families, fused) for fused in (True, False)}
    print(f"loss fused {float(res[True][0]):.9g} layers {float(res[False][0]):.9g}; x.grad {_err(res[True][1], res[False][1]):.2e}; "
          + " ".join(f"{n} {float((res[True][2][n] - g).abs().max()):.2e}" if n.endswith(".s")
                     else f"{n} {_err(res[True][2][n], g):.2e}" for n, g in res[False][2].items()))
    assert {"glow_actnorm_inv_rt", "glow_actnorm_inv_bwd_rt"} <= res[True][3], sorted(res[True][3])
    assert not {"glow_actnorm_inv_rt", "glow_actnorm_inv_bwd_rt"} & res[False][3], sorted(res[False][3])
    assert "linear_rows_rt" in res[False][3] and "linear_rows_rt" not in res[True][3]
    assert abs(float(res[True][0]) - float(res[False][0])) <= 1e-6 * abs(float(res[False][0]))
    assert _err(res[True][1], res[False][1]) <= 5e-6
    assert set(res[True][2]) == set(res[False][2]) and len(res[True][2]) > 0
    for n, g in res[False][2].items():
        if n.endswith(".s"):
            assert float((res[True][2][n] - g).abs().max()) <= 4e-6, n
        else:
            assert _err(res[True][2][n], g) <= 2e-5, n


@pytest.mark.parametrize("dim,rows", [(6, 1031), (200, 517)], ids=lambda v: str(v))
def test_spline_model_loss_with_the_fused_rt_pair_at_other_dims(amd, families, monkeypatch, dim, rows):
    from torch_mnf_amd import _dispatch

    monkeypatch.setattr(_dispatch, "GLOW_RT_MIN_ROWS", 0)
    monkeypatch.setattr(_dispatch, "GLOW_ACTNORM_RT", True)  # (the rt pair is opt-in)
    model = _spline_model(amd, dim)
    x_cpu = recipes.gaussian(971, rows, dim)
    res = {fused: _training_pass(amd, model, x_cpu, families, fused, backward=False) for fused in (True, False)}
    assert "glow_actnorm_inv_rt" in res[True][3] and "glow_actnorm_inv_rt" not in res[False][3]
    assert abs(float(res[True][0]) - float(res[False][0])) <= 1e-6 * abs(float(res[False][0]))


def test_switches(amd, families, monkeypatch):
    from torch_mnf_amd import _dispatch

    rt = {"glow_actnorm_inv_rt", "glow_actnorm_inv_bwd_rt"}
    x48 = recipes.gaussian(972, 517, 48)
    model = _spline_model(amd, 48, blocks=1)
    # the rt pair is opt-in: by default layer by layer even where Glow's rt kernels take any row count
    assert _dispatch.GLOW_ACTNORM_RT is False
    with monkeypatch.context() as m:
        m.setattr(_dispatch, "GLOW_RT_MIN_ROWS", 0)
        seen = _training_pass(amd, model, x48, families, True)[3]
        assert not rt & seen and "linear_rows_rt" in seen
    monkeypatch.setattr(_dispatch, "GLOW_ACTNORM_RT", True)
    # fewer than GLOW_RT_MIN_ROWS rows and no force: layer by layer
    assert 517 < _dispatch.GLOW_RT_MIN_ROWS
    assert not rt & _training_pass(amd, model, x48, families, True)[3]
    # force_generic = 2: the pair on the rt kernels at any row count; 1: layer by layer
    model.flows[1].force_generic = 2
    assert rt <= _training_pass(amd, model, x48, families, True)[3]
    model.flows[1].force_generic = 1
    seen = _training_pass(amd, model, x48, families, True)[3]
    assert not rt & seen and "linear_rows_generic" in seen
    # dim 32 stays on the per-shape pair, also where Glow's rt kernels would take any row count
    monkeypatch.setattr(_dispatch, "GLOW_RT_MIN_ROWS", 0)
    monkeypatch.setattr(_dispatch, "GLOW_ACTNORM_RT", True)  # (the rt pair is opt-in)
    model32 = _spline_model(amd, 32, blocks=1)
    seen = _training_pass(amd, model32, recipes.gaussian(973, 517, 32), families, True)[3]
    assert {"glow_actnorm_inv", "glow_actnorm_inv_bwd"} <= seen and not rt & seen
    model32.flows[1].force_generic = 2
    assert not (rt | {"glow_actnorm_inv"}) & _training_pass(amd, model32, recipes.gaussian(973, 517, 32), families, True)[3]
