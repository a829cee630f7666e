"""``NormalizingFlowModel.sample(..., return_log_prob=True)``: the sample and its own log-density from ONE forward pass,
log_q[r] = log N(z_r; 0, I) - log_det_forward(z_r).

* ``mnf_normal_rows_sq`` (noise bit for bit ``mnf_normal_rows``, |z|^2 from the registers) and ``mnf_gauss_logq_sq``, each
  against float64 with a bound that follows from fp32 rounding alone;
* the one-launch route (``mnf_affine_half_stack_sample_logq``, kernel family ``ahf_split_stack_sample_lq``): x bit for bit
  the x-only launch's, log_q of a row independent of where its batch ends, pieces concatenate;
* a float64 referee with nothing of the device in it (the host noise reference through the float64 oracle), with two
  preconditions asserted so that the budget cannot be met vacuously;
* the general route (run-time-shaped, narrow half, mixed block, fp32 request), the unseeded form, what the user sees
  (``log_prob(x)`` against log_q), gradients against the oracle's autograd, graph capture.

Models carry nn.Linear-range weights (``affine_half_params(s_last_gain=1)``) as in test_hip_sample_seeded.py, whose model
builders are reused here.  Measured figures: profiles/r30/README.md."""
import ctypes
import math

import numpy as np
import pytest
import torch

import recipes
import rng_reference as R
from helpers import budgeted, normwise_err
from test_hip_autograd import check_vs_float64
from test_hip_parity import DEV, _layers_f64, amd, build_ahf_stack, O  # noqa: F401  (amd, O: fixtures)
from test_hip_sample_seeded import (GROUP_ROWS, ROWS, SEEDS, SHAPES, ahf_layers, ahf_model, fp32_model, normal_rows, rt_model,
                                    same, spline_block_model)

pytestmark = pytest.mark.gpu

FAMILY = "ahf_split_stack_sample_lq"
SAMPLE_FAMILIES = ("ahf_split_stack_sample", FAMILY)
HALF_LOG_2PI = 0.5 * math.log(2 * math.pi)
U = 2.0 ** -24  # fp32 unit roundoff
WHOLE = 4099


def draw(model, rows, seed, first_row=0):
    """(x, log_q) without gradients: the route a sampling user takes."""
    with torch.no_grad():
        return model.sample(rows, seed=seed, first_row=first_row, return_log_prob=True)


def lq64_of(O, layers, seed, rows, dim, row0=0):
    """The float64 referee: the host noise reference through the float64 oracle.  Returns (lq64, z64, per-layer max |ld|)."""
    z64 = torch.from_numpy(R.z0_normal(seed, rows, dim, row0)[0])
    lq64 = -0.5 * (z64 * z64).sum(1) - dim * HALF_LOG_2PI - O.flow_stack(z64, _layers_f64(layers), False)[1]
    x, layer_max = z64, []
    for spec in _layers_f64(layers):
        x, ld = O.apply_layer(spec, x, False)
        layer_max.append(float(ld.abs().max()))
    return lq64, z64, layer_max


def lq32_of(O, layers, z64):
    """The oracle's own fp32 pass on the same noise (precondition (i))."""
    z = z64.float()
    return -0.5 * (z * z).sum(1) - z.shape[1] * np.float32(HALF_LOG_2PI) - O.flow_stack(z, layers, False)[1]


# ------------------------------------------------------------------------------------------------- 1. noise with |z|^2
@pytest.mark.parametrize("seed", SEEDS, ids=hex)
@pytest.mark.parametrize("rows,dim,row0", [(1, 1, 0), (17, 2, 5), (333, 50, 1000), (64, 800, 2 ** 31 - 7)])
def test_normal_rows_sq(amd, rows, dim, row0, seed):
    out = torch.full((rows, dim), float("nan"), device=DEV)
    sq = torch.full((rows,), float("nan"), device=DEV)
    amd._lib.check("mnf_normal_rows_sq", amd._lib.load().mnf_normal_rows_sq(
        ctypes.c_uint64(seed & R.M64), row0, out.data_ptr(), sq.data_ptr(), rows, dim, None))
    torch.cuda.synchronize()
    assert same(out, normal_rows(amd, seed, row0, rows, dim)), "the noise is not mnf_normal_rows' bit for bit"
    # any fp32 summation order of dim non-negative terms, each rounded once: relative error <= (dim + 1) u, first order
    ref = (out.double() ** 2).sum(1).cpu().numpy()
    rel = np.abs(sq.double().cpu().numpy() - ref) / ref
    print(f"mnf_normal_rows_sq {rows}x{dim}: worst relative error {rel.max():.3e}, bound {(dim + 1) * U * 1.01:.3e}")
    assert (rel <= (dim + 1) * U * 1.01).all(), (rel.max(), (dim + 1) * U * 1.01)


def test_normal_rows_sq_unaligned_rows(amd):
    """An output that is only 4-byte aligned (and one 8-byte aligned) takes the narrower stores: same numbers."""
    rows, dim, seed = 37, 8, SEEDS[1]
    ref = normal_rows(amd, seed, 3, rows, dim)
    for shift in (1, 2):
        buf = torch.full((rows * dim + 4,), float("nan"), device=DEV)
        sq = torch.empty(rows, device=DEV)
        out = buf[shift:shift + rows * dim]
        amd._lib.check("mnf_normal_rows_sq", amd._lib.load().mnf_normal_rows_sq(
            ctypes.c_uint64(seed), 3, out.data_ptr(), sq.data_ptr(), rows, dim, None))
        torch.cuda.synchronize()
        assert same(out.view(rows, dim), ref)
        assert bool(torch.isnan(buf[:shift]).all()) and bool(torch.isnan(buf[shift + rows * dim:]).all())


# ------------------------------------------------------------------------------------------------- 2. the epilogue
@pytest.mark.parametrize("rows", [1, 255, 4099])
@pytest.mark.parametrize("dim", [2, 800])
def test_gauss_logq_sq(amd, rows, dim):
    g = torch.Generator().manual_seed(3000 + rows + dim)
    sq = (torch.rand(rows, generator=g) * 2 * dim).to(DEV)
    ld = (torch.rand(rows, generator=g) * 100 - 50).to(DEV)
    lq = torch.full((rows,), float("nan"), device=DEV)
    amd._lib.check("mnf_gauss_logq_sq", amd._lib.load().mnf_gauss_logq_sq(sq.data_ptr(), ld.data_ptr(), lq.data_ptr(), rows, dim, None))
    torch.cuda.synchronize()
    ref = -0.5 * sq.double() - dim * HALF_LOG_2PI - ld.double()
    bound = 4 * U * (0.5 * sq.double() + dim * HALF_LOG_2PI + ld.double().abs())
    err = (lq.double() - ref).abs()
    print(f"mnf_gauss_logq_sq {rows} rows, dim {dim}: worst error / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())


# ------------------------------------------------------------------------------------------------- 3. one-launch route
@pytest.mark.parametrize("dim,hid,n_layers", SHAPES, ids=[f"d{d}-h{h}-L{n}" for d, h, n in SHAPES])
def test_one_launch_route(amd, dim, hid, n_layers):
    model = ahf_model(amd, dim, hid, n_layers)
    seed = SEEDS[1] + dim + hid
    whole_x, whole_lq = draw(model, WHOLE, seed)
    assert amd.last_kernel() == FAMILY, amd.last_kernel()
    for rows in ROWS:
        x, lq = draw(model, rows, seed)
        assert amd.last_kernel() == FAMILY, amd.last_kernel()
        assert not x.requires_grad and not lq.requires_grad
        assert same(x, model.sample(rows, seed=seed)), f"d={dim} hid={hid} L={n_layers} rows={rows}: x differs from the x-only launch"
        assert amd.last_kernel() == "ahf_split_stack_sample"
        assert lq.shape == (rows,) and lq.dtype == torch.float32 and bool(torch.isfinite(lq).all())
        assert same(lq, whole_lq[:rows]), f"d={dim} hid={hid} L={n_layers} rows={rows}: a row's log_q depends on where the batch ends"
        assert same(x, whole_x[:rows])


def test_group_loop_runs_more_than_once(amd):
    """More row groups than resident workgroups (dim <= 64: two workgroups per CU x 128 rows, + 77); two pieces split at an
    odd row, the second at first_row > 0, are the whole."""
    model = ahf_model(amd, 32, 16, 2)
    rows = 2 * torch.cuda.get_device_properties(0).multi_processor_count * GROUP_ROWS + 77
    x, lq = draw(model, rows, SEEDS[1])
    assert amd.last_kernel() == FAMILY
    assert same(x, model.sample(rows, seed=SEEDS[1])) and bool(torch.isfinite(lq).all())
    cut = rows // 2 | 1
    xa, lqa = draw(model, cut, SEEDS[1])
    xb, lqb = draw(model, rows - cut, SEEDS[1], first_row=cut)
    assert same(torch.cat([xa, xb]), x) and same(torch.cat([lqa, lqb]), lq)


# ------------------------------------------------------------------------------------------------- 4. float64 referee
def referee(amd, O, model, layers, dim, rows, seed, row0, what):
    lq64, z64, layer_max = lq64_of(O, layers, seed, rows, dim, row0)
    own = normwise_err(lq32_of(O, layers, z64).numpy(), lq64.numpy())
    floor = 100 * 1e-5 * float(lq64.abs().max())
    print(f"{what}: oracle fp32 vs float64 {own:.3e}; smallest layer max |log_det| {min(layer_max):.3g} against {floor:.3g}")
    assert own <= 1e-5, "precondition (i): the case is outside what fp32 can hold"
    assert min(layer_max) >= floor, "precondition (ii): a dropped layer would not show against the budget"
    x, lq = draw(model, rows, seed, row0)
    err = normwise_err(lq.cpu().numpy(), lq64.numpy())
    print(f"{what}: device log_q against float64: {err:.3e} ({100 * err / 1e-5:.0f} % of 1e-5)")
    budgeted(err, 1e-5, f"{what} vs float64 oracle on the reference noise")
    return x, lq


@pytest.mark.parametrize("dim,hid,n_layers", [(64, 24, 9), (256, 24, 2), (32, 16, 2)])
def test_log_q_against_the_float64_oracle(amd, O, dim, hid, n_layers):
    model = ahf_model(amd, dim, hid, n_layers)
    referee(amd, O, model, ahf_layers(dim, hid, n_layers), dim, 257, SEEDS[1], 0, f"sample log_q d={dim} h={hid} L={n_layers}")
    assert amd.last_kernel() == FAMILY


def test_log_q_against_the_float64_oracle_past_row_2_31(amd, O):
    dim, hid, n_layers = 64, 24, 9
    model = ahf_model(amd, dim, hid, n_layers)
    referee(amd, O, model, ahf_layers(dim, hid, n_layers), dim, 257, SEEDS[0], 2 ** 31 + 56, "sample log_q d=64 first_row 2^31+56")
    assert amd.last_kernel() == FAMILY


# ------------------------------------------------------------------------------------------------- 5. general route
def rt_layers():
    return [{"kind": "affine_half", "parity": bool(i % 2),
             "params": recipes.affine_half_params(2900 + i, 64, h_sizes=(24, 24), s_last_gain=1.0)} for i in range(3)]


def narrow_layers():
    return [{"kind": "affine_half", "parity": bool(i % 2), "params": recipes.affine_half_params(2910 + i, 2, s_last_gain=1.0)}
            for i in range(3)]


def check_general(amd, model, rows, seed):
    x, lq = draw(model, rows, seed)
    assert amd.last_kernel() not in SAMPLE_FAMILIES, amd.last_kernel()
    assert lq.shape == (rows,) and lq.dtype == torch.float32 and bool(torch.isfinite(lq).all())
    assert same(x, model.sample(rows, seed=seed))
    assert amd.last_kernel() not in SAMPLE_FAMILIES
    return x, lq


def test_general_route_run_time_shaped(amd, O):
    model, _ = rt_model(amd)
    rows, seed = 2100, SEEDS[1] + 3
    x, lq = check_general(amd, model, rows, seed)
    lq64, z64, _ = lq64_of(O, rt_layers(), seed, rows, 64)
    own = normwise_err(lq32_of(O, rt_layers(), z64).numpy(), lq64.numpy())
    assert own <= 1e-5
    err = normwise_err(lq.cpu().numpy(), lq64.numpy())
    print(f"general route, run-time-shaped: log_q against float64 {err:.3e} (oracle fp32 {own:.3e})")
    budgeted(err, 1e-5, "general-route log_q, run-time-shaped (64, (24, 24)) x 3, vs float64 oracle")
    # pieces of >= 2,048 rows (each on the kernel the whole took) concatenate bit for bit
    whole_x, whole_lq = draw(model, 4196, seed)
    xa, lqa = draw(model, 2048, seed)
    xb, lqb = draw(model, 2148, seed, first_row=2048)
    assert same(torch.cat([xa, xb]), whole_x) and same(torch.cat([lqa, lqb]), whole_lq)


def test_general_route_narrow_half(amd, O):
    layers = narrow_layers()
    model = build_ahf_stack(amd, layers, 2)
    rows, seed = 1000, SEEDS[0] + 5
    x, lq = check_general(amd, model, rows, seed)
    lq64, z64, _ = lq64_of(O, layers, seed, rows, 2)
    assert normwise_err(lq32_of(O, layers, z64).numpy(), lq64.numpy()) <= 1e-5
    budgeted(normwise_err(lq.cpu().numpy(), lq64.numpy()), 1e-5, "general-route log_q, dim 2 x 3 layers, vs float64 oracle")


def test_general_route_fp32_request(amd, O):
    model, rows = fp32_model(amd)
    seed = SEEDS[1] + 7
    x, lq = check_general(amd, model, rows, seed)
    layers = ahf_layers(64, 24, 3, base_seed=2930)
    lq64, z64, _ = lq64_of(O, layers, seed, rows, 64)
    assert normwise_err(lq32_of(O, layers, z64).numpy(), lq64.numpy()) <= 1e-5
    budgeted(normwise_err(lq.cpu().numpy(), lq64.numpy()), 1e-5, "general-route log_q, fp32 request, vs float64 oracle")


def test_general_route_mixed_block(amd):
    """[ActNormFlow, Glow, NSF_CL]: log_q is the formula on the forward pass's own log_det (the layers themselves are held
    to the oracle in their own tests): float64 on the device's z and log_det, at the epilogue's rounding bound."""
    model, rows = spline_block_model(amd)
    seed = SEEDS[1] + 9
    x, lq = check_general(amd, model, rows, seed)
    z = normal_rows(amd, seed, 0, rows, 16)
    with torch.no_grad():
        xs, ld = model.forward(z)
    assert same(xs[-1], x)
    sq = (z.double() ** 2).sum(1)
    ref = -0.5 * sq - 16 * HALF_LOG_2PI - ld.double()
    bound = (4 + 17) * U * (0.5 * sq + 16 * HALF_LOG_2PI + ld.double().abs())  # (the epilogue's 4 u + |z|^2's (dim + 1) u)
    assert bool(((lq.double() - ref).abs() <= bound).all())


# ------------------------------------------------------------------------------------------------- 6. what the user sees
def test_log_prob_of_the_sample_is_log_q(amd):
    model = ahf_model(amd, 64, 24, 9)
    x, lq = draw(model, WHOLE, SEEDS[0])
    assert amd.last_kernel() == FAMILY
    with torch.no_grad():
        lp = model.log_prob(x)
    err = normwise_err(lp.cpu().numpy(), lq.cpu().numpy())
    print(f"log_prob(x) against the sampler's log_q, (64, 24, 9) at {WHOLE} rows: {err:.3e} ({100 * err / 1e-5:.0f} % of 1e-5)")
    budgeted(err, 1e-5, "log_prob(sample) vs the sampler's own log_q, d=64 L=9")
    # the two routes' log_q: the general route on the same model (run fusion off for the call)
    model.fuse_affine_runs = False
    try:
        x2, lq2 = draw(model, WHOLE, SEEDS[0])
        assert amd.last_kernel() not in SAMPLE_FAMILIES
    finally:
        model.fuse_affine_runs = True
    diff = normwise_err(lq2.cpu().numpy(), lq.cpu().numpy())
    print(f"general-route log_q against one-launch log_q: {diff:.3e}")
    budgeted(diff, 1e-5, "general-route log_q vs one-launch log_q, d=64 L=9")


# ------------------------------------------------------------------------------------------------- 7. unseeded
def test_unseeded(amd):
    model, n = ahf_model(amd, 64, 24, 9), 1000
    with torch.no_grad():
        torch.manual_seed(11)
        x, lq = model.sample(n, return_log_prob=True)
        torch.manual_seed(11)
        assert same(x, model.sample(n))
        assert lq.shape == (n,) and lq.dtype == torch.float32 and not lq.requires_grad
        err = normwise_err(model.log_prob(x).cpu().numpy(), lq.cpu().numpy())
        print(f"unseeded: log_prob(x) against log_q {err:.3e}")
        budgeted(err, 1e-5, "unseeded log_prob(sample) vs log_q, d=64 L=9")


def test_no_rows(amd):
    model = ahf_model(amd, 64, 24, 9)
    for kw in (dict(seed=3), dict(seed=3, first_row=9), dict()):
        x0, lq0 = model.sample(0, return_log_prob=True, **kw)
        assert x0.shape == (0, 64) and lq0.shape == (0,) and lq0.dtype == torch.float32 and x0.is_cuda and lq0.is_cuda


# ------------------------------------------------------------------------------------------------- 8. gradients
def test_gradients_against_the_oracle(amd, O):
    dim, rows, seed = 8, 257, SEEDS[1] + 11
    layers = [{"kind": "affine_half", "parity": bool(i % 2), "params": recipes.affine_half_params(3100 + i, dim, s_last_gain=1.0)}
              for i in range(3)]
    model = build_ahf_stack(amd, layers, dim)
    z64 = torch.from_numpy(R.z0_normal(seed, rows, dim)[0])
    grads = {}
    for dt in (torch.float32, torch.float64):
        specs = [dict(s, params={k: v.detach().to(dt).clone().requires_grad_(True) for k, v in s["params"].items()}) for s in layers]
        z = z64.to(dt)
        xs, ld = O.flow_stack(z, specs, False)
        lq = -0.5 * (z * z).sum(1) - dim * HALF_LOG_2PI - ld
        ((lq + 0.5 * (xs[-1] ** 2).sum(1)).mean()).backward()
        grads[dt] = [{k: v.grad for k, v in s["params"].items()} for s in specs]
    x, lq = model.sample(rows, seed=seed, return_log_prob=True)
    assert x.requires_grad and lq.requires_grad
    assert amd.last_kernel() not in SAMPLE_FAMILIES
    (lq + 0.5 * (x ** 2).sum(1)).mean().backward()
    checked = 0
    for i, flow in enumerate(model.flows):
        for name, p in flow.named_parameters():
            assert p.grad is not None, (i, name)
            check_vs_float64(p.grad, grads[torch.float32][i][name], grads[torch.float64][i][name],
                             f"sample(return_log_prob) reverse-KL grad layer {i} {name}")
            checked += 1
    assert checked == 3 * 16
    with torch.no_grad():
        x0, lq0 = model.sample(rows, seed=seed, return_log_prob=True)
    # (the values are the autograd route's bit for bit only where both ran the same kernels: not asserted)
    assert not x0.requires_grad and not lq0.requires_grad and lq0.shape == lq.shape


def test_gradients_wanted_on_a_one_launch_model(amd, O):
    """The c2-shaped model's no-grad route is the one launch; with grad on it takes the general route through the layers'
    autograd nodes, and the forward values are still log q."""
    dim, hid, n_layers, rows, seed = 64, 24, 9, 257, SEEDS[1]
    model = ahf_model(amd, dim, hid, n_layers)
    assert any(p.requires_grad for p in model.parameters())
    x, lq = model.sample(rows, seed=seed, return_log_prob=True)
    assert amd.last_kernel() not in SAMPLE_FAMILIES, amd.last_kernel()
    assert x.requires_grad and lq.requires_grad
    lq64, _, _ = lq64_of(O, ahf_layers(dim, hid, n_layers), seed, rows, dim)
    budgeted(normwise_err(lq.detach().cpu().numpy(), lq64.numpy()), 1e-5, "autograd-route log_q d=64 L=9 vs float64 oracle")
    lq.mean().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    model.zero_grad(set_to_none=True)
    # without the flag a seeded call stays under no_grad, whatever the grad mode
    assert not model.sample(rows, seed=seed).requires_grad
    assert amd.last_kernel() == "ahf_split_stack_sample"


# ------------------------------------------------------------------------------------------------- 9. capture
def test_graph_capture(amd):
    model, rows, seed = ahf_model(amd, 64, 24, 9), 1000, SEEDS[1]
    eager_x, eager_lq = draw(model, rows, seed)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            draw(model, rows, seed)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_x, out_lq = draw(model, rows, seed)
    for _ in range(2):
        out_x.fill_(float("nan"))
        out_lq.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert same(out_x, eager_x) and same(out_lq, eager_lq)
