"""Seeded sampling of a run on the run-time-shaped tier as ONE launch: ``mnf_affine_half_rt_stack_sample`` and
``mnf_affine_half_rt_stack_sample_logq`` (kernel families ``ahf_stack_rt_sample(_lq)``, one layer ``ahf_rt_sample(_lq)``),
whose first layer generates its rows in registers instead of reading the tensor ``mnf_normal_rows`` writes.

* route and bits: x is ``torch.equal`` to ``forward(mnf_normal_rows(...))`` on the same tier, and the log-q call's x to the
  x-only call's, in every plan class -- odd half (pairs of the noise straddle the halves), even half that is no multiple of
  8, the fused two-net first layer, the second and the widest size class, a streaming single layer, the one-net branch
  (no scale / no shift), 32 layers -- at row counts around a tile, a workgroup's block and RT_MIN_ROWS;
* row purity: pieces cut at an odd row concatenate to the whole, past row 2^31, with more row blocks than workgroups; the
  seed is taken mod 2^64;
* an output that is only 4-byte aligned; log_q against a float64 referee with nothing of the device in it (the two
  preconditions of test_hip_sample_logq.py asserted) and against ``log_prob(x)``; the fall-backs; graph capture.

``_dispatch.RT_SAMPLE_MIN_ROWS`` is set here, so nothing depends on its shipped value; the layers carry
``force_generic = 2`` so that small row counts reach the tier.  Measured figures: profiles/r31/README.md."""
import ctypes

import pytest
import torch

import recipes
from helpers import budgeted, normwise_err
from test_hip_parity import DEV, amd, O  # noqa: F401  (amd, O: fixtures)
from test_hip_sample_logq import draw, referee
from test_hip_sample_seeded import SEEDS, same, two_launch

pytestmark = pytest.mark.gpu

STACK, STACK_LQ, ONE, ONE_LQ = "ahf_stack_rt_sample", "ahf_stack_rt_sample_lq", "ahf_rt_sample", "ahf_rt_sample_lq"
NEW_FAMILIES = (STACK, STACK_LQ, ONE, ONE_LQ)
ROWS = [1, 37, 257, 2049]

# name: (dim, h_sizes, parities, scale, shift, row counts) -- the code path each is here for is in the module docstring
CASES = {
    "d6_h8_L3_p010": (6, (8,), (0, 1, 0), True, True, ROWS),
    "d6_h8_L3_p101": (6, (8,), (1, 0, 1), True, True, ROWS),
    "d12_h8x8_L2": (12, (8, 8), (0, 1), True, True, ROWS),
    "d64_h24x24_L3": (64, (24, 24), (0, 1, 0), True, True, ROWS),
    "d64_h96_L2": (64, (96,), (0, 1), True, True, ROWS),
    "d16_h200_L2": (16, (200,), (0, 1), True, True, ROWS),
    "d1024_h256x256_L1": (1024, (256, 256), (1,), True, True, [300]),
    "d32_h24_L2_no_scale": (32, (24,), (0, 1), False, True, ROWS),
    "d32_h24_L2_no_shift": (32, (24,), (1, 0), True, False, ROWS),
    "d8_h8_L32": (8, (8,), tuple(i % 2 for i in range(32)), True, True, ROWS),
}


def layer_specs(name):
    dim, h_sizes, parities, scale, shift, _ = CASES[name]
    base = 3100 + 50 * list(CASES).index(name)
    # (32 layers of nn.Linear-range s on a 4-column half leave fp32 in the oracle itself: a tenth of that range there)
    gain = 0.1 if len(parities) == 32 else 1.0
    return [{"kind": "affine_half", "parity": bool(p),
             "params": recipes.affine_half_params(base + i, dim, h_sizes=h_sizes, s_last_gain=gain, scale=scale, shift=shift)}
            for i, p in enumerate(parities)]


_models = {}


def rt_model(amd, name, **flags):
    """The case's model on the run-time-shaped tier (every layer ``force_generic = 2``)."""
    key = (name, tuple(sorted(flags.items())))
    if key not in _models:
        dim, h_sizes, _, scale, shift, _ = CASES[name]
        flows = []
        for spec in layer_specs(name):
            f = amd.AffineHalfFlow(dim, spec["parity"], h_sizes=h_sizes, scale=scale, shift=shift)
            f.load_state_dict(spec["params"])
            f.force_generic = 2
            for k, v in flags.items():
                setattr(f, k, v)
            flows.append(f)
        _models[key] = amd.NormalizingFlowModel(amd.StandardNormal(dim), flows).to(DEV)
    return _models[key]


@pytest.fixture
def route_on(amd, monkeypatch):
    monkeypatch.setattr(amd._dispatch, "RT_SAMPLE_MIN_ROWS", 1)


def families(name):
    return (ONE, ONE_LQ) if len(CASES[name][2]) == 1 else (STACK, STACK_LQ)


# ------------------------------------------------------------------------------------------------- (a) route and bits
@pytest.mark.parametrize("name", list(CASES))
def test_one_launch_is_the_two_launch_arithmetic(amd, route_on, name):
    model = rt_model(amd, name)
    dim, fam, fam_lq = CASES[name][0], *families(name)
    for k, rows in enumerate(CASES[name][5]):
        seed = SEEDS[k % 2] + k
        x = model.sample(rows, seed=seed)
        assert amd.last_kernel() == fam, amd.last_kernel()
        assert x.shape == (rows, dim) and x.dtype == torch.float32 and not x.requires_grad
        ref = two_launch(amd, model, seed, 0, rows)
        assert amd.last_kernel() in ("ahf_stack_rt", "ahf_rt"), amd.last_kernel()
        assert bool(torch.isfinite(ref).all())
        assert same(x, ref), f"{name} rows={rows}: {int((x != ref).sum())} elements differ from forward(mnf_normal_rows)"
        x2, lq = draw(model, rows, seed)
        assert amd.last_kernel() == fam_lq, amd.last_kernel()
        assert same(x2, x), f"{name} rows={rows}: x of the log-q call differs from the x-only call"
        assert lq.shape == (rows,) and lq.dtype == torch.float32 and not lq.requires_grad and bool(torch.isfinite(lq).all())


# ------------------------------------------------------------------------------------------------- (b) row purity
def test_pieces_past_row_2_31_and_the_seed_mod_2_64(amd, route_on):
    name, rows, row0, seed = "d6_h8_L3_p010", 257, 2 ** 31 + 56, SEEDS[1]
    model = rt_model(amd, name)
    x, lq = draw(model, rows, seed, row0)
    assert amd.last_kernel() == STACK_LQ
    assert same(x, two_launch(amd, model, seed, row0, rows))
    cut = 101
    xa, lqa = draw(model, cut, seed, row0)
    xb, lqb = draw(model, rows - cut, seed, row0 + cut)
    assert same(torch.cat([xa, xb]), x) and same(torch.cat([lqa, lqb]), lq)
    assert same(torch.cat([model.sample(cut, seed=seed, first_row=row0), model.sample(rows - cut, seed=seed, first_row=row0 + cut)]), x)
    assert amd.last_kernel() == STACK
    x64, lq64 = draw(model, rows, seed + 2 ** 64, row0)
    assert same(x64, x) and same(lq64, lq)
    x1, lq1 = draw(model, rows, seed + 1, row0)
    assert not same(x1, x) and not same(lq1, lq)
    assert not same(draw(model, rows, seed, row0 + 1)[0], x)


def test_more_row_blocks_than_workgroups(amd, route_on):
    """2^18 + 77 rows at (8, (8,)) x 2: every workgroup of the persistent grid walks several row blocks."""
    dim, rows, seed = 8, 2 ** 18 + 77, SEEDS[0]
    flows = []
    for i in range(2):
        f = amd.AffineHalfFlow(dim, bool(i % 2), h_sizes=(8,))
        f.load_state_dict(recipes.affine_half_params(3900 + i, dim, h_sizes=(8,), s_last_gain=1.0))
        f.force_generic = 2
        flows.append(f)
    model = amd.NormalizingFlowModel(amd.StandardNormal(dim), flows).to(DEV)
    x, lq = draw(model, rows, seed)
    assert amd.last_kernel() == STACK_LQ
    assert same(x, two_launch(amd, model, seed, 0, rows)) and bool(torch.isfinite(lq).all())
    assert same(x, model.sample(rows, seed=seed)) and amd.last_kernel() == STACK
    cut = rows // 2 | 1
    xa, lqa = draw(model, cut, seed)
    xb, lqb = draw(model, rows - cut, seed, cut)
    assert same(torch.cat([xa, xb]), x) and same(torch.cat([lqa, lqb]), lq)


# ------------------------------------------------------------------------------------------------- (c) unaligned output
def test_output_at_a_4_byte_offset(amd, route_on):
    name, rows, seed, row0 = "d64_h24x24_L3", 257, SEEDS[1], 3
    model = rt_model(amd, name)
    dim = CASES[name][0]
    run = model._sample_run()
    f0, n = run.layers[0], len(run.layers)
    flat = run.rt_flat(torch.device(DEV, torch.cuda.current_device()))
    par = amd._lib.int_array([int(bool(f.parity)) for f in run.layers])
    lib = amd._lib.load()
    shape = (dim, len(f0.h_sizes), f0._hid, 1, 1)
    want_x, want_lq = draw(model, rows, seed, row0)
    for shift in (0, 1):
        buf = torch.full((rows * dim + 4,), float("nan"), device=DEV)
        y = buf[shift:shift + rows * dim]
        assert y.data_ptr() % 16 == 4 * shift
        amd._lib.check("mnf_affine_half_rt_stack_sample", lib.mnf_affine_half_rt_stack_sample(
            ctypes.c_uint64(seed), row0, y.data_ptr(), flat.data_ptr(), par, n, rows, *shape, None))
        torch.cuda.synchronize()
        assert amd.last_kernel() == STACK
        assert same(y.view(rows, dim), want_x), f"y at a {4 * shift}-byte offset"
        assert bool(torch.isnan(buf[:shift]).all()) and bool(torch.isnan(buf[shift + rows * dim:]).all())
        buf.fill_(float("nan"))
        lq = torch.full((rows + 2,), float("nan"), device=DEV)
        amd._lib.check("mnf_affine_half_rt_stack_sample_logq", lib.mnf_affine_half_rt_stack_sample_logq(
            ctypes.c_uint64(seed), row0, y.data_ptr(), lq[1:].data_ptr(), flat.data_ptr(), par, n, rows, *shape, None))
        torch.cuda.synchronize()
        assert amd.last_kernel() == STACK_LQ
        assert same(y.view(rows, dim), want_x) and same(lq[1:rows + 1], want_lq)
        assert bool(torch.isnan(lq[:1]).all()) and bool(torch.isnan(lq[rows + 1:]).all())
        assert bool(torch.isnan(buf[:shift]).all()) and bool(torch.isnan(buf[shift + rows * dim:]).all())


# ------------------------------------------------------------------------------------------------- (d) float64 referee
@pytest.mark.parametrize("name", ["d6_h8_L3_p010", "d64_h24x24_L3", "d64_h96_L2"])
def test_log_q_against_the_float64_oracle(amd, O, route_on, name):
    """Measured on an MI355X: see profiles/r31/README.md."""
    model, dim = rt_model(amd, name), CASES[name][0]
    x, lq = referee(amd, O, model, layer_specs(name), dim, 257, SEEDS[1], 0, f"rt sample log_q {name}")
    assert amd.last_kernel() == STACK_LQ, amd.last_kernel()
    with torch.no_grad():
        lp = model.log_prob(x)
    err = normwise_err(lp.cpu().numpy(), lq.cpu().numpy())
    print(f"{name}: log_prob(x) against the sampler's log_q: {err:.3e} ({100 * err / 1e-5:.0f} % of 1e-5)")
    budgeted(err, 1e-5, f"log_prob(sample) vs the rt sampler's own log_q, {name}")


# ------------------------------------------------------------------------------------------------- (e) fall-backs
def test_switch_none_is_the_general_route(amd, monkeypatch):
    monkeypatch.setattr(amd._dispatch, "RT_SAMPLE_MIN_ROWS", None)
    name, rows, seed = "d64_h24x24_L3", 257, SEEDS[1]
    model = rt_model(amd, name)
    x = model.sample(rows, seed=seed)
    assert amd.last_kernel() == "ahf_stack_rt", amd.last_kernel()
    x2, lq = draw(model, rows, seed)
    assert amd.last_kernel() not in NEW_FAMILIES, amd.last_kernel()
    assert same(x2, x)
    monkeypatch.setattr(amd._dispatch, "RT_SAMPLE_MIN_ROWS", rows + 1)  # below the floor: the same
    assert same(model.sample(rows, seed=seed), x) and amd.last_kernel() == "ahf_stack_rt"
    monkeypatch.setattr(amd._dispatch, "RT_SAMPLE_MIN_ROWS", rows)
    x3, lq3 = draw(model, rows, seed)
    assert amd.last_kernel() == STACK_LQ and same(x3, x)
    err = normwise_err(lq3.cpu().numpy(), lq.cpu().numpy())
    print(f"one-launch log_q against the general route's: {err:.3e}")
    budgeted(err, 1e-5, "rt one-launch log_q vs general-route log_q, (64, (24, 24)) x 3")


def test_gradients_wanted_take_the_general_route(amd, route_on):
    name, rows, seed = "d12_h8x8_L2", 257, SEEDS[0]
    model = rt_model(amd, name)
    assert any(p.requires_grad for p in model.parameters())
    x, lq = model.sample(rows, seed=seed, return_log_prob=True)
    assert amd.last_kernel() not in NEW_FAMILIES, amd.last_kernel()
    assert x.requires_grad and lq.requires_grad
    (lq + 0.5 * (x ** 2).sum(1)).mean().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool((p.grad != 0).any()) for p in model.parameters())
    model.zero_grad(set_to_none=True)
    x0, lq0 = draw(model, rows, seed)
    assert amd.last_kernel() == STACK_LQ and not x0.requires_grad and not lq0.requires_grad
    budgeted(normwise_err(lq.detach().cpu().numpy(), lq0.cpu().numpy()), 1e-5, "autograd-route log_q vs rt one-launch log_q")


def test_fp32_request_takes_the_general_route(amd, route_on):
    name, rows, seed = "d64_h24x24_L3", 2049, SEEDS[1]
    model = rt_model(amd, name, force_generic=0, force_fp32_mfma=True)
    x = model.sample(rows, seed=seed)
    assert amd.last_kernel() not in NEW_FAMILIES and not amd.last_kernel().endswith("_rt"), amd.last_kernel()
    x2, lq = draw(model, rows, seed)
    assert amd.last_kernel() not in NEW_FAMILIES, amd.last_kernel()
    assert same(x2, x) and bool(torch.isfinite(lq).all())
    # the same model without the request, at a row count the tier takes by itself (no force_generic)
    plain = rt_model(amd, name, force_generic=0)
    xp = plain.sample(rows, seed=seed)
    assert amd.last_kernel() == STACK, amd.last_kernel()
    assert same(xp, two_launch(amd, plain, seed, 0, rows))
    plain.sample(2047, seed=seed)  # below RT_MIN_ROWS rt_route says no, whatever the switch
    assert amd.last_kernel() not in NEW_FAMILIES, amd.last_kernel()


# ------------------------------------------------------------------------------------------------- (f) capture
def test_graph_capture(amd, route_on):
    model, rows, seed = rt_model(amd, "d64_h24x24_L3"), 1000, SEEDS[1]
    eager_x, eager_lq = draw(model, rows, seed)
    assert amd.last_kernel() == STACK_LQ
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            draw(model, rows, seed)
            model.sample(rows, seed=seed)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_x, out_lq = draw(model, rows, seed)
        out_only = model.sample(rows, seed=seed)
    for _ in range(2):
        for o in (out_x, out_lq, out_only):
            o.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert same(out_x, eager_x) and same(out_lq, eager_lq) and same(out_only, eager_x)
