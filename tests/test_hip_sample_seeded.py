"""Seeded sampling: ``NormalizingFlowModel.sample(n, seed=s, first_row=r0)`` returns rows r0 .. r0 + n - 1 of x = forward(z)
with z[r, c] = z0_normal(s, r, c), the library's counter-based normal stream (tests/rng_reference.py restates it).

* ``mnf_normal_rows`` (the stream with a row offset) against the host reference, under test_hip_rng.py's own rule and
  tolerance, and bit for bit ``mnf_sample_z0_noise`` at row0 = 0;
* the one-launch route (``mnf_affine_half_stack_sample``, kernel family ``ahf_split_stack_sample``: the noise is generated
  in the stack kernel's registers, only x is written) against the two-launch form ``forward(mnf_normal_rows(...))`` with
  ``torch.equal``: every full-tile shape class of the stack kernel (two tiles per wave at dim <= 64, one tile and eight
  waves above, dynamic LDS and chunked s / t at dim 256, hidden widths 16 / 24 / 32, one layer and several), row counts
  around a 16-row tile and around one 128-row group (16 rows x tiles x waves: 16 * 2 * 4 at dim <= 64, 16 * 1 * 8 above),
  one count past a full grid;
* the float64 oracle on the float64 reference noise (nothing of the device in it);
* chunks of one seed concatenate to the whole; every model without a sample launch takes the general route to the same
  definition; ``sample(n)`` without a seed is what it was; the launch is capturable; the C entry's argument checks.

Models carry nn.Linear-range weights (``affine_half_params(s_last_gain=1)``: |s| well below 2) so that no row leaves the
split range: the stack kernel decides its fp32 fall-back per wave, which would make a row depend on its tile mates."""
import ctypes

import numpy as np
import pytest
import torch

import recipes
import rng_reference as R
from helpers import budgeted, normwise_err
from test_hip_parity import DEV, _layers_f64, amd, build_ahf_stack, cuda, O  # noqa: F401  (amd, O: fixtures)
from test_hip_rng import NORMAL_TOL, check_normals

pytestmark = pytest.mark.gpu

SEEDS = [R.Z0_XOR, 0x123456789ABCDEF0]  # (0x5bd1e995: element (0, 0) has h1 == 0, the largest radius; seed >> 32 != 0)
GROUP_ROWS = 128
SHAPES = [(64, 24, 9), (32, 16, 2), (32, 24, 1), (128, 24, 3), (256, 24, 2), (128, 32, 2),  # (dim, hidden, layers)
          (64, 16, 2), (32, 32, 1), (64, 32, 1)]  # (hidden width 32 at d <= 64: one layer, else layer by layer)
ROWS = [1, 15, 16, 17, GROUP_ROWS - 1, GROUP_ROWS, GROUP_ROWS + 1, 4099]
FAMILY = "ahf_split_stack_sample"


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


def ahf_layers(dim, hid, n_layers, base_seed=2800):
    return [{"kind": "affine_half", "parity": bool(i % 2),
             "params": recipes.affine_half_params(base_seed + 16 * hid + i, dim, h_sizes=(hid,) * 3, s_last_gain=1.0)}
            for i in range(n_layers)]


_models = {}


def ahf_model(amd, dim, hid, n_layers):
    key = (dim, hid, n_layers)
    if key not in _models:
        flows = []
        for spec in ahf_layers(dim, hid, n_layers):
            f = amd.AffineHalfFlow(dim, spec["parity"], h_sizes=(hid,) * 3)
            f.load_state_dict(spec["params"])
            flows.append(f)
        _models[key] = amd.NormalizingFlowModel(amd.StandardNormal(dim), flows).to(DEV)
    return _models[key]


def normal_rows(amd, seed, row0, rows, dim):
    out = torch.full((rows, dim), float("nan"), device=DEV)
    amd._lib.check("mnf_normal_rows", amd._lib.load().mnf_normal_rows(
        ctypes.c_uint64(seed & R.M64), row0, out.data_ptr(), rows, dim, None))
    torch.cuda.synchronize()
    return out


def two_launch(amd, model, seed, row0, rows):
    """THE definition: the materialised noise through ``forward``."""
    with torch.no_grad():
        return model.forward(normal_rows(amd, seed, row0, rows, model.base.dim))[0][-1]


# ------------------------------------------------------------------------------------------------- noise with offset
@pytest.mark.parametrize("seed", SEEDS, ids=hex)
@pytest.mark.parametrize("rows,dim,row0", [(1, 1, 0), (17, 2, 5), (333, 50, 1000), (64, 800, 2 ** 31 - 7)])
def test_normal_rows_vs_reference(amd, rows, dim, row0, seed):
    got = normal_rows(amd, seed, row0, rows, dim).cpu().numpy()
    check_normals("z0", got, R.z0_normal(seed, rows, dim, row0), f"mnf_normal_rows {rows}x{dim} row0 {row0} seed {seed:#x}")
    assert NORMAL_TOL["z0"] == 9e-7


@pytest.mark.parametrize("seed", SEEDS, ids=hex)
def test_normal_rows_at_row0_zero_is_sample_z0_noise(amd, seed):
    for rows, dim in ((17, 2), (333, 50), (64, 800)):
        old = torch.full((rows, dim), float("nan"), device=DEV)
        amd._lib.check("mnf_sample_z0_noise", amd._lib.load().mnf_sample_z0_noise(
            ctypes.c_uint64(seed), old.data_ptr(), rows, dim, None))
        assert same(normal_rows(amd, seed, 0, rows, dim), old)
        assert same(amd.StandardNormal(dim).sample((rows,), seed=seed), old)
        assert same(amd.StandardNormal(dim).sample(rows, seed=seed, first_row=7), normal_rows(amd, seed, 7, rows, dim))


# ------------------------------------------------------------------------------------------------- one-launch route
@pytest.mark.parametrize("dim,hid,n_layers", SHAPES, ids=[f"d{d}-h{h}-L{n}" for d, h, n in SHAPES])
def test_one_launch_is_the_two_launch_arithmetic(amd, dim, hid, n_layers):
    model = ahf_model(amd, dim, hid, n_layers)
    for k, rows in enumerate(ROWS):
        seed = SEEDS[k % 2] + k
        x = model.sample(rows, seed=seed)
        assert amd.last_kernel() == FAMILY, amd.last_kernel()
        assert x.shape == (rows, dim) and x.dtype == torch.float32 and not x.requires_grad
        ref = two_launch(amd, model, seed, 0, rows)
        assert amd.last_kernel() != FAMILY
        assert bool(torch.isfinite(ref).all())
        assert same(x, ref), f"d={dim} hid={hid} L={n_layers} rows={rows}: {int((x != ref).sum())} elements differ"


def test_group_loop_runs_more_than_once(amd):
    """More row groups than the launch has workgroups: the launcher's resident count (dim <= 64: two workgroups per CU)
    x 128 rows, + 77."""
    dim = 32
    model = ahf_model(amd, dim, 16, 2)
    rows = 2 * torch.cuda.get_device_properties(0).multi_processor_count * GROUP_ROWS + 77
    x = model.sample(rows, seed=SEEDS[1])
    assert amd.last_kernel() == FAMILY
    assert same(x, two_launch(amd, model, SEEDS[1], 0, rows))


# ------------------------------------------------------------------------------------------------- independent reference
@pytest.mark.parametrize("dim,hid,n_layers", [(64, 24, 9), (256, 24, 2)])
def test_against_the_float64_oracle_on_the_reference_noise(amd, O, dim, hid, n_layers):
    """Measured on an MI355X: see profiles/r28/README.md."""
    rows, seed = 257, SEEDS[1]
    layers = ahf_layers(dim, hid, n_layers)
    z64 = torch.from_numpy(R.z0_normal(seed, rows, dim)[0])
    ref64 = O.flow_stack(z64, _layers_f64(layers), False)[0][-1].numpy()
    ref32 = O.flow_stack(z64.float(), layers, False)[0][-1].numpy()
    own = normwise_err(ref32, ref64)
    print(f"d={dim} L={n_layers}: the oracle's own fp32 pass against float64: {own:.3e}")
    assert own <= 1e-5, "the case is outside what fp32 can hold: not a case for this budget"
    model = ahf_model(amd, dim, hid, n_layers)
    x = model.sample(rows, seed=seed)
    assert amd.last_kernel() == FAMILY
    err = normwise_err(x.cpu().numpy(), ref64)
    print(f"d={dim} L={n_layers}: device sample against float64: {err:.3e} ({100 * err / 1e-5:.0f} % of 1e-5)")
    budgeted(err, 1e-5, f"seeded sample d={dim} L={n_layers} vs float64 oracle on the reference noise")


# ------------------------------------------------------------------------------------------------- general route
def rt_model(amd):
    dim = 64
    flows = []
    for i in range(3):
        f = amd.AffineHalfFlow(dim, bool(i % 2), h_sizes=(24, 24))
        f.load_state_dict(recipes.affine_half_params(2900 + i, dim, h_sizes=(24, 24), s_last_gain=1.0))
        flows.append(f)
    return amd.NormalizingFlowModel(amd.StandardNormal(dim), flows).to(DEV), 2049


def half_moons_model(amd):
    layers = [{"kind": "affine_half", "parity": bool(i % 2), "params": recipes.affine_half_params(2910 + i, 2, s_last_gain=1.0)}
              for i in range(9)]
    return build_ahf_stack(amd, layers, 2), 4096


def spline_block_model(amd):
    dim = 16
    torch.manual_seed(2920)
    model = amd.NormalizingFlowModel(amd.StandardNormal(dim), [amd.ActNormFlow(dim), amd.Glow(dim), amd.NSF_CL(dim, K=8, B=3, n_h=8)]).to(DEV)
    with torch.no_grad():
        model.inverse(cuda(recipes.gaussian(2921, 512, dim)))  # ActNorm's data-dependent initialisation
    assert model.flows[0].data_dep_init_done
    return model, 1000


def fp32_model(amd):
    model = build_ahf_stack(amd, ahf_layers(64, 24, 3, base_seed=2930), 64)
    for f in model.flows:
        f.force_fp32_mfma = True
    return model, 1000


GENERAL = {"rt_shaped": rt_model, "half_moons_dim2": half_moons_model, "spline_block": spline_block_model,
           "fp32_request": fp32_model}


@pytest.mark.parametrize("name", list(GENERAL))
def test_general_route(amd, name):
    model, rows = GENERAL[name](amd)
    seed = SEEDS[1] + 3
    x = model.sample(rows, seed=seed)
    assert amd.last_kernel() != FAMILY, amd.last_kernel()
    assert x.shape == (rows, model.base.dim) and bool(torch.isfinite(x).all())
    assert same(x, two_launch(amd, model, seed, 0, rows))
    # (a row range is again forward() on that range's noise -- whichever kernel forward picks at that row count)
    assert same(model.sample(rows - 100, seed=seed, first_row=100), two_launch(amd, model, seed, 100, rows - 100))


# ------------------------------------------------------------------------------------------------- chunks
@pytest.mark.parametrize("route", ["one_launch", "general"])
def test_chunks_equal_the_whole(amd, route):
    model = ahf_model(amd, 64, 24, 9) if route == "one_launch" else half_moons_model(amd)[0]
    seed = SEEDS[0]
    whole = model.sample(257, seed=seed)
    assert (amd.last_kernel() == FAMILY) == (route == "one_launch")
    parts = torch.cat([model.sample(100, seed=seed), model.sample(157, seed=seed, first_row=100)])
    assert same(parts, whole)
    assert same(model.sample(257, seed=seed + 2 ** 64), whole)  # (the seed is masked to 64 bits)
    assert not same(model.sample(257, seed=seed + 1), whole)
    assert model.sample(0, seed=seed).shape == (0, model.base.dim)


# ------------------------------------------------------------------------------------------------- nothing else moved
def test_unseeded_sample_is_unchanged(amd):
    model = ahf_model(amd, 64, 24, 9)
    torch.manual_seed(0)
    x = model.sample(1000)
    assert amd.last_kernel() == "ahf_split_stack"
    torch.manual_seed(0)
    z = model.base.sample(1000)
    assert same(x, model.forward(z)[0][-1])
    s = amd.StandardNormal(7).sample((5,))
    assert s.shape == (5, 7) and s.is_cuda and s.dtype == torch.float32
    assert amd.StandardNormal(7).sample().shape == (7,)


# ------------------------------------------------------------------------------------------------- capture
def test_graph_capture(amd):
    model, rows, seed = ahf_model(amd, 64, 24, 9), 1000, SEEDS[1]
    eager = model.sample(rows, seed=seed)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            model.sample(rows, seed=seed)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = model.sample(rows, seed=seed)
    for _ in range(2):
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert same(out, eager)


# ------------------------------------------------------------------------------------------------- argument validation
def test_c_entry_argument_checks(amd):
    L = amd._lib
    dim, rows = 64, 129
    model = ahf_model(amd, dim, 24, 9)
    run = model._sample_run()
    images, splits = run.images(torch.device(DEV, torch.cuda.current_device()))
    assert images is not None and splits is not None
    f0, n = run.layers[0], len(run.layers)
    par = L.int_array([int(bool(f.parity)) for f in run.layers])
    y = torch.full((rows, dim), float("nan"), device=DEV)

    def call(y_ptr=y.data_ptr(), n_layers=n, n_rows=rows, row0=0, img=images.data_ptr(), spl=splits.data_ptr(), parity=par):
        rc = L.load().mnf_affine_half_stack_sample(ctypes.c_uint64(5), row0, y_ptr, img, spl, parity, n_layers, n_rows, dim,
                                                  len(f0.h_sizes), f0._hid, None)
        torch.cuda.synchronize()
        return rc

    for bad in (dict(y_ptr=None), dict(n_layers=33), dict(n_layers=0), dict(n_rows=-1), dict(row0=-1), dict(img=None),
                dict(spl=None), dict(parity=None)):
        assert call(**bad) == L.MNF_ERR_INVALID_ARG, bad
    assert call(n_rows=0) == L.MNF_OK
    assert bool(torch.isnan(y).all()), "a rows == 0 call wrote something"
    assert call(y_ptr=y.data_ptr() + 4, n_rows=rows - 1) == L.MNF_ERR_UNSUPPORTED  # y not 16-byte aligned
    assert bool(torch.isnan(y).all())
    assert call() == L.MNF_OK and amd.last_kernel() == FAMILY
    assert same(y, model.sample(rows, seed=5))
