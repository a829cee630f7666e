"""The density-only stack launch (``mnf_affine_half_stack`` with ``y = NULL``): the no-grad ``log_prob`` writes no row
tensor.  The reference of every comparison is the STORING launch with the same ``logprob`` / ``sqnorm`` arguments (or
``model.inverse`` plus the separate epilogue), never a second density-only call; the launch runs the same arithmetic
whether or not it stores, so every comparison is bit for bit (``same_bits``: NaN payloads included).

Shapes: dim 64 (two tiles per wave), 256 (one tile, eight waves, dynamic LDS, chunked s / t), 40 (ragged halves with
16-byte accesses), 6 and 2 (ragged, element by element); 2, 3 and 9 layers (both LDS buffers end a run); row counts
around one 128-row group, and one count past a full grid so the group loop runs twice."""
import ctypes

import pytest
import torch

import recipes
from helpers import c2_layers
from test_hip_parity import DEV, amd, build_ahf_stack, cuda, select_kernel  # noqa: F401  (amd: fixture)

pytestmark = pytest.mark.gpu

DIMS = [64, 256, 40, 6, 2]
ROWS = [1, 127, 128, 129, 1013]
GROUP_ROWS = 128  # 16 rows x tiles x waves of ahf_split_stack_kernel: 16 * 2 * 4 at d <= 64, 16 * 1 * 8 above


def rows_past_one_grid(dim):
    """One row count at which the split stack kernel's group loop runs twice: launch_split_stack's ``resident``
    workgroups (two per CU while the double-buffered image fits twice, d <= 64; else one) of 128 rows, plus 129."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return (2 if dim <= 64 else 1) * cus * GROUP_ROWS + 129


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


_models = {}


def stack_model(amd, dim, n_layers, kernel="split"):
    key = (dim, n_layers, kernel)
    if key not in _models:
        model = build_ahf_stack(amd, c2_layers(dim, n_layers), dim)
        for f in model.flows:
            select_kernel(f, kernel)
        _models[key] = model
    return _models[key]


def whole_run(model):
    runs = model._affine_runs()
    assert list(runs) == [0] and len(runs[0].layers) == len(model.flows)
    return runs[0]


def launch(amd, run, x, inverse, mode, density, kernel):
    """One ``_AffineRun.launch``: storing (keep=True) or density-only.  ``mode`` "lp": the fused epilogue is asked for
    (with ``sqnorm`` as its fall-back, as ``_pass`` does); "sq": |z|^2 alone.  Outputs start as NaN: one that the
    launch did not write fails every comparison."""
    rows = x.shape[0]
    nan = lambda: torch.full((rows,), float("nan"), device=DEV)
    ld, sq, lp = nan(), nan(), nan()
    total = torch.zeros(1, dtype=torch.float64, device=DEV)
    outs = run.launch(x, inverse, ld, False, sq, keep=not density, logprob=(lp, total) if mode == "lp" else None,
                      density_only=density)
    assert outs is not None, "no stack kernel for this shape"
    assert amd.last_kernel() == ("ahf_split_stack" if kernel == "split" else "ahf_stack_fp32"), amd.last_kernel()
    if density:
        assert outs == [None]
    else:
        assert len(outs) == len(run.layers) and all(o.shape == x.shape for o in outs)
    fused = mode == "lp" and run.logprob_fused
    assert fused == (mode == "lp" and kernel == "split")
    return {"ld": ld, "lp": lp if fused else None, "sq": None if fused else sq, "total": total if fused else None}


def assert_same_launch(got, ref, what):
    for name in ("ld", "lp", "sq"):
        assert (got[name] is None) == (ref[name] is None), (what, name)
        if got[name] is not None:
            assert same_bits(got[name], ref[name]), f"{what}: {name} differs from the storing launch"
    if got["total"] is not None:
        want = float(got["lp"].double().sum())
        assert abs(float(got["total"]) - want) <= 1e-9 * abs(want), (what, float(got["total"]), want)


KERNEL_DIMS = [("split", d) for d in DIMS] + [("fp32", 64)]  # (fp32: the dims with an fp32 stack kernel)


@pytest.mark.parametrize("inverse", [True, False], ids=["inverse", "forward"])
@pytest.mark.parametrize("n_layers", [2, 3, 9])
@pytest.mark.parametrize("kernel,dim", KERNEL_DIMS, ids=[f"{k}-d{d}" for k, d in KERNEL_DIMS])
def test_launch_matches_storing_launch(amd, kernel, dim, n_layers, inverse):
    run = whole_run(stack_model(amd, dim, n_layers, kernel))
    counts = ROWS + ([rows_past_one_grid(dim)] if dim in (64, 256) and n_layers == 9 else [])
    x_all = cuda(recipes.gaussian(70 + dim, max(counts), dim))
    with torch.no_grad():
        for rows in counts:
            x = x_all[:rows].contiguous()
            for mode in ("lp", "sq"):
                ref = launch(amd, run, x, inverse, mode, False, kernel)
                got = launch(amd, run, x, inverse, mode, True, kernel)
                assert_same_launch(got, ref, f"{kernel} d={dim} L={n_layers} rows={rows} {mode}")


@pytest.mark.parametrize("kernel,dim", KERNEL_DIMS, ids=[f"{k}-d{d}" for k, d in KERNEL_DIMS])
def test_log_prob_matches_storing_pass(amd, kernel, dim):
    """``log_prob`` (density-only) against the same pass with every tensor kept (``_pass`` without ``last_only``)."""
    model = stack_model(amd, dim, 9, kernel)
    x = cuda(recipes.gaussian(90 + dim, 1013, dim))
    with torch.no_grad():
        lp_ref = torch.empty(x.shape[0], device=DEV)
        tot_ref = torch.zeros(1, dtype=torch.float64, device=DEV)
        zs, ld_ref = model._pass(x, True, want_sqnorm=True, want_logprob=(lp_ref, tot_ref))
        assert len(zs) == 10 and all(z is not None for z in zs)
        if kernel == "split":
            assert model._logprob_done
        else:  # the separate epilogue on (|z|^2, log_det), as log_prob runs it
            assert not model._logprob_done and model._last_sqnorm is not None
            amd._lib.check("mnf_gauss_logprob_sq", amd._lib.load().mnf_gauss_logprob_sq(
                model._last_sqnorm.data_ptr(), ld_ref.data_ptr(), lp_ref.data_ptr(), None, x.shape[0], dim,
                amd.flows._stream()))
        lp, total = model.log_prob(x, return_sum=True)
        assert model._logprob_done == (kernel == "split")
        lp_only = model.log_prob(x)
    assert same_bits(lp, lp_ref) and same_bits(lp_only, lp)
    want = float(lp.double().sum())
    assert abs(float(total) - want) <= 1e-9 * abs(want)


def _actnorm(amd, dim, seed):
    an = amd.ActNormFlow(dim).to(DEV)
    an.load_state_dict(recipes.actnorm_params(seed, dim))
    an.data_dep_init_done = True
    return an


def test_run_closes_the_pass_on_a_running_log_det(amd):
    """[AHF, AHF, AHF, ActNorm]: in inverse order the run is the LAST launch and adds to a non-zero log_det
    (accumulate = 1)."""
    dim = 64
    ahf = list(build_ahf_stack(amd, c2_layers(dim, 3), dim).flows)
    model = amd.NormalizingFlowModel(amd.StandardNormal(dim), ahf + [_actnorm(amd, dim, 810)]).to(DEV)
    x = cuda(recipes.gaussian(811, 1013, dim))
    with torch.no_grad():
        lp_ref = torch.empty(x.shape[0], device=DEV)
        tot_ref = torch.zeros(1, dtype=torch.float64, device=DEV)
        zs, _ = model._pass(x, True, want_sqnorm=True, want_logprob=(lp_ref, tot_ref))
        assert model._logprob_done and len(zs) == 5 and amd.last_kernel() == "ahf_split_stack"
        lp, total = model.log_prob(x, return_sum=True)
        assert model._logprob_done and amd.last_kernel() == "ahf_split_stack"
    assert same_bits(lp, lp_ref)
    assert abs(float(total) - float(lp.double().sum())) <= 1e-9 * abs(float(total))


def test_run_that_is_not_last_drops_only_its_intermediates(amd):
    """[ActNorm, AHF, AHF, AHF]: in inverse order the run comes first (keep=False, z kept for ActNorm)."""
    dim = 64
    ahf = list(build_ahf_stack(amd, c2_layers(dim, 3), dim).flows)
    model = amd.NormalizingFlowModel(amd.StandardNormal(dim), [_actnorm(amd, dim, 820)] + ahf).to(DEV)
    x = cuda(recipes.gaussian(821, 1013, dim))
    with torch.no_grad():
        zs, ld = model.inverse(x)
        assert len(zs) == 5
        lp_ref = torch.empty(x.shape[0], device=DEV)
        amd._lib.check("mnf_gauss_logprob", amd._lib.load().mnf_gauss_logprob(
            zs[-1].data_ptr(), ld.data_ptr(), lp_ref.data_ptr(), None, x.shape[0], dim, amd.flows._stream()))
        lp = model.log_prob(x)
        assert same_bits(lp, lp_ref)
        assert same_bits(model.base_log_prob(x), model.base.log_prob(zs[-1]))


class _OtherBase:
    """Not a StandardNormal: ``log_prob`` needs z itself."""

    def log_prob(self, z):
        return -z.abs().sum(1)


def test_other_base_keeps_z(amd):
    dim = 64
    flows = list(build_ahf_stack(amd, c2_layers(dim, 3), dim).flows)
    model = amd.NormalizingFlowModel(_OtherBase(), flows).to(DEV)
    x = cuda(recipes.gaussian(830, 129, dim))
    with torch.no_grad():
        zs, ld = model.inverse(x)
        assert same_bits(model.log_prob(x), ld + model.base.log_prob(zs[-1]))
        assert same_bits(model.base_log_prob(x), model.base.log_prob(zs[-1]))


@pytest.mark.parametrize("dim", [64, 256])
def test_range_guard(amd, dim):
    """Two rows scaled by 3e4 (their tiles are redone on the fp32 path inside the launch) and one row holding inf."""
    run = whole_run(stack_model(amd, dim, 9))
    x = recipes.gaussian(840 + dim, 1013, dim)
    x[77] *= 3e4
    x[400] *= 3e4
    x[613, 5] = float("inf")
    x = cuda(x)
    with torch.no_grad():
        for inverse in (True, False):
            ref = launch(amd, run, x, inverse, "lp", False, "split")
            got = launch(amd, run, x, inverse, "lp", True, "split")
            for name in ("ld", "lp"):
                assert same_bits(got[name], ref[name]), (dim, inverse, name)
            assert torch.equal(torch.isfinite(got["lp"]), torch.isfinite(ref["lp"]))
            assert not bool(torch.isfinite(got["lp"][613]))
            # (not a comparison of NaN with NaN: at most the three 16-row tiles touched above may be non-finite)
            assert int(torch.isfinite(got["lp"]).sum()) >= x.shape[0] - 3 * 16


def test_nothing_is_materialised(amd):
    dim, n_layers = 64, 9
    model = stack_model(amd, dim, n_layers)
    rows = rows_past_one_grid(dim)
    x = cuda(recipes.gaussian(850, rows, dim))
    plane = rows * dim * 4
    with torch.no_grad():
        model.log_prob(x[:128].contiguous(), return_sum=True)  # the operand images are packed here
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        lp, total = model.log_prob(x, return_sum=True)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
    assert model._logprob_done and lp.shape == (rows,)
    assert peak <= plane, f"log_prob allocated {peak} bytes: more than one ({rows}, {dim}) plane of {plane}"


def test_inverse_unaffected(amd):
    dim, n_layers = 64, 9
    x = cuda(recipes.gaussian(860, 1013, dim))
    model = build_ahf_stack(amd, c2_layers(dim, n_layers), dim)
    fresh = build_ahf_stack(amd, c2_layers(dim, n_layers), dim)
    with torch.no_grad():
        model.log_prob(x)
        zs, ld = model.inverse(x)
        zs_f, ld_f = fresh.inverse(x)
    assert len(zs) == len(zs_f) == n_layers + 1 and zs[0] is x
    for a, b in zip(zs, zs_f):
        assert same_bits(a, b)
    assert same_bits(ld, ld_f)


def test_graph_capture(amd):
    dim, rows = 2, 4096
    model = stack_model(amd, dim, 9)
    x = cuda(recipes.gaussian(870, rows, dim))
    with torch.no_grad():
        lp, total = model.log_prob(x, return_sum=True)
        assert model._logprob_done
    replay = model.graphed_log_prob(x)
    lp_g, total_g = replay(x)
    torch.cuda.synchronize()
    assert same_bits(lp_g, lp)
    assert abs(float(total_g) - float(lp.double().sum())) <= 1e-9 * abs(float(total))


def test_abi_rule_for_null_y(amd):
    """``y`` may be NULL exactly when ``intermediates`` is NULL, ``log_det`` is given and something consumes the rows
    inside the kernel; anything else is MNF_ERR_INVALID_ARG before a launch."""
    L = amd._lib
    dim, n, rows = 64, 3, 129
    run = whole_run(stack_model(amd, dim, n))
    x = cuda(recipes.gaussian(880, rows, dim))
    images, splits = run.images(x.device)
    assert images is not None and splits is not None
    f0 = run.layers[0]
    par = L.int_array([int(bool(f.parity)) for f in run.layers])
    mid = torch.empty((n - 1, rows, dim), device=DEV)
    ld, sq = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())

    def call(y, mids, log_det, sqn, split):
        rc = L.load().mnf_affine_half_stack(
            ptr(x), ptr(y), ptr(mids), ptr(log_det), ptr(sqn), None, None, 0, ptr(images), ptr(split), par, n, rows, dim,
            1, len(f0.h_sizes), f0._hid, amd.flows._stream())
        torch.cuda.synchronize()
        return rc

    for split in (splits, None):
        assert call(None, None, ld, None, split) == L.MNF_ERR_INVALID_ARG  # nothing consumes the rows
        assert call(None, mid, ld, sq, split) == L.MNF_ERR_INVALID_ARG
        assert call(None, None, None, sq, split) == L.MNF_ERR_INVALID_ARG
    y = torch.empty_like(x)
    for split, family in ((splits, "ahf_split_stack"), (None, "ahf_stack_fp32")):
        ld_ref, sq_ref = torch.empty_like(ld), torch.empty_like(sq)
        assert call(y, None, ld_ref, sq_ref, split) == L.MNF_OK
        ld.fill_(float("nan"))
        sq.fill_(float("nan"))
        assert call(None, None, ld, sq, split) == L.MNF_OK
        assert amd.last_kernel() == family
        assert same_bits(ld, ld_ref) and same_bits(sq, sq_ref)
