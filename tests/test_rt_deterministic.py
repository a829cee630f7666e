"""The run-time-shaped gradient launches with fixed-order parameter sums (include/mnf_hip.h mnf_*_bwd_rt_det).

In process (default mode): the _det entries through ctypes repeat bit for bit, stay within parity of the atomic entries
(the two differ in summation order only) and ADD to grad_flat.  In a child process under MNF_DETERMINISTIC=1
(tests/rt_deterministic_child.py, run by path): the layers land on the *_bwd_rt kernels and match the float64 oracle,
rt-only training repeats bit for bit (tools/soak_determinism_rt.py), a graphed training step replays identically, and a
gradient pass on an atomic VALU kernel warns once."""
import os
import subprocess
import sys

import pytest
import torch

from helpers import assert_parity

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"


@pytest.fixture(scope="module")
def amd():
    import torch_mnf_amd

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch_mnf_amd


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _flat(f):
    return torch.cat([p.detach().reshape(-1) for p in f.parameters()]).contiguous()


def _setup(amd, kind, rows):
    """(call(grad_x, grad_flat, det, workspace) -> rc, grad_x, flat, workspace floats) for one layer at `rows` rows"""
    from torch_mnf_amd import _lib
    from torch_mnf_amd.flows import _grad_scale

    lib = _lib.load()
    g = torch.Generator(device=DEV).manual_seed(rows + len(kind))
    if kind == "ahf":
        f = amd.AffineHalfFlow(64, parity=True, h_sizes=(24, 24)).to(DEV)
        hid, dim = (24, 24), 64
    elif kind == "nsf":
        f = amd.NSF_CL(128, K=8, B=3, n_h=32).to(DEV)
        hid, dim = (32, 32, 32), 128
    else:
        f = amd.RNVP(800, h_sizes=(100,)).to(DEV)
        hid, dim = (100,), 800
    flat = _flat(f)
    h = _lib.int_array(hid)
    x = torch.randn(rows, dim, device=DEV, generator=g)
    gy = torch.randn(rows, dim, device=DEV, generator=g) / rows
    gl = torch.randn(rows, device=DEV, generator=g) / rows
    sc = _grad_scale(gy, gl, rows, dim, x.device)
    if kind == "ahf":
        n_ws = lib.mnf_affine_half_bwd_rt_det_workspace(rows, dim, 2, h, 1, 1)

        def call(gx, gf, det, ws):
            a = (x.data_ptr(), None, gy.data_ptr(), gl.data_ptr(), gx.data_ptr(), gf.data_ptr(), flat.data_ptr(), sc.data_ptr(),
                 rows, dim, 1, 0, 2, h, 1, 1)
            if det:
                return lib.mnf_affine_half_bwd_rt_det(*a, ws.data_ptr(), ws.numel(), _stream())
            return lib.mnf_affine_half_bwd_rt(*a, _stream())
    elif kind == "nsf":
        with torch.no_grad():
            y, _ = f.forward(x)
        n_ws = lib.mnf_nsf_cl_bwd_rt_det_workspace(rows, dim, 8, 3, h)

        def call(gx, gf, det, ws):
            a = (x.data_ptr(), y.data_ptr(), gy.data_ptr(), gl.data_ptr(), gx.data_ptr(), gf.data_ptr(), flat.data_ptr(),
                 sc.data_ptr(), rows, dim, 8, 3.0, 0, 3, h)
            if det:
                return lib.mnf_nsf_cl_bwd_rt_det(*a, ws.data_ptr(), ws.numel(), _stream())
            return lib.mnf_nsf_cl_bwd_rt(*a, _stream())
    else:
        n_ws = lib.mnf_rnvp_bwd_rt_det_workspace(rows, dim, 1, h)

        def call(gx, gf, det, ws):
            a = (x.data_ptr(), None, 17, gy.data_ptr(), gl.data_ptr(), gx.data_ptr(), gf.data_ptr(), flat.data_ptr(),
                 sc.data_ptr(), rows, dim, 1, h)
            if det:
                return lib.mnf_rnvp_bwd_rt_det(*a, ws.data_ptr(), ws.numel(), _stream())
            return lib.mnf_rnvp_bwd_rt(*a, _stream())
    return call, x, flat, n_ws


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ahf", "nsf", "rnvp"])
@pytest.mark.parametrize("rows", [262144, 4096 + 37, 2049])
def test_det_entries_repeat_bit_for_bit_and_match_the_atomic_ones(amd, kind, rows):
    from torch_mnf_amd import _lib

    call, x, flat, n_ws = _setup(amd, kind, rows)
    assert n_ws > 0 and n_ws * 4 <= (512 << 20), n_ws
    ws = torch.empty(n_ws, dtype=torch.float32, device=DEV)
    runs = []
    for _ in range(5):
        gx, gf = torch.empty_like(x), torch.zeros_like(flat)
        assert call(gx, gf, True, ws) == _lib.MNF_OK
        assert amd.last_kernel() == f"{kind}_bwd_rt"
        runs.append((gx, gf))
    torch.cuda.synchronize()
    for gx, gf in runs[1:]:
        assert torch.equal(gx, runs[0][0]) and torch.equal(gf, runs[0][1])
    assert bool(torch.isfinite(runs[0][1]).all()) and float(runs[0][1].abs().max()) > 0
    # against the atomic entry (default mode): the same products, another summation order
    if not amd.deterministic():
        gx_a, gf_a = torch.empty_like(x), torch.zeros_like(flat)
        assert call(gx_a, gf_a, False, None) == _lib.MNF_OK
        torch.cuda.synchronize()
        assert_parity(runs[0][1].cpu().numpy(), gf_a.cpu().numpy(), what=f"{kind}_bwd_rt_det grad_flat vs atomic, {rows} rows")
        assert_parity(runs[0][0].cpu().numpy(), gx_a.cpu().numpy(), what=f"{kind}_bwd_rt_det grad_x vs atomic, {rows} rows")
    # grad_flat is ADDED to: two calls into one buffer give exactly twice one call
    gx, gf = torch.empty_like(x), torch.zeros_like(flat)
    assert call(gx, gf, True, ws) == _lib.MNF_OK
    assert call(gx, gf, True, ws) == _lib.MNF_OK
    torch.cuda.synchronize()
    assert torch.equal(gf, 2 * runs[0][1])
    # a workspace one float short is refused before anything runs
    assert call(gx, gf, True, ws[:n_ws - 1]) == _lib.MNF_ERR_INVALID_ARG


@pytest.mark.gpu
def test_deterministic_mode_covers_the_run_time_shaped_gradient_shapes():
    env = dict(os.environ, MNF_DETERMINISTIC="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "rt_deterministic_child.py")], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=1500)
    tail = "\n".join((p.stdout + p.stderr).splitlines()[-30:])
    assert p.returncode == 0, tail
    assert "rt deterministic child ok" in p.stdout, tail


@pytest.mark.gpu
def test_rt_only_training_repeats_bit_for_bit_in_deterministic_mode():
    env = dict(os.environ, MNF_DETERMINISTIC="1")
    p = subprocess.run([sys.executable, "tools/soak_determinism_rt.py", "6", "65536"], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=900)
    lines = [ln for ln in p.stdout.splitlines() if "Adam steps twice" in ln]
    assert len(lines) == 3, p.stdout + p.stderr
    for ln, family in zip(lines, ("ahf_bwd_rt", "nsf_bwd_rt", "rnvp_bwd_rt")):
        assert " 0 of " in ln and "MNF_DETERMINISTIC=1" in ln and family in ln, ln
    assert p.returncode == 0, p.stdout + p.stderr
