"""GPU tests of MNFConv2d's gradient kernels (``mnf_mnf_conv_bwd_weight`` / ``mnf_mnf_conv_bwd_input``, families
"mnf_conv_bwd_weight" / "mnf_conv_bwd_input"; the route behind ``_dispatch.MNF_CONV_BWD_FUSED``): a shape matrix at the C
entries against aten's convolution_backward on the CPU in float32 / float64, the same matrix on small integers (exact),
the route through the layer on fixture G13 against autograd through the float64 oracle, and hipGraph capture."""
import numpy as np
import pytest
import torch

import recipes
from helpers import assert_parity, normwise_err
from test_hip_mnf_conv_fwd import GBASE, conv_layer, g13_forward, oracle_grads, shape_case
from test_oracle_golden import G13_CASES

pytestmark = pytest.mark.gpu
DEV = "cuda"
W_FAMILY, X_FAMILY = "mnf_conv_bwd_weight", "mnf_conv_bwd_input"
GUARD = 1024  # floats on either side of each output and of the workspace, which must come back untouched
NAMES = ("grad_x", "grad_Wz", "grad_W_var", "grad_b_var")

# (n_in, n_out, k, batch, H, W): each the smallest that reaches one branch
SHAPES = [
    (3, 1, 1, 1, 1, 1),       # one pixel, fewer pixels than slices, k = 1: no border
    (1, 17, 3, 1, 9, 9),      # 81 input pixels: the last tile is one pixel; a ragged channel tile
    (2, 64, 3, 2, 6, 11),     # non-square, four full output-channel tiles, tiles straddle rows and images
    (1, 20, 7, 1, 7, 7),      # kernel = image: every input pixel has exactly one term
    (64, 8, 5, 1, 5, 6),      # four full input-channel tiles in the input kernel, K = 1,600
    (5, 64, 8, 1, 8, 9),      # K' = 4,096: the input envelope's edge
    (83, 64, 7, 1, 7, 8),     # K = 4,067: the weight entry runs, the input entry refuses
    (1, 20, 5, 64, 28, 28),   # 36,864 output and 50,176 input pixels: many slices, the persistent loops wrap
    (20, 50, 5, 3, 12, 12),   # LeNet's second layer
]
IDS = ["x".join(map(str, s)) for s in SHAPES]


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


@pytest.fixture
def both(amd, monkeypatch):
    monkeypatch.setattr(amd._dispatch, "MNF_CONV_FUSED", True)
    monkeypatch.setattr(amd._dispatch, "MNF_CONV_BWD_FUSED", True)


def gaussian_case(shape):
    """The forward tests' operands for the shape, g standard normal and gv 30 x standard normal."""
    n_in, n_out, k, batch, H, W = shape
    c = shape_case(shape)
    seed = 9100 + 7 * n_in + 3 * n_out + k + batch
    o = c["eps"].shape
    return dict(x=c["x"], Wz=c["W_mean"] * c["z"].view(-1, 1, 1, 1), W_var=c["W_log_var"].exp(),
                g=recipes.gaussian(seed + 6, batch, o[1] * o[2] * o[3]).reshape(o),
                gv=30 * recipes.gaussian(seed + 7, batch, o[1] * o[2] * o[3]).reshape(o))


def integer_case(shape):
    """Every operand an integer in -2 .. 2, stored as float32: every partial sum is an integer below 2^24."""
    n_in, n_out, k, batch, H, W = shape
    gen = torch.Generator().manual_seed(4400 + 7 * n_in + 3 * n_out + k + batch)
    draw = lambda *s: torch.randint(-2, 3, s, generator=gen).float()  # noqa: E731
    o = (batch, n_out, H - k + 1, W - k + 1)
    return dict(x=draw(batch, n_in, H, W), Wz=draw(n_out, n_in, k, k), W_var=draw(n_out, n_in, k, k), g=draw(*o), gv=draw(*o))


def reference(c, dt):
    """aten.convolution_backward on the CPU, composed as _MnfConvFwdFn.backward composes it."""
    p = {k_: v.to(dt) for k_, v in c.items()}
    conv_bwd = torch.ops.aten.convolution_backward
    geometry = ([p["Wz"].shape[0]], [1, 1], [0, 0], [1, 1], False, [0, 0], 1)
    gx, g_wz, _ = conv_bwd(p["g"], p["x"], p["Wz"], *geometry, [True, True, False])
    gx2, g_wv, g_bv = conv_bwd(p["gv"], p["x"] * p["x"], p["W_var"], *geometry, [True, True, True])
    return dict(grad_x=gx + 2 * p["x"] * gx2, grad_Wz=g_wz, grad_W_var=g_wv, grad_b_var=g_bv)


def guarded(n):
    buf = torch.full((n + 2 * GUARD,), float("nan"), device=DEV)
    return buf, buf[GUARD:GUARD + n]


def run_entries(amd, c):
    """Both C entries on a case's float32 operands, every output and the workspace pre-filled with NaN between NaN guard
    bands: {name: host tensor} (without grad_x where the input entry does not have the shape)."""
    lib = amd._lib.load()
    d = {k_: v.to(DEV).contiguous() for k_, v in c.items()}
    batch, n_in, H, W = d["x"].shape
    n_out, k = d["Wz"].shape[0], d["Wz"].shape[-1]
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.mnf_mnf_conv_bwd_weight_supported(n_in, n_out, k, H, W) == 1
    n_ws = lib.mnf_mnf_conv_bwd_weight_workspace(batch, n_in, n_out, k, H, W)
    assert 0 < n_ws <= 8 * 2 ** 20
    bufs, out = {}, {}
    for name, n in (("grad_Wz", d["Wz"].numel()), ("grad_W_var", d["Wz"].numel()), ("grad_b_var", n_out), ("workspace", n_ws)):
        bufs[name], out[name] = guarded(n)
    rc = lib.mnf_mnf_conv_bwd_weight(d["x"].data_ptr(), d["g"].data_ptr(), d["gv"].data_ptr(), out["grad_Wz"].data_ptr(),
                                     out["grad_W_var"].data_ptr(), out["grad_b_var"].data_ptr(), out["workspace"].data_ptr(),
                                     n_ws, batch, n_in, H, W, n_out, k, stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert amd.last_kernel() == W_FAMILY
    if lib.mnf_mnf_conv_bwd_input_supported(n_in, n_out, k, H, W):
        bufs["grad_x"], out["grad_x"] = guarded(d["x"].numel())
        rc = lib.mnf_mnf_conv_bwd_input(d["x"].data_ptr(), d["g"].data_ptr(), d["gv"].data_ptr(), d["Wz"].data_ptr(),
                                        d["W_var"].data_ptr(), out["grad_x"].data_ptr(), batch, n_in, H, W, n_out, k, stream)
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert amd.last_kernel() == X_FAMILY
    for name, b in bufs.items():
        n = out[name].numel()
        assert bool(torch.isnan(torch.cat([b[:GUARD], b[GUARD + n:]])).all()), f"a launch wrote outside {name}"
    out.pop("workspace")
    shapes = dict(grad_x=d["x"].shape, grad_Wz=d["Wz"].shape, grad_W_var=d["Wz"].shape, grad_b_var=(n_out,))
    res = {name: t.cpu().reshape(shapes[name]) for name, t in out.items()}
    for name, t in res.items():
        assert bool(torch.isfinite(t).all()), f"{name} is not finite"
    return res


# ------------------------------------------------------------------ the C entries, shape by shape
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_entries_shape_matrix_vs_aten(amd, shape):
    """Each gradient within the project's 1e-5 normwise plus twice the reference's own fp32-fp64 distance (at most 4.7e-6
    for these operands, on grad_b_var of the 36,864-pixel case: the 5e-5 cap is met by the reference alone); a second call
    is bit for bit the first."""
    c = gaussian_case(shape)
    lib = amd._lib.load()
    n_in, n_out, k, _, H, W = shape
    has_x = lib.mnf_mnf_conv_bwd_input_supported(n_in, n_out, k, H, W) == 1
    assert has_x == (n_in <= 64)
    ref32, ref64 = reference(c, torch.float32), reference(c, torch.float64)
    got = run_entries(amd, c)
    assert ("grad_x" in got) == has_x
    for name in NAMES:
        if name in got:
            err = assert_parity(got[name], ref32[name].numpy(), ref64[name].numpy(), what=f"mnf_mnf_conv_bwd {shape} {name}")
            print(f"{shape} {name}: {err:.3e}")
    again = run_entries(amd, c)
    for name, t in got.items():
        assert torch.equal(t, again[name]), f"{name} does not repeat bit for bit"


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_entries_on_small_integers_are_exact(amd, shape):
    """Operands in -2 .. 2: every partial sum is an integer below 2^24 (at most 8 x 36,864 in the weight kernel, 2 * 2 * 4 *
    4,096 in the input kernel), so every output EQUALS the float64 reference whatever the order of the sums -- a pixel
    dropped or counted twice at a tile, slice or image boundary, or a border term that was not zeroed, shows here."""
    c = integer_case(shape)
    ref = reference(c, torch.float64)
    got = run_entries(amd, c)
    for name, t in got.items():
        wrong = int((t.double() != ref[name]).sum())
        assert wrong == 0, f"{shape} {name}: {wrong} of {t.numel()} elements differ from the exact result"


# ------------------------------------------------------------------ through the layer
def spy_on(amd, monkeypatch):
    """Both entries wrapped on the library object: calls[name] = the kernel family right after each call."""
    lib, calls = amd._lib.load(), {"mnf_mnf_conv_bwd_weight": [], "mnf_mnf_conv_bwd_input": []}
    for name in calls:
        real = getattr(lib, name)

        def spy(*a, _real=real, _name=name):
            rc = _real(*a)
            calls[_name].append(amd.last_kernel())
            return rc

        monkeypatch.setattr(lib, name, spy)
    return calls


@pytest.mark.parametrize("tag", ["c1", "c2"])
def test_layer_gradients_on_the_fused_backward_vs_float64_oracle(amd, O, golden, both, monkeypatch, tag):
    """The procedure and budget of test_fused_route_gradients_vs_float64_oracle with both switches on: every parameter the
    output depends on (plus x for c2) against autograd through the float64 oracle, within 1e-5 + twice the float32 oracle's
    own distance; c1's input needs no gradient, so the input entry is never called; a FlatParameters home receives the same
    gradients within 2e-6."""
    fx = golden("g13_mnf_conv2d")
    shape = fx[f"{tag}.y"].shape
    w_out = recipes.gaussian(7700 + G13_CASES[tag][1], shape[0], int(np.prod(shape[1:]))).reshape(shape)
    ref = oracle_grads(O, fx, tag, w_out)
    calls = spy_on(amd, monkeypatch)

    def run(homed):
        layer = conv_layer(amd, fx, tag)
        flat = amd.FlatParameters(layer) if homed else None
        x = torch.from_numpy(fx[f"{tag}.x"]).to(DEV).requires_grad_(tag == "c2")
        y = g13_forward(layer, fx, tag, x)
        assert amd.last_kernel() == "mnf_conv_fwd"
        for v in calls.values():
            v.clear()
        (y * w_out.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        assert calls["mnf_mnf_conv_bwd_weight"] == [W_FAMILY]
        assert calls["mnf_mnf_conv_bwd_input"] == ([X_FAMILY] if tag == "c2" else [])
        got = {n: (p.grad.detach().cpu().double() if p.grad is not None else None) for n, p in layer.named_parameters()}
        if x.grad is not None:
            got["x"] = x.grad.detach().cpu().double()
        return got, flat

    got, _ = run(False)
    assert ("x" in got) == (tag == "c2")
    for name, r64 in ref[torch.float64].items():
        r = r64.numpy()
        g = got[name]
        if not np.any(r):
            assert g is None or not np.any(g.numpy()), name
            continue
        widen = 2 * normwise_err(ref[torch.float32][name].double().numpy(), r)
        err = normwise_err(g.numpy().reshape(r.shape), r)
        print(f"{tag} grad {name}: {err:.3e} (budget {GBASE + widen:.3e})")
        assert err <= GBASE + widen, f"MNFConv2d backward (fused) {tag} grad {name}: {err:.2e} > 1e-5 + {widen:.2e}"
    homed, flat = run(True)
    for name, g in got.items():
        if g is not None and homed[name] is not None and float(g.abs().max()) > 0:
            assert normwise_err(homed[name].numpy(), g.numpy()) <= 2e-6, name
    assert all(p.grad is v for p, v in zip(flat.params, flat._grad_views))


def unsupported_input_run(amd, monkeypatch, bwd_switch):
    torch.manual_seed(6)
    layer = amd.MNFConv2d(65, 8, 3).to(DEV)
    monkeypatch.setattr(amd._dispatch, "MNF_CONV_FUSED", True)
    monkeypatch.setattr(amd._dispatch, "MNF_CONV_BWD_FUSED", bwd_switch)
    x = recipes.gaussian(41, 2, 65 * 25).reshape(2, 65, 5, 5).to(DEV).requires_grad_(True)
    eps = recipes.gaussian(42, 2, 8 * 9).reshape(2, 8, 3, 3).to(DEV)
    eps_z = recipes.gaussian(43, 1, 8).reshape(8).to(DEV)
    masks = [recipes.bernoulli_mask(44 + i, 1, 8).to(DEV) for i in range(len(layer.flow_q.flows))]
    y = layer.forward(x, eps=eps, eps_z=eps_z, masks=masks)
    assert amd.last_kernel() == "mnf_conv_fwd"
    (y * recipes.gaussian(45, 2, 72).reshape(2, 8, 3, 3).to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return x.grad.clone(), layer.W_mean.grad.clone()


def test_unsupported_input_part_runs_the_route_of_today(amd, monkeypatch):
    """65 input channels: the input entry refuses the shape, so x.grad is what the switch-off route computes, bit for bit;
    the weight family still runs."""
    lib = amd._lib.load()
    assert lib.mnf_mnf_conv_bwd_input_supported(65, 8, 3, 5, 5) == 0 and lib.mnf_mnf_conv_bwd_weight_supported(65, 8, 3, 5, 5) == 1
    calls = spy_on(amd, monkeypatch)
    gx_off, gw_off = unsupported_input_run(amd, monkeypatch, False)
    assert calls == {"mnf_mnf_conv_bwd_weight": [], "mnf_mnf_conv_bwd_input": []}
    gx_on, gw_on = unsupported_input_run(amd, monkeypatch, True)
    assert calls == {"mnf_mnf_conv_bwd_weight": [W_FAMILY], "mnf_mnf_conv_bwd_input": []}
    assert torch.equal(gx_on, gx_off)
    assert normwise_err(gw_on.cpu().numpy(), gw_off.cpu().numpy()) <= 2e-5  # (two correct fp32 routes)


def test_switch_off_never_reaches_the_entries(amd, golden, monkeypatch):
    fx = golden("g13_mnf_conv2d")
    assert amd._dispatch.MNF_CONV_BWD_FUSED is False
    monkeypatch.setattr(amd._dispatch, "MNF_CONV_FUSED", True)
    calls = spy_on(amd, monkeypatch)
    layer = conv_layer(amd, fx, "c2")
    x = torch.from_numpy(fx["c2.x"]).to(DEV).requires_grad_(True)
    g13_forward(layer, fx, "c2", x).sum().backward()
    torch.cuda.synchronize()
    assert calls == {"mnf_mnf_conv_bwd_weight": [], "mnf_mnf_conv_bwd_input": []}
    assert x.grad is not None and layer.W_mean.grad is not None


# ------------------------------------------------------------------ capture
def test_entries_in_a_hipgraph_replay_the_eager_result(amd):
    """Both entries on preallocated buffers inside torch.cuda.graph on a side stream: after the outputs are filled with NaN,
    a replay gives the eager results bit for bit."""
    lib = amd._lib.load()
    shape = (20, 50, 5, 3, 12, 12)
    n_in, n_out, k, batch, H, W = shape
    d = {k_: v.to(DEV).contiguous() for k_, v in gaussian_case(shape).items()}
    n = d["Wz"].numel()
    n_ws = lib.mnf_mnf_conv_bwd_weight_workspace(batch, n_in, n_out, k, H, W)
    work = torch.empty(n_ws, device=DEV)
    packed, gx = torch.empty(2 * n + n_out, device=DEV), torch.empty_like(d["x"])

    def launch():
        stream = torch.cuda.current_stream().cuda_stream
        rc = lib.mnf_mnf_conv_bwd_weight(d["x"].data_ptr(), d["g"].data_ptr(), d["gv"].data_ptr(), packed.data_ptr(),
                                         packed.data_ptr() + 4 * n, packed.data_ptr() + 8 * n, work.data_ptr(), n_ws, batch,
                                         n_in, H, W, n_out, k, stream)
        assert rc == 0, rc
        rc = lib.mnf_mnf_conv_bwd_input(d["x"].data_ptr(), d["g"].data_ptr(), d["gv"].data_ptr(), d["Wz"].data_ptr(),
                                        d["W_var"].data_ptr(), gx.data_ptr(), batch, n_in, H, W, n_out, k, stream)
        assert rc == 0, rc

    launch()
    torch.cuda.synchronize()
    eager = packed.clone(), gx.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up off the default stream, as capture requires
        launch()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    packed.fill_(float("nan"))
    gx.fill_(float("nan"))
    work.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(packed, eager[0]) and torch.equal(gx, eager[1])
    # the packed outputs (one zeroing, one reduction) are the separate outputs' values
    sep = run_entries(amd, {k_: v.cpu() for k_, v in d.items()})
    assert torch.equal(packed[:n].cpu().view_as(sep["grad_Wz"]), sep["grad_Wz"])
    assert torch.equal(packed[n:2 * n].cpu().view_as(sep["grad_W_var"]), sep["grad_W_var"])
    assert torch.equal(packed[2 * n:].cpu(), sep["grad_b_var"])
