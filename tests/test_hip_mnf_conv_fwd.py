"""GPU tests of MNFConv2d.forward as ONE matrix-core launch (``mnf_mnf_conv_fwd``, kernel family "mnf_conv_fwd"; the route
behind ``_dispatch.MNF_CONV_FUSED``): the reference's own outputs (fixture G13), a shape matrix at the C entry against the
float32 / float64 oracle, gradients against autograd through the float64 oracle, and the route's plumbing (non-contiguous
input, unsupported shapes, repeatability, hipGraph capture)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import recipes
from helpers import RTOL, assert_close, assert_parity, normwise_err
from test_oracle_golden import G13_CASES, G13_KEYS, g13_specs

pytestmark = pytest.mark.gpu
DEV = "cuda"
FAMILY = "mnf_conv_fwd"
# gradient bar (tests/test_hip_kl.py): 1e-5 normwise + twice the fp32-vs-fp64 distance of the oracle
GBASE = 1e-5


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
def fused(amd, monkeypatch):
    monkeypatch.setattr(amd._dispatch, "MNF_CONV_FUSED", True)


def conv_layer(amd, fx, tag):
    n_in, n_out, k, seed = G13_CASES[tag]
    layer = amd.MNFConv2d(n_in, n_out, k)
    layer.load_state_dict({k_: torch.from_numpy(fx[f"{tag}.{k_}"]) for k_ in G13_KEYS}, strict=False)
    for which, flow in (("q", layer.flow_q), ("r", layer.flow_r)):
        for i, f in enumerate(flow.flows):
            f.load_state_dict(recipes.rnvp_params(1300 + seed + 10 * (which == "r") + i, n_out, 50))
    return layer.to(DEV)


def g13_inputs(fx, tag):
    """Fixture G13's input and captured draws of ``forward``, on the device."""
    dev = lambda name: torch.from_numpy(fx[f"{tag}.{name}"]).to(DEV)  # noqa: E731
    return dict(x=dev("x"), eps=dev("fwd.eps_out"), eps_z=dev("fwd.eps_z"), masks=list(dev("fwd.masks")))


def g13_forward(layer, fx, tag, x=None, inputs=None):
    inp = dict(inputs or g13_inputs(fx, tag))
    if x is not None:
        inp["x"] = x
    return layer.forward(inp.pop("x"), **inp)


# ------------------------------------------------------------------ the reference's own outputs
@pytest.mark.parametrize("tag", ["c1", "c2"])
def test_g13_forward_on_the_fused_route_vs_reference(amd, golden, fused, tag):
    """Fixture G13 through layer.forward with every draw injected, switch on: the budget the MIOpen route is held to
    (test_g13_mnf_conv2d_vs_reference).  c1: K = 25 (no multiple of 4), 20 channels (a ragged second channel tile), 8-wide
    output rows (every 16-pixel tile straddles a row); c2: K = 500 (several weight chunks), 50 channels, 32 pixels."""
    fx = golden("g13_mnf_conv2d")
    layer = conv_layer(amd, fx, tag)
    with torch.no_grad():
        y = g13_forward(layer, fx, tag)
    assert amd.last_kernel() == FAMILY
    err = assert_close(y, fx[f"{tag}.y"], RTOL, f"MNFConv2d.forward ({FAMILY}) {tag} vs the reference")
    print(f"{tag}: normwise error {err:.3e}")


# ------------------------------------------------------------------ the C entry, shape by shape
# (n_in, n_out, k, batch, H, W): each the smallest that reaches one branch
SHAPES = [
    (3, 1, 1, 1, 1, 1),       # one pixel, K = 3 < 4, one channel
    (1, 17, 3, 1, 9, 9),      # 49 pixels: the last tile is one pixel; 7-wide rows
    (2, 64, 3, 2, 6, 11),     # non-square input, all four channel tiles full
    (1, 20, 7, 1, 7, 7),      # kernel = image: one pixel per image
    (64, 8, 5, 1, 5, 6),      # K = 1,600
    (83, 64, 7, 1, 7, 8),     # K = 4,067: the envelope's edge
    (1, 20, 5, 64, 28, 28),   # 36,864 pixels: the persistent loop wraps, images straddle tiles
]


def shape_case(shape):
    n_in, n_out, k, batch, H, W = shape
    seed = 9100 + 7 * n_in + 3 * n_out + k + batch
    per = n_in * k * k
    oh, ow = H - k + 1, W - k + 1
    return dict(
        x=recipes.gaussian(seed, batch, n_in * H * W).reshape(batch, n_in, H, W),
        W_mean=(0.1 * recipes.gaussian(seed + 1, n_out, per)).reshape(n_out, n_in, k, k),
        W_log_var=(-9 + 0.1 * recipes.gaussian(seed + 2, n_out, per)).reshape(n_out, n_in, k, k),  # as the layer initialises it
        b_log_var=(-9 + 0.1 * recipes.gaussian(seed + 3, 1, n_out)).reshape(n_out),
        z=(1 + 0.1 * recipes.gaussian(seed + 4, 1, n_out)).reshape(n_out),
        eps=recipes.gaussian(seed + 5, batch, n_out * oh * ow).reshape(batch, n_out, oh, ow))


GUARD = 1024  # floats on either side of each output, which must come back untouched


def run_entry(amd, c, want_var):
    """One mnf_mnf_conv_fwd call on a case's float32 operands: (out, var_out or None), both on the host."""
    lib = amd._lib.load()
    x = c["x"].to(DEV)
    Wz = (c["W_mean"] * c["z"].view(-1, 1, 1, 1)).to(DEV)
    Wv, bv = c["W_log_var"].exp().to(DEV), c["b_log_var"].exp().to(DEV)
    bm = torch.zeros(Wz.shape[0], device=DEV)
    eps = c["eps"].to(DEV)
    n = eps.numel()
    bufs = [torch.full((n + 2 * GUARD,), float("nan"), device=DEV) for _ in range(2 if want_var else 1)]
    out = bufs[0][GUARD:GUARD + n]
    var = bufs[1][GUARD:GUARD + n] if want_var else None
    batch, n_in, H, W = x.shape
    rc = lib.mnf_mnf_conv_fwd(x.data_ptr(), Wz.data_ptr(), Wv.data_ptr(), bm.data_ptr(), bv.data_ptr(), eps.data_ptr(),
                              out.data_ptr(), None if var is None else var.data_ptr(), batch, n_in, H, W, Wz.shape[0],
                              Wz.shape[-1], torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert amd.last_kernel() == FAMILY
    for b in bufs:
        edge = torch.cat([b[:GUARD], b[GUARD + n:]])
        assert bool(torch.isnan(edge).all()), "the launch wrote outside its output"
    return out.cpu().reshape(eps.shape), None if var is None else var.cpu().reshape(eps.shape)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_entry_shape_matrix_vs_oracle(amd, O, shape):
    c = shape_case(shape)
    n_in, n_out, k = shape[:3]
    assert amd._lib.load().mnf_mnf_conv_fwd_supported(n_in, n_out, k, shape[4], shape[5]) == 1
    ref, ref_var = {}, {}
    for dt in (torch.float32, torch.float64):
        p = {k_: v.to(dt) for k_, v in c.items()}
        ref[dt] = O.mnf_conv2d_forward(p["x"], p["z"], p["W_mean"], p["W_log_var"], p["b_log_var"], p["eps"]).numpy()
        ref_var[dt] = F.conv2d(p["x"] ** 2, weight=p["W_log_var"].exp(), bias=p["b_log_var"].exp()).numpy()  # (mnf_conv.py:84)
    out, var = run_entry(amd, c, True)
    what = f"mnf_mnf_conv_fwd {shape}"
    e1 = assert_parity(out, ref[torch.float32], ref[torch.float64], what=what + " out")
    e2 = assert_parity(var, ref_var[torch.float32], ref_var[torch.float64], what=what + " var_out")
    print(f"{shape}: out {e1:.3e}, var_out {e2:.3e}")
    lean, none = run_entry(amd, c, False)
    assert none is None and torch.equal(lean, out), "the result depends on whether var_out is asked for"


def test_entry_repeats_bit_for_bit(amd):
    c = shape_case((2, 64, 3, 2, 6, 11))
    a, av = run_entry(amd, c, True)
    b, bv = run_entry(amd, c, True)
    assert torch.equal(a, b) and torch.equal(av, bv)


# ------------------------------------------------------------------ the route's plumbing
def test_non_contiguous_input_gives_the_contiguous_result(amd, golden, fused):
    fx = golden("g13_mnf_conv2d")
    layer = conv_layer(amd, fx, "c2")
    x = torch.from_numpy(fx["c2.x"]).to(DEV)
    view = x.transpose(2, 3).contiguous().transpose(2, 3)  # the same numbers, strides of the transposed layout
    assert not view.is_contiguous() and torch.equal(view, x)
    with torch.no_grad():
        a = g13_forward(layer, fx, "c2", x)
        b = g13_forward(layer, fx, "c2", view)
    assert amd.last_kernel() == FAMILY
    assert torch.equal(a, b)


def test_unsupported_shape_runs_the_route_of_today(amd, monkeypatch):
    """65 output channels are outside the kernel's envelope: with the switch on the layer runs what it runs with the
    switch off, bit for bit on injected draws."""
    torch.manual_seed(5)
    layer = amd.MNFConv2d(1, 65, 3).to(DEV)
    assert amd._lib.load().mnf_mnf_conv_fwd_supported(1, 65, 3, 9, 9) == 0
    x = recipes.gaussian(31, 2, 81).reshape(2, 1, 9, 9).to(DEV)
    eps = recipes.gaussian(32, 2, 65 * 49).reshape(2, 65, 7, 7).to(DEV)
    eps_z = recipes.gaussian(33, 1, 65).reshape(65).to(DEV)
    masks = [recipes.bernoulli_mask(34 + i, 1, 65).to(DEV) for i in range(len(layer.flow_q.flows))]
    outs = []
    for switch in (False, True):
        monkeypatch.setattr(amd._dispatch, "MNF_CONV_FUSED", switch)
        with torch.no_grad():
            outs.append(layer.forward(x, eps=eps, eps_z=eps_z, masks=masks))
        assert amd.last_kernel() != FAMILY
    assert torch.equal(outs[0], outs[1])


def test_float64_input_raises_as_on_the_shipped_route(amd, golden, monkeypatch):
    fx = golden("g13_mnf_conv2d")
    layer = conv_layer(amd, fx, "c1")
    lib, calls = amd._lib.load(), []
    monkeypatch.setattr(lib, "mnf_mnf_conv_fwd", lambda *a: calls.append(a) or 0)
    x = torch.from_numpy(fx["c1.x"]).to(DEV)
    errors = []
    for switch in (False, True):
        monkeypatch.setattr(amd._dispatch, "MNF_CONV_FUSED", switch)
        for bad in (x.double(), x.half(), x.cpu()):
            with pytest.raises(RuntimeError) as info, torch.no_grad():
                g13_forward(layer, fx, "c1", bad)
            errors.append(str(info.value))
            assert layer._fused_forward_has(bad) is False
    assert errors[:3] == errors[3:] and calls == []


def test_no_grad_forward_of_an_input_that_requires_grad_keeps_nothing(amd, golden, fused, monkeypatch):
    """Under no_grad the launch gets no var_out and the result carries no graph, whatever x.requires_grad says; with
    gradients wanted it gets one -- and the values are the same."""
    fx = golden("g13_mnf_conv2d")
    layer = conv_layer(amd, fx, "c2")
    lib = amd._lib.load()
    real, var_args = lib.mnf_mnf_conv_fwd, []

    def spy(*a):
        var_args.append(a[7])
        return real(*a)

    monkeypatch.setattr(lib, "mnf_mnf_conv_fwd", spy)
    x = torch.from_numpy(fx["c2.x"]).to(DEV).requires_grad_(True)
    with torch.no_grad():
        a = g13_forward(layer, fx, "c2", x)
    b = g13_forward(layer, fx, "c2", x)
    assert var_args[0] is None and var_args[1] is not None
    assert a.grad_fn is None and not a.requires_grad and b.grad_fn is not None
    assert torch.equal(a, b.detach())


def test_switch_off_never_reaches_the_kernel(amd, golden):
    fx = golden("g13_mnf_conv2d")
    layer = conv_layer(amd, fx, "c1")
    assert amd._dispatch.MNF_CONV_FUSED is False
    with torch.no_grad():
        g13_forward(layer, fx, "c1")
    assert amd.last_kernel() != FAMILY


def test_layer_forward_repeats_and_draws_its_own_noise(amd, golden, fused):
    fx = golden("g13_mnf_conv2d")
    layer = conv_layer(amd, fx, "c1")
    with torch.no_grad():
        a, b = g13_forward(layer, fx, "c1"), g13_forward(layer, fx, "c1")
        x = torch.from_numpy(fx["c1.x"]).to(DEV)
        c, d = layer.forward(x), layer.forward(x)  # default draws
    assert torch.equal(a, b)
    assert amd.last_kernel() == FAMILY
    assert c.shape == a.shape and bool(torch.isfinite(c).all()) and not torch.equal(c, d)


def test_forward_in_a_hipgraph_replays_the_eager_result(amd, golden, fused):
    fx = golden("g13_mnf_conv2d")
    layer = conv_layer(amd, fx, "c2")
    inputs = g13_inputs(fx, "c2")  # staged before the capture: no host copies inside it
    side = torch.cuda.Stream()
    with torch.no_grad():
        eager = g13_forward(layer, fx, "c2", inputs=inputs)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):  # warm-up off the default stream, as capture requires
            g13_forward(layer, fx, "c2", inputs=inputs)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y = g13_forward(layer, fx, "c2", inputs=inputs)
        assert amd.last_kernel() == FAMILY
    y.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, eager)


# ------------------------------------------------------------------ gradients
_ORACLE_GRADS: dict = {}


def oracle_grads(O, fx, tag, w_out):
    """{dtype: {name: gradient}} of sum(y * w_out) by autograd through the oracle (x's too for c2); computed once per tag."""
    if tag not in _ORACLE_GRADS:
        t = lambda name, dt: torch.from_numpy(fx[f"{tag}.{name}"]).to(dt)  # noqa: E731
        ref = {}
        for dt in (torch.float32, torch.float64):
            p = {k_: t(k_, dt).clone().requires_grad_(True) for k_ in G13_KEYS}
            specs = g13_specs(tag, "q", fx[f"{tag}.fwd.masks"])
            for sp in specs:
                sp["mask"] = sp["mask"].to(dt)
                sp["params"] = {k_: v.to(dt).clone().requires_grad_(True) for k_, v in sp["params"].items()}
            x = t("x", dt).requires_grad_(tag == "c2")
            z, _ = O.mnf_conv2d_sample_z(p["q0_mean"], p["q0_log_var"], t("fwd.eps_z", dt), specs)
            y = O.mnf_conv2d_forward(x, z, p["W_mean"], p["W_log_var"], p["b_log_var"], t("fwd.eps_out", dt))
            (y * w_out.to(dt)).sum().backward()
            grads = {k_: v.grad for k_, v in p.items() if v.grad is not None}
            for i, sp in enumerate(specs):
                grads.update({f"flow_q.flows.{i}.{k_}": v.grad for k_, v in sp["params"].items()})
            if tag == "c2":
                grads["x"] = x.grad
            ref[dt] = grads
        _ORACLE_GRADS[tag] = ref
    return _ORACLE_GRADS[tag]


@pytest.mark.parametrize("tag", ["c1", "c2"])
def test_fused_route_gradients_vs_float64_oracle(amd, O, golden, fused, tag):
    """The procedure of tests/test_hip_kl.py::test_mnf_conv2d_forward_gradients_vs_float64_oracle with the switch on: every
    parameter the output depends on (plus x for c2) against autograd through the float64 oracle on fixture G13's draws,
    within 1e-5 + twice the float32 oracle's own distance; a FlatParameters home receives the same gradients in place,
    within 2e-6 normwise."""
    fx = golden("g13_mnf_conv2d")
    shape = fx[f"{tag}.y"].shape
    w_out = recipes.gaussian(7700 + G13_CASES[tag][1], shape[0], int(np.prod(shape[1:]))).reshape(shape)
    ref = oracle_grads(O, fx, tag, w_out)

    def run(homed):
        layer = conv_layer(amd, fx, tag)
        flat = amd.FlatParameters(layer) if homed else None
        x = torch.from_numpy(fx[f"{tag}.x"]).to(DEV).requires_grad_(tag == "c2")
        y = g13_forward(layer, fx, tag, x)
        assert amd.last_kernel() == FAMILY
        (y * w_out.to(DEV)).sum().backward()
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
        assert err <= GBASE + widen, f"MNFConv2d.forward ({FAMILY}) {tag} grad {name}: {err:.2e} > 1e-5 + {widen:.2e}"
    homed, flat = run(True)
    for name, g in got.items():
        if g is not None and homed[name] is not None and float(g.abs().max()) > 0:
            assert normwise_err(homed[name].numpy(), g.numpy()) <= 2e-6, name
    assert all(p.grad is v for p, v in zip(flat.params, flat._grad_views))
