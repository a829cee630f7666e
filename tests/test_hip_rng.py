"""The three in-kernel random streams of mnf_device.h against their host restatement (tests/rng_reference.py):

* the materialisers mnf_rnvp_mask (bit-exact), mnf_mnf_linear_noise and mnf_sample_z0_noise (float64 reference on the
  device's own float32 uniforms), at shapes with odd dims, half pairs, 4 k + 2 and 4 k columns, and the per-slab seeds
  of a layer wider than 64 outputs;
* the streams' edges, reached on purpose with rng_reference.seed_for: the largest magnitude (h1 >> 8 == 0), u1 == 1 and
  just below it (log2 -> +-0 / -1e-7: the square root must not see a positive logarithm), phases where cos or sin
  crosses zero -- through the materialisers AND through the kernels that generate the noise in place;
* the consumers (mnf_sample_z0_seeded and its two gradient forms, MNFLinear.forward in eval and in training) against
  float64 on the REFERENCE's noise, not on what the device materialises;
* the two call sites of ml_normal no other test reaches with a seed: the fp32 fix-up kernels of MNFLinear's forward
  and gradient pass (profiles/r13/rng_stream.txt lists every call site of the streams with the test that pins it).

Normals are compared by |dev - ref| / max(1, r_ref), r_ref = sqrt(-2 ln u1).  NORMAL_TOL: 4 x the worst figure measured
over every case of this file on an MI355X, rounded up to one digit (profiles/r13/rng_stream.txt); never above 1e-5.
"""
import ctypes

import numpy as np
import pytest
import torch

import recipes
import rng_reference as R
from helpers import assert_parity, budgeted, normwise_err

pytestmark = pytest.mark.gpu
DEV = "cuda"

NORMAL_TOL = {"ml": 1e-6, "z0": 9e-7}  # measured worst: 2.268e-7 / 2.178e-7
assert all(v <= 1e-5 for v in NORMAL_TOL.values())

SEED_HI = 0x123456789ABCDEF0   # seed >> 32 != 0
SEED_C = 0x9E3779B97F4A7C15    # the consumers' seed (element (0, 0) of both normal streams is ~0.6 under it)


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


def _u64(seed):
    return ctypes.c_uint64(int(seed) & R.M64)


def _materialise(amd, fn, seed, rows, cols):
    out = torch.full((rows, cols), float("nan"), device=DEV)
    amd._lib.check(fn, getattr(amd._lib.load(), fn)(_u64(seed), out.data_ptr(), rows, cols, None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check_normals(stream, dev, ref, what):
    """|dev - ref| / max(1, r_ref) <= NORMAL_TOL[stream] everywhere, and everything finite.  Prints the array's worst
    figure (pytest -s): the maximum over the file is what NORMAL_TOL was set from."""
    x, h1, _ = ref
    dev = np.asarray(dev, dtype=np.float64)
    assert dev.shape == x.shape, (dev.shape, x.shape)
    assert np.isfinite(dev).all(), f"{what}: not finite at {np.argwhere(~np.isfinite(dev))[:4].tolist()}"
    err = np.abs(dev - x) / np.maximum(1.0, R.radius(h1))
    worst = float(err.max()) if err.size else 0.0
    at = np.unravel_index(int(err.argmax()), err.shape)
    print(f"{what}: worst |dev - ref| / max(1, r) = {worst:.3e} at {tuple(int(i) for i in at)} "
          f"(ref {x[at]:+.6f}, h1 {int(h1[at]):#010x})")
    assert worst <= NORMAL_TOL[stream], f"{what}: {worst:.3e} > {NORMAL_TOL[stream]:.0e} at {at}"
    return worst


# ------------------------------------------------------------------------------------------------------ materialisers
@pytest.mark.parametrize("seed", [0, SEED_HI], ids=hex)
@pytest.mark.parametrize("rows,dim", [(1, 1), (17, 31), (33, 32), (16, 33), (333, 50), (70, 800)])
def test_mask_materialiser_is_the_reference_bit_for_bit(amd, rows, dim, seed):
    got = _materialise(amd, "mnf_rnvp_mask", seed, rows, dim)
    assert np.array_equal(got, R.mask(seed, rows, dim))


@pytest.mark.parametrize("seed", [0, SEED_HI], ids=hex)  # (seed 0: element (0, 0) has h1 == 0, the largest radius)
@pytest.mark.parametrize("rows,n_out", [(1, 1), (17, 10), (333, 64)])
def test_mnf_linear_noise_materialiser_vs_reference(amd, rows, n_out, seed):
    got = _materialise(amd, "mnf_mnf_linear_noise", seed, rows, n_out)
    check_normals("ml", got, R.ml_normal(seed, rows, n_out), f"mnf_mnf_linear_noise {rows}x{n_out} seed {seed:#x}")


@pytest.mark.parametrize("n_out", [65, 256])
def test_mnf_linear_noise_for_uses_the_slab_seeds(amd, n_out):
    """A layer wider than 64 outputs draws one stream per 64-output slab: seed + k * 0x9E3779B97F4A7C15 mod 2**64, the
    column index restarting in each slab."""
    layer = amd.MNFLinear(8, n_out)
    for seed in (SEED_HI, R.M64):  # (the second one wraps past 2**64 at slab 1)
        got = layer.noise_for(seed, 37).cpu().numpy()
        check_normals("ml", got, R.mnf_linear_noise(seed, 37, n_out), f"MNFLinear(8, {n_out}).noise_for seed {seed:#x}")


@pytest.mark.parametrize("seed", [R.Z0_XOR, SEED_HI], ids=hex)  # (seed 0x5bd1e995: element (0, 0) has h1 == 0)
@pytest.mark.parametrize("rows,dim", [(1, 1), (1, 7), (17, 2), (1000, 27), (333, 50), (19, 6), (64, 800)])
def test_sample_z0_noise_materialiser_vs_reference(amd, rows, dim, seed):
    got = _materialise(amd, "mnf_sample_z0_noise", seed, rows, dim)
    check_normals("z0", got, R.z0_normal(seed, rows, dim), f"mnf_sample_z0_noise {rows}x{dim} seed {seed:#x}")


# --------------------------------------------------------------------------------------------------------- edge seeds
def _sample_z0_in_kernel(amd, seed, rows, dim):
    """mnf_sample_z0_seeded with mean 0 and log-variance 0: z0 = fma(1, eps, 0) IS the noise the kernel generated."""
    zero = torch.zeros(dim, device=DEV)
    out = torch.full((rows, dim), float("nan"), device=DEV)
    amd._lib.check("mnf_sample_z0_seeded", amd._lib.load().mnf_sample_z0_seeded(
        zero.data_ptr(), zero.data_ptr(), _u64(seed), out.data_ptr(), rows, dim, None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


_UNIT_LAYERS: dict = {}


def _mnf_linear_in_kernel(amd, seed, rows, n_out):
    """mnf_mnf_linear_fwd on x = 0 with b_mean = 0 and b_log_var = 0: out = 0 + sqrt(1) * eps IS the noise the forward
    kernel generated for its tile."""
    from torch_mnf_amd import layers as L

    n_in = 16
    layer = _UNIT_LAYERS.get(n_out)
    if layer is None:
        layer = amd.MNFLinear(n_in, n_out)
        with torch.no_grad():
            layer.b_mean.zero_()
            layer.b_log_var.zero_()
        layer = _UNIT_LAYERS[n_out] = layer.to(DEV)
    x = torch.zeros(rows, n_in, device=DEV)
    z = torch.ones(rows, n_in, device=DEV)
    out, flags = L._mnf_linear_forward(layer, x, z, None, int(seed) & R.M64, L._require_operands(layer, x.device), None)
    assert amd.last_kernel() == "mnf_linear_fwd"
    torch.cuda.synchronize()
    assert not flags.any()  # no group went to the fix-up kernel
    return out.cpu().numpy()


K24 = 1 << 24
EDGES = ([("h1>>8=0", 0xAB)]
         + [(f"h1>>8=2^24-{d}", ((K24 - d) << 8) | 0x5A) for d in (1, 2, 3)]
         + [(f"h2>>8={name}", R.h1_for_h2((k << 8) | 0x33)) for name, k in (("0", 0), ("2^22", 1 << 22), ("2^23", 1 << 23),
                                                                           ("2^24-1", K24 - 1))])


@pytest.mark.parametrize("edge,h1", EDGES, ids=[e for e, _ in EDGES])
@pytest.mark.parametrize("stream", ["ml", "z0"])
def test_edge_seeds(amd, stream, edge, h1):
    """An element with a chosen h1 (so a chosen u1, or through h2 a chosen phase), at (3, 2) of a 4 x 4 call and in the
    last row of a 17-row call (a partial tile of the kernels that generate in place): finite, and the reference's value."""
    ref_fn, fn, in_kernel = {"ml": (R.ml_normal, "mnf_mnf_linear_noise", _mnf_linear_in_kernel),
                             "z0": (R.z0_normal, "mnf_sample_z0_noise", _sample_z0_in_kernel)}[stream]
    for rows, cols, row, col, hi in ((4, 4, 3, 2, 0), (17, 6, 16, 2, 0x9ABCDEF0)):  # (6 columns: z0's scalar path)
        seed = R.seed_for(h1, hi, row, col, stream)
        ref = ref_fn(seed, rows, cols)
        assert int(ref[1][row, col]) == h1
        if edge == "h1>>8=0":
            assert abs(float(R.radius(ref[1])[row, col]) - R.R_MAX) < 1e-12
        if edge == "h1>>8=2^24-1":
            assert ref[0][row, col] == 0.0  # u1 == 1 exactly: the noise is +-0
        what = f"{stream} {edge} at ({row}, {col}) of {rows}x{cols}"
        got = _materialise(amd, fn, seed, rows, cols)
        check_normals(stream, got, ref, what + " materialised")
        got_k = in_kernel(amd, seed, rows, cols)
        check_normals(stream, got_k, ref, what + " in-kernel")
        assert np.array_equal(got, got_k), f"{what}: the kernel's noise is not what the materialiser writes"


# ---------------------------------------------------------------- consumers of the normal streams, on the reference's noise
Z0_SHAPES = [(1, 1), (1, 7), (17, 2), (1000, 27), (333, 50), (19, 6), (19, 8)]  # ((19, 8): the 4-wide forward and gradient kernels)


@pytest.mark.parametrize("rows,dim", Z0_SHAPES)
def test_sample_z0_seeded_and_its_gradients_on_reference_noise(amd, rows, dim):
    """mnf_sample_z0_seeded against mean + exp(log_var / 2) eps_ref, and mnf_sample_z0_seeded_bwd / _bwd_det against
    float64 autograd of the same expression (standard deviations of ~1, so that the noise is what is compared)."""
    lib = amd._lib.load()
    seed = SEED_C
    mean = (0.1 * recipes.gaussian(61, 1, dim)[0]).contiguous()
    log_var = (0.3 * recipes.gaussian(62, 1, dim)[0]).contiguous()
    g = (recipes.gaussian(63, rows, dim) / rows).contiguous()
    eps_ref = torch.from_numpy(R.z0_normal(seed, rows, dim)[0])
    m64, v64 = mean.double().requires_grad_(True), log_var.double().requires_grad_(True)
    z64 = m64 + (v64 / 2).exp() * eps_ref
    (z64 * g.double()).sum().backward()
    what = f"sample_z0_seeded {rows}x{dim}"
    mean_d, lv_d, g_d = mean.to(DEV), log_var.to(DEV), g.to(DEV)
    z_got = torch.full((rows, dim), float("nan"), device=DEV)
    amd._lib.check("z0s", lib.mnf_sample_z0_seeded(mean_d.data_ptr(), lv_d.data_ptr(), _u64(seed), z_got.data_ptr(), rows,
                                                    dim, None))
    torch.cuda.synchronize()
    budgeted(normwise_err(z_got.cpu().numpy(), z64.detach().numpy()), 1e-5, what + " z0 vs float64 on reference noise")
    out = torch.zeros(2 * dim, device=DEV)
    amd._lib.check("bwds", lib.mnf_sample_z0_seeded_bwd(g_d.data_ptr(), _u64(seed), lv_d.data_ptr(), out.data_ptr(),
                                                         out.data_ptr() + 4 * dim, rows, dim, None))
    n_ws = int(lib.mnf_sample_z0_bwd_workspace(rows, dim))
    ws = torch.empty(max(n_ws, 1), device=DEV)
    out_det = torch.zeros(2 * dim, device=DEV)
    amd._lib.check("bwd_det", lib.mnf_sample_z0_bwd_det(g_d.data_ptr(), None, _u64(seed), lv_d.data_ptr(),
                                                         out_det.data_ptr(), out_det.data_ptr() + 4 * dim, rows, dim,
                                                         ws.data_ptr(), ws.numel(), None))
    torch.cuda.synchronize()
    for name, o in (("seeded_bwd", out), ("bwd_det", out_det)):
        budgeted(normwise_err(o[:dim].cpu().numpy(), m64.grad.numpy()), 1e-5, f"{what} {name} grad_mean")
        budgeted(normwise_err(o[dim:].cpu().numpy(), v64.grad.numpy()), 1e-5, f"{what} {name} grad_log_var")


class _FixedZ:
    """Stand-in for sample_z: a known z with a grad slot, and no draw from torch's generator before the noise seed."""

    def __init__(self, z):
        self.z = z

    def __call__(self, batch_size=1, eps=None, masks=None):
        return self.z, torch.zeros(self.z.shape[0], device=self.z.device)


def _mnf_linear_params(seed, n_in, n_out):
    g = torch.Generator().manual_seed(seed)
    return {"W_mean": 0.1 * torch.randn(n_out, n_in, generator=g), "W_log_var": -2 + 0.5 * torch.randn(n_out, n_in, generator=g),
            "b_mean": 0.1 * torch.randn(n_out, generator=g), "b_log_var": -2 + 0.5 * torch.randn(n_out, generator=g)}


def _oracle(O, p, x, z, eps64, w_out):
    """(fp32, fp64) gradients of sum(out * w_out) through the oracle's MNFLinear.forward, and both outputs."""
    grads, outs = [], []
    for dt in (torch.float32, torch.float64):
        xx, zz = x.detach().to(dt).requires_grad_(True), z.detach().to(dt).requires_grad_(True)
        q = {k: v.detach().to(dt).clone().requires_grad_(True) for k, v in p.items()}
        o = O.mnf_linear_forward(xx, zz, q["W_mean"], q["W_log_var"], q["b_mean"], q["b_log_var"], eps64.to(dt))
        (o * w_out.to(dt)).sum().backward()
        grads.append({"x": xx.grad, "z": zz.grad, **{k: v.grad for k, v in q.items()}})
        outs.append(o.detach())
    return grads[0], grads[1], outs[0], outs[1]


def _drawn_seed(torch_seed):
    """The seed MNFLinear.forward draws from torch's CPU generator right after torch.manual_seed(torch_seed)."""
    torch.manual_seed(torch_seed)
    return int(torch.empty((), dtype=torch.int64).random_().item()) & R.M64


@pytest.mark.parametrize("n_out", [10, 65])
def test_mnf_linear_forward_and_gradients_on_reference_noise(amd, O, n_out):
    """MNFLinear.forward with the noise generated in the kernel (eval, and training with the six gradients of
    mnf_mnf_linear_bwd) against the float64 oracle fed the REFERENCE's noise for the seed the call drew (variances of
    ~0.1 + x^2, so that the noise term is a visible part of the output).  n_out = 65: two slabs, two seeds."""
    from test_hip_autograd import check_vs_float64

    n_in, rows = 33, 37
    p = _mnf_linear_params(7100 + n_out, n_in, n_out)
    x = recipes.gaussian(7200 + n_out, rows, n_in).abs()
    z = 1.0 + 0.3 * recipes.gaussian(7300 + n_out, rows, n_in)
    w_out = recipes.gaussian(7400 + n_out, rows, n_out)
    layer = amd.MNFLinear(n_in, n_out)
    layer.load_state_dict(p, strict=False)
    layer.to(DEV)
    xg, zg = x.to(DEV).requires_grad_(True), z.to(DEV).requires_grad_(True)
    layer.sample_z = _FixedZ(zg)
    eps_ref = torch.from_numpy(R.mnf_linear_noise(_drawn_seed(77), rows, n_out)[0])
    g32, g64, o32, o64 = _oracle(O, p, x, z, eps_ref, w_out)
    what = f"MNFLinear({n_in}, {n_out}) rows={rows} on reference noise"
    with torch.no_grad():
        torch.manual_seed(77)
        y_eval = layer.forward(xg)
    assert amd.last_kernel() == "mnf_linear_fwd"
    assert_parity(y_eval, o32.numpy(), o64.numpy(), what + " eval")
    torch.manual_seed(77)
    y = layer.forward(xg)
    assert y.requires_grad
    assert_parity(y, o32.numpy(), o64.numpy(), what + " training")
    (y * w_out.to(DEV)).sum().backward()
    assert amd.last_kernel() == "mnf_linear_bwd"
    got = {"x": xg.grad, "z": zg.grad, **{k: getattr(layer, k).grad for k in p}}
    for k in g64:
        check_vs_float64(got[k].cpu(), g32[k], g64[k], f"{what} grad {k}")


# ----------------------------------------------------------------------------- call sites no other test reaches with a seed
def test_mnf_linear_fixup_kernels_generate_the_reference_noise(amd):
    """mnf_linear_fixup_kernel (mnf_mnf_linear.hip) and ml_bwd_fixup_kernel (mnf_mnf_linear_bwd.hip) redo in fp32 the
    128-row groups whose x z or x^2 leave the split range, and regenerate the noise for them when the call was seeded.
    Seeded call against the explicit call on the reference's noise (the host builds it): 165 rows = one whole group and a
    ragged one, the ragged one flagged, 10 outputs."""
    from torch_mnf_amd import layers as L

    n_in, n_out, rows = 50, 10, 128 + 37
    p = _mnf_linear_params(7500, n_in, n_out)
    x = recipes.gaussian(7501, rows, n_in).abs()
    x[140] *= 400.0  # x^2 ~ 1e5 > f16's 65504 in group 1
    z = 1.0 + 0.3 * recipes.gaussian(7502, rows, n_in)
    w_out = recipes.gaussian(7503, rows, n_out)
    seed = SEED_HI
    eps_ref = torch.from_numpy(R.ml_normal(seed, rows, n_out)[0]).float().to(DEV)
    layer = amd.MNFLinear(n_in, n_out)
    layer.load_state_dict(p, strict=False)
    layer.to(DEV)
    _, flags = L._mnf_linear_forward(layer, x.to(DEV), z.to(DEV), None, seed, L._require_operands(layer, torch.device(DEV, 0)), None)
    assert flags.tolist() == [0, 1], "group 1 should have gone to the fix-up kernel, group 0 not"
    runs = {}
    for name, eps in (("seeded", None), ("explicit", eps_ref)):
        layer.zero_grad()
        xg, zg = x.to(DEV).requires_grad_(True), z.to(DEV).requires_grad_(True)
        params = (layer.W_mean, layer.W_log_var, layer.b_mean, layer.b_log_var)
        y = L._MnfLinearFn.apply(xg, zg, *params, layer, eps, seed if eps is None else 0)
        (y * w_out.to(DEV)).sum().backward()
        assert amd.last_kernel() == "mnf_linear_bwd"
        runs[name] = {"out": y.detach().cpu(), "x": xg.grad.cpu(), "z": zg.grad.cpu(),
                      **{k: getattr(layer, k).grad.clone().cpu() for k in p}}
    for k, ref in runs["explicit"].items():
        # (row 140 dominates every norm: it is in the group the fix-up kernels compute)
        budgeted(normwise_err(runs["seeded"][k].numpy(), ref.numpy()), 1e-5, f"MNFLinear fix-up kernels, seeded vs explicit: {k}")
    for k in ("out", "x", "z"):  # per-row tensors: the flagged group without row 140, so that its other rows count
        sl = [r for r in range(128, rows) if r != 140]
        budgeted(normwise_err(runs["seeded"][k][sl].numpy(), runs["explicit"][k][sl].numpy()), 1e-5,
                 f"MNFLinear fix-up kernels, seeded vs explicit, rows 128.. without 140: {k}")


# ------------------------------------------------------------- every mask call site under a seed whose high half is not zero
# (kernel that must run, dim, hidden widths, rows, layer switches): rows no multiple of 16, dim no multiple of 32 wherever
# the kernel takes such a shape (rnvp_resident and rnvp_split at these widths: d = 800 only)
MASK_FWD_SITES = [
    ("rnvp_narrow", 50, (50,), 131, {}),
    ("rnvp_split_resident_operands", 70, (50,), 131, {}),
    ("rnvp_split", 800, (30,), 131, {}),
    ("rnvp_mfma_fp32", 70, (50,), 131, {"force_fp32_mfma": True}),
    ("rnvp_resident", 800, (50,), 100, {}),
    ("rnvp_few", 20, (50,), 63, {}),
    ("rnvp_generic", 20, (50,), 63, {"force_generic": True}),
    ("rnvp_rt", 50, (17,), 37, {"force_generic": 2}),
]
MASK_BWD_SITES = [
    ("rnvp_bwd_few", 33, (7,), 65, {}, {}),
    ("rnvp_bwd_mfma", 50, (50,), 129, {}, {"RNVP_BWD_MFMA_MIN_ROWS": 0, "RNVP_BWD_MFMA_MIN_DIM": 0, "RNVP_BWD_FEW_GRID_OFF": True}),
    ("rnvp_bwd_generic", 50, (50,), 129, {"force_generic": True}, {"RNVP_BWD_FEW_GRID_OFF": True}),
    ("rnvp_bwd_rt", 50, (17,), 300, {"force_generic": 2}, {}),
]


def _rnvp(amd, dim, hs, switches):
    f = amd.RNVP(dim, h_sizes=hs)
    f.load_state_dict(recipes.rnvp_params_layers(8800 + dim, dim, hs))
    for k, v in switches.items():
        setattr(f, k, v)
    return f.to(DEV)


@pytest.mark.parametrize("kernel,dim,hs,rows,switches", MASK_FWD_SITES, ids=[c[0] for c in MASK_FWD_SITES])
def test_mask_call_sites_forward_with_a_64_bit_seed(amd, kernel, dim, hs, rows, switches):
    """The seeded tests of the other files use seeds below 2**32 (77, 5, 12345): the (uint32_t)(seed >> 32) term of a
    site's row hash (written out by hand in mnf_rnvp_resident.hip) is not exercised by them.  Seeded call against the
    explicit call on the mask the HOST builds, seed >> 32 != 0, and last_kernel() names the kernel that took it."""
    f = _rnvp(amd, dim, hs, switches)
    z = recipes.gaussian(8801 + dim, rows, dim).to(DEV)
    mask = torch.from_numpy(R.mask(SEED_HI, rows, dim)).to(DEV)
    with torch.no_grad():
        x_s, ld_s = f.forward(z, seed=SEED_HI)
        assert amd.last_kernel() == kernel, amd.last_kernel()
        x_m, ld_m = f.forward(z, mask=mask)
    # (the in-kernel-mask form of the gate and the float-mask form agree to rounding, not bit for bit)
    budgeted(normwise_err(x_s.cpu().numpy(), x_m.cpu().numpy()), 1e-5, f"{kernel} seeded (64-bit seed) vs host mask: x")
    budgeted(normwise_err(ld_s.cpu().numpy(), ld_m.cpu().numpy()), 1e-5, f"{kernel} seeded (64-bit seed) vs host mask: log_det")


@pytest.mark.parametrize("kernel,dim,hs,rows,switches,dispatch", MASK_BWD_SITES, ids=[c[0] for c in MASK_BWD_SITES])
def test_mask_call_sites_backward_with_a_64_bit_seed(amd, monkeypatch, kernel, dim, hs, rows, switches, dispatch):
    """The gradient kernels regenerate the mask of a seeded forward call: their gradients against those of the explicit
    call on the host-built mask (kernel against kernel, two fp32 evaluations of the row sums: the 2e-5 bar of
    test_hip_autograd.GTOL), seed >> 32 != 0."""
    import torch_mnf_amd.flows as fl

    for k, v in dispatch.items():
        monkeypatch.setattr(fl._dispatch, k, v)
    w_x = recipes.gaussian(8802 + dim, rows, dim).to(DEV)
    w_l = recipes.gaussian(8803 + dim, rows, 1)[:, 0].to(DEV)
    mask = torch.from_numpy(R.mask(SEED_HI, rows, dim)).to(DEV)
    grads = {}
    for name, kw in (("seeded", {"seed": SEED_HI}), ("explicit", {"mask": mask})):
        f = _rnvp(amd, dim, hs, switches)
        z = recipes.gaussian(8801 + dim, rows, dim).to(DEV).requires_grad_(True)
        x, ld = f.forward(z, **kw)
        ((x * w_x).sum() + (ld * w_l).sum()).backward()
        if name == "seeded":
            assert amd.last_kernel() == kernel, amd.last_kernel()
        grads[name] = {"z": z.grad, **{n: q.grad for n, q in f.named_parameters()}}
    for k, g in grads["explicit"].items():
        budgeted(normwise_err(grads["seeded"][k].cpu().numpy(), g.cpu().numpy()), 2e-5,
                 f"{kernel} seeded (64-bit seed) vs host mask: grad {k}")
