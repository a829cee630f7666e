"""Training a run of equal-shaped AffineHalfFlow layers WITHOUT a per-shape kernel as ONE autograd node on the
run-time-shaped kernels (``fuse_rt_training``): one "ahf_stack_rt" launch forward with every output kept, one
"ahf_bwd_stack_rt" launch backward (mnf_affine_half_bwd_rt_stack / _det).

The gradient launch is the single layer's kernel with a layer loop, so its fixed-order form is compared BIT FOR BIT with
n calls of the single layer's fixed-order entry on the same inputs and the same gradient scale; that comparison is also
the test of the cotangent hand-over between layers (each lane reads the grad_x it stored).  Row counts: 300 has a partial
tile, 2,100 several row blocks, 65,536 x 64 gives every workgroup of the persistent grid several row blocks per layer."""
import pytest
import torch

import recipes
from helpers import assert_close
from test_hip_autograd import OracleGrads, cot_loss  # the audited gradient budget: GBASE + float64 head-room

pytestmark = pytest.mark.gpu

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


def _stream():
    return torch.cuda.current_stream().cuda_stream


def bits(a):
    return a.contiguous().view(torch.int32)


def same_bits(a, b, what=""):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert torch.equal(bits(a), bits(b)), f"{what}: {int((bits(a) != bits(b)).sum())} of {a.numel()} elements differ"


# (dim, h_sizes, kwargs): the gradient kernel's shape classes -- one and several input tiles, unaligned rows (dim 10),
# one column per half (dim 2), the widest hidden layers, three and two hidden layers, NICE and no-shift variants
SHAPES = [(64, (24, 24), {}), (64, (64, 64, 64), {}), (10, (16, 40), {}), (2, (24, 24), {}), (512, (24, 24, 24), {}),
          (64, (24, 24), {"scale": False}), (64, (24, 24), {"shift": False})]
RUNS = [(d, h, kw, n) for d, h, kw in SHAPES for n in ((2, 3, 9) if not kw and d != 512 else (3,))]
RUN_IDS = [f"d{d}-h{'x'.join(map(str, h))}-L{n}" + "".join(f"-{k}{int(v)}" for k, v in kw.items()) for d, h, kw, n in RUNS]
LP_RUNS = [(d, h, kw) for d, h, kw in SHAPES]
SHAPE_IDS = [f"d{d}-h{'x'.join(map(str, h))}" + "".join(f"-{k}{int(v)}" for k, v in kw.items()) for d, h, kw in SHAPES]


class Run:
    """n layers' parameters back to back, a batch, and the forward run's outputs (mnf_affine_half_rt_stack, ctypes)."""

    def __init__(self, amd, dim, hs, kw, n, rows, inverse, parities, gain=1.0):
        from torch_mnf_amd import _lib

        self.lib, self._lib = _lib.load(), _lib
        self.dim, self.n, self.rows, self.inverse = dim, n, rows, inverse
        self.hid = (len(hs), _lib.int_array(list(hs)))
        self.flags = (int(kw.get("scale", True)), int(kw.get("shift", True)))
        flats = []
        for i in range(n):
            f = amd.AffineHalfFlow(dim, parity=bool(parities[i]), h_sizes=hs, **kw)
            f.load_state_dict(recipes.affine_half_params(500 + 3 * dim + i, dim, h_sizes=hs, s_last_gain=gain, **kw))
            flats.append(torch.cat([p.detach().reshape(-1) for p in f.parameters()]))
        self.n_params = flats[0].numel()
        self.flats = torch.cat(flats).to(DEV).contiguous()
        self.parities = [int(bool(p)) for p in parities]
        self.par = _lib.int_array(self.parities)
        # (a batch of half the unit scale: nine layers of either direction stay finite in every row)
        self.x = recipes.gaussian(600 + dim + rows, rows, dim, scale=0.5).to(DEV)
        self.outs = torch.empty((n, rows, dim), device=DEV)
        self.ld = torch.empty(rows, device=DEV)
        rc = self.lib.mnf_affine_half_rt_stack(
            self.x.data_ptr(), self.outs[-1].data_ptr(), self.outs.data_ptr() if n > 1 else None, self.ld.data_ptr(), None,
            None, None, 0, self.flats.data_ptr(), self.par, n, rows, dim, int(inverse), *self.hid, *self.flags, _stream())
        assert rc == _lib.MNF_OK, rc
        assert bool(torch.isfinite(self.outs).all()) and bool(torch.isfinite(self.ld).all())

    def tail(self):
        return (self.n, self.rows, self.dim, int(self.inverse), *self.hid, *self.flags)

    def ws_queries(self):
        """(floats for the run, floats for one layer, grid of the run, grid of one layer)"""
        a = (self.rows, self.dim, *self.hid, *self.flags)
        n_run = self.lib.mnf_affine_half_bwd_rt_stack_det_workspace(*a, self.n)
        n_one = self.lib.mnf_affine_half_bwd_rt_det_workspace(*a)
        slot = lambda k: (k + 63) // 64 * 64
        return n_run, n_one, n_run // slot(self.n * self.n_params), n_one // slot(self.n_params)

    def stack(self, gy, lp, gl, sc, det=True, want_flat=True):
        """One launch -> (rc, grad_x, grad_flats, kernel family)."""
        import torch_mnf_amd

        sc = sc.reshape(-1).expand(self.n).contiguous() if sc.numel() == 1 else sc  # (one scale per applied layer)
        gx, work = torch.full_like(self.x, float("nan")), torch.full_like(self.x, float("nan"))
        gf = torch.zeros_like(self.flats) if want_flat else None
        ptr = lambda t: None if t is None else t.data_ptr()
        args = (self.x.data_ptr(), self.outs.data_ptr(), ptr(gy), ptr(lp), ptr(gl), gx.data_ptr(),
                work.data_ptr() if self.n > 1 else None, ptr(gf), self.flats.data_ptr(), sc.data_ptr(), self.par, *self.tail())
        if det:
            n_ws = self.ws_queries()[0]
            ws = torch.empty(n_ws, device=DEV)
            rc = self.lib.mnf_affine_half_bwd_rt_stack_det(*args, ws.data_ptr(), n_ws, _stream())
        else:
            rc = self.lib.mnf_affine_half_bwd_rt_stack(*args, _stream())
        return rc, gx, gf, torch_mnf_amd.last_kernel()

    def layer_by_layer(self, gy, gl, sc, want_flat=True):
        """n calls of the single layer's fixed-order entry, last applied layer first -> (grad_x, grad_flats)."""
        gf = torch.zeros_like(self.flats) if want_flat else None
        self.flats64 = torch.zeros_like(self.flats, dtype=torch.float64)
        n_ws = self.ws_queries()[1]
        ws = torch.empty(n_ws, device=DEV)
        g = gy
        for i in range(self.n - 1, -1, -1):
            k = self.n - 1 - i if self.inverse else i  # model index of applied layer i
            x_in = self.x if i == 0 else self.outs[i - 1]
            gx = torch.full_like(self.x, float("nan"))
            rc = self.lib.mnf_affine_half_bwd_rt_det(
                x_in.data_ptr(), self.outs[i].data_ptr(), None if g is None else g.data_ptr(),
                None if gl is None else gl.data_ptr(), gx.data_ptr(),
                None if gf is None else gf.data_ptr() + 4 * self.n_params * k, self.flats.data_ptr() + 4 * self.n_params * k,
                sc.data_ptr(), self.rows, self.dim, self.parities[k], int(self.inverse), *self.hid, *self.flags,
                ws.data_ptr(), n_ws, _stream())
            assert rc == self._lib.MNF_OK, rc
            if gf is not None:  # the workgroups' slots of this call, added up in float64
                slot = (self.n_params + 63) // 64 * 64
                self.flats64[k * self.n_params:(k + 1) * self.n_params] = ws.view(-1, slot)[:, :self.n_params].double().sum(0)
            g = gx
        return g, gf


def cotangents(rows, dim, seed=0):
    g = torch.Generator(device=DEV).manual_seed(700 + rows + dim + seed)
    return torch.randn(rows, dim, device=DEV, generator=g) / rows, torch.randn(rows, device=DEV, generator=g) / rows


def check_one_launch_equals_n_launches(amd, dim, hs, kw, n, rows, inverse, parities, atomic_sums=True):
    from torch_mnf_amd import _lib
    from torch_mnf_amd.flows import _grad_scale

    run = Run(amd, dim, hs, kw, n, rows, inverse, parities)
    what = f"d={dim} h={hs} {kw} L={n} rows={rows} inv={inverse} par={parities}"
    n_run, n_one, grid_run, grid_one = run.ws_queries()
    # the slots stay far below their 512 MiB cap, so one launch and the single layer's launch have the same grid
    assert 0 < n_run * 4 < (512 << 20) // 4 and 0 < n_one * 4 < (512 << 20) // 4, (what, n_run, n_one)
    assert grid_run == grid_one and grid_run >= 1, (what, grid_run, grid_one)
    gy, gl = cotangents(rows, dim)
    sc = _grad_scale(gy, gl, rows, dim, run.x.device)
    ref_gx, ref_gf = run.layer_by_layer(gy, gl, sc)
    assert bool(torch.isfinite(ref_gx).all()) and bool(torch.isfinite(ref_gf).all()) and float(ref_gf.abs().max()) > 0, what
    rc, gx, gf, kernel = run.stack(gy, None, gl, sc, det=True)
    assert rc == _lib.MNF_OK and kernel == "ahf_bwd_stack_rt", (what, rc, kernel)
    same_bits(gx, ref_gx, what + " grad_x, fixed-order form")
    same_bits(gf, ref_gf, what + " grad_flats, fixed-order form")
    rc, gx, gf, kernel = run.stack(gy, None, gl, sc, det=False)
    if amd.deterministic():  # atomic sums are refused in that mode, as by mnf_affine_half_bwd_rt
        assert rc == _lib.MNF_ERR_UNSUPPORTED, what
        return
    assert rc == _lib.MNF_OK and kernel == "ahf_bwd_stack_rt", (what, rc, kernel)
    same_bits(gx, ref_gx, what + " grad_x, atomic form")
    if atomic_sums:
        from helpers import normwise_err

        # The reference: the n single-layer fixed-order calls' own slots (one per workgroup), added up in float64 -- the
        # same products as those calls' fp32 result, without a second fp32 summation order's rounding in the comparison
        ref64 = run.flats64
        assert_close(ref_gf.double(), ref64, 1e-6, what + " the reference's fp32 sums against its float64 sums")
        print(f"{what}: atomic grad_flats {normwise_err(gf.double().cpu().numpy(), ref64.cpu().numpy()):.3e} from the reference's "
              f"slots summed in float64 ({normwise_err(gf.cpu().numpy(), ref_gf.cpu().numpy()):.3e} from its fp32 sums)")
        assert_close(gf.double(), ref64, 1e-6, what + " grad_flats, atomic form")


@pytest.mark.parametrize("dim,hs,kw,n", RUNS, ids=RUN_IDS)
def test_one_launch_equals_n_launches_bit_for_bit(amd, dim, hs, kw, n):
    """Both directions; alternating parities and the same parity twice in a row; a partial tile and several row blocks."""
    alternating = [i % 2 for i in range(n)]
    twice = [1, 1] + [i % 2 for i in range(n - 2)]
    for rows in (300, 2100):
        for inverse in (False, True):
            for parities in (alternating, twice):
                check_one_launch_equals_n_launches(amd, dim, hs, kw, n, rows, inverse, parities)


@pytest.mark.parametrize("inverse", [False, True])
def test_hand_over_at_65536_rows(amd, inverse):
    """Every workgroup of the persistent grid owns several row blocks per layer: grad_x and the fixed-order sums bit for
    bit, the atomic form's grad_x bit for bit (its sums: the next test)."""
    check_one_launch_equals_n_launches(amd, 64, (24, 24), {}, 3, 65536, inverse, [0, 1, 0], atomic_sums=False)


@pytest.mark.parametrize("inverse", [False, True])
def test_atomic_sums_at_65536_rows(amd, inverse):
    """The atomic form's grad_flats at 65,536 rows, 1e-6 normwise of the n single-layer fixed-order calls' sums -- their
    slots added up in float64, so that one fp32 summation order is compared, not two (two fp32 orders of these 512-term
    sums were 5.3e-7 .. 1.0e-6 apart)."""
    check_one_launch_equals_n_launches(amd, 64, (24, 24), {}, 3, 65536, inverse, [0, 1, 0])


@pytest.mark.parametrize("n", [1, 4])
def test_missing_cotangents_and_one_layer(amd, n):
    """grad_y_last or grad_ld NULL, no parameter sums (grad_flats NULL), and n_layers = 1: the call it always was, under
    its own family name."""
    from torch_mnf_amd import _lib
    from torch_mnf_amd.flows import _grad_scale

    dim, hs, rows = 64, (24, 24), 2100
    for inverse in (False, True):
        run = Run(amd, dim, hs, {}, n, rows, inverse, [i % 2 for i in range(n)])
        gy, gl = cotangents(rows, dim, seed=n)
        for a, b, want_flat in ((gy, None, True), (None, gl, True), (gy, gl, False)):
            sc = _grad_scale(a, b, rows, dim, run.x.device)
            ref_gx, ref_gf = run.layer_by_layer(a, b, sc, want_flat)
            rc, gx, gf, kernel = run.stack(a, None, b, sc, det=True, want_flat=want_flat)
            assert rc == _lib.MNF_OK and kernel == ("ahf_bwd_stack_rt" if n > 1 else "ahf_bwd_rt")
            same_bits(gx, ref_gx, f"L={n} inv={inverse} grad_x")
            if want_flat:
                same_bits(gf, ref_gf, f"L={n} inv={inverse} grad_flats")


@pytest.mark.parametrize("dim,hs,kw", LP_RUNS, ids=SHAPE_IDS)
def test_lp_form_equals_the_materialised_cotangent(amd, dim, hs, kw):
    """d loss / d log p in, the last applied layer's grad_y = -outs[n - 1] lp_grad formed at the kernel's loads: the
    bits of form (a) on that tensor with grad_ld = lp_grad."""
    from torch_mnf_amd import _lib
    from torch_mnf_amd.flows import _grad_scale

    n = 3
    for rows in (300, 2100):
        run = Run(amd, dim, hs, kw, n, rows, True, [0, 1, 0])
        _, lp_grad = cotangents(rows, dim, seed=9)
        sc = _grad_scale(None, lp_grad, rows, dim, run.x.device)
        gy = -run.outs[n - 1] * lp_grad.unsqueeze(1)
        what = f"lp form d={dim} h={hs} {kw} rows={rows}"
        rc_a, gx_a, gf_a, _ = run.stack(gy, None, lp_grad, sc, det=True)
        rc_b, gx_b, gf_b, kernel = run.stack(None, lp_grad, None, sc, det=True)
        assert rc_a == rc_b == _lib.MNF_OK and kernel == "ahf_bwd_stack_rt", what
        assert bool(torch.isfinite(gx_a).all()) and float(gf_a.abs().max()) > 0, what
        same_bits(gx_b, gx_a, what + " grad_x")
        same_bits(gf_b, gf_a, what + " grad_flats")
        if not amd.deterministic():
            rc, gx_c, gf_c, _ = run.stack(None, lp_grad, None, sc, det=False)
            assert rc == _lib.MNF_OK
            same_bits(gx_c, gx_a, what + " grad_x, atomic form")
            assert_close(gf_c, gf_a, 1e-6, what + " grad_flats, atomic form")
        # both forms at once are refused
        assert run.stack(gy, lp_grad, None, sc)[0] == _lib.MNF_ERR_INVALID_ARG
        assert run.stack(None, lp_grad, lp_grad, sc)[0] == _lib.MNF_ERR_INVALID_ARG


# ------------------------------------------------------------------------------------------------ the Python route
def state_dicts(dim, hs, n, kw, seed0=31, gain=2.0):
    return [recipes.affine_half_params(seed0 + dim + i, dim, h_sizes=hs, s_last_gain=gain, **kw) for i in range(n)]


def build(amd, dim, hs, n, kw, sds, switch, force=0, tail=None, stack=False):
    flows = []
    for i, sd in enumerate(sds):
        f = amd.AffineHalfFlow(dim, parity=bool(i % 2), h_sizes=hs, **kw)
        f.load_state_dict(sd)
        f.force_generic = force
        flows.append(f)
    if stack:
        flows = [amd.FusedAffineStack(flows)]
        flows[0].fuse_rt_training = switch
    model = amd.NormalizingFlowModel(amd.StandardNormal(dim, DEV), flows + ([tail] if tail is not None else [])).to(DEV)
    model.fuse_rt_training = switch
    return model


def force_for(amd, dim, hs, kw, rows):
    """force_generic that puts the layers on the run-time-shaped tier: 2 below RT_MIN_ROWS and for shapes that have
    per-shape kernels ((64, (64, 64, 64))), else 0 (default dispatch)."""
    from torch_mnf_amd import _dispatch, _lib

    image = _lib.load().mnf_affine_half_image_floats(dim, len(hs), _lib.int_array(list(hs)), int(kw.get("scale", True)),
                                                     int(kw.get("shift", True)))
    return 2 if image > 0 or rows < _dispatch.RT_MIN_ROWS else 0


def grads_of(model, x):
    return {"x": x.grad, **{k: q.grad for k, q in model.named_parameters()}}


@pytest.mark.parametrize("dim,hs,kw", LP_RUNS, ids=SHAPE_IDS)
def test_gradients_against_the_float64_oracle(amd, O, dim, hs, kw):
    """Switch on, n = 3: -log_prob(x).mean() (the lp form) and a cot_loss on (zs[-1], log_det) of inverse / forward
    (the general form) against the float64 oracle at the audited budget.  Parameters and inputs: the recipes of
    test_hip_round6.py::test_affine_half_rt_gradients, layer i drawn with seed 31 + dim + i."""
    n = 3
    sds = state_dicts(dim, hs, n, kw)
    sd_all = {f"flows.{i}.{k}": v for i, sd in enumerate(sds) for k, v in sd.items()}

    def chain(x, p, inverse):
        ld = 0
        for i in (reversed(range(n)) if inverse else range(n)):
            x, l1 = O.affine_half(x, {k: p[f"flows.{i}.{k}"] for k in sds[i]}, bool(i % 2), inverse, **kw)
            ld = ld + l1
        return x, ld

    def nll(x, p, dt):
        z, ld = chain(x, p, True)
        return -(ld + O.std_normal_log_prob(z)).mean()

    for rows in (300, 2100):
        x_cpu = recipes.gaussian(232 + dim, rows, dim)
        w_y, w_l = recipes.gaussian(33, rows, dim), recipes.gaussian(34, rows, 1)[:, 0]
        force = force_for(amd, dim, hs, kw, rows)
        what = f"rt train run d={dim} h={hs} {kw} rows={rows}"
        model = build(amd, dim, hs, n, kw, sds, True, force)
        x = x_cpu.to(DEV).requires_grad_(True)
        lp = model.log_prob(x)
        assert amd.last_kernel() == "ahf_stack_rt" and "_AffineRunFn" in type(lp.grad_fn).__name__, what
        (-lp.mean()).backward()
        assert amd.last_kernel() == "ahf_bwd_stack_rt", what
        OracleGrads(nll, x_cpu, sd_all).check_all(grads_of(model, x), what + " -log_prob.mean()")
        for inverse in (True, False):
            model = build(amd, dim, hs, n, kw, sds, True, force)
            x = x_cpu.to(DEV).requires_grad_(True)
            zs, ld = model.inverse(x) if inverse else model.forward(x)
            assert amd.last_kernel() == "ahf_stack_rt", what
            ((zs[-1] * w_y.to(DEV)).sum() + (ld * w_l.to(DEV)).sum()).backward()
            assert amd.last_kernel() == "ahf_bwd_stack_rt", what
            ref = OracleGrads(cot_loss(lambda xx, p: chain(xx, p, inverse), w_y, w_l), x_cpu, sd_all)
            ref.check_all(grads_of(model, x), f"{what} cot_loss inv={inverse}")


def step(model, x_dev, loss="nll", w=None, mid=None):
    """One forward + backward -> (forward kernel, backward kernel, grad_fn name, gradients)."""
    import torch_mnf_amd as amd

    x = x_dev.detach().clone().requires_grad_(True)
    if loss == "nll":
        out = model.log_prob(x)
        k_fwd, node = amd.last_kernel(), type(out.grad_fn).__name__
        (-out.mean()).backward()
    else:
        zs, ld = model.inverse(x) if loss == "inverse" else model.forward(x)
        k_fwd, node = amd.last_kernel(), type(zs[-1].grad_fn).__name__
        total = (zs[-1] * w[0]).sum() + (ld * w[1]).sum()
        if mid is not None:
            total = total + (zs[mid] * w[0]).sum()
        total.backward()
    return k_fwd, amd.last_kernel(), node, grads_of(model, x)


def same_gradients(amd, on, off, what):
    for k in off:
        if k != "x":
            (same_bits(on[k], off[k], f"{what} {k}") if amd.deterministic() else assert_close(on[k], off[k], 1e-6, f"{what} {k}"))
    same_bits(on["x"], off["x"], what + " x.grad")


@pytest.mark.parametrize("loss", ["nll", "inverse", "forward"])
def test_the_route(amd, loss):
    """Switch on: one _AffineRunFn node, ahf_stack_rt / ahf_bwd_stack_rt; off: ahf_rt / ahf_bwd_rt; the gradients of the
    two routes agree -- x.grad bit for bit, the parameters bit for bit under MNF_DETERMINISTIC=1, else 1e-6 normwise.

    The gradient kernel's results depend on the power-of-two gradient scale in their last bit, and the layer-by-layer
    route computes one scale per layer from that layer's materialised cotangents (2048, 1024, 1024 on a batch of this
    shape in the lp form).  The run's launch takes one scale per applied layer, and the route computes exactly those: it
    walks the at most 512 rows mnf_affine_half_grad_scale samples through the layers first (flows._rt_layer_scales)."""
    dim, hs, n, rows = 64, (24, 24), 3, 4096
    sds = state_dicts(dim, hs, n, {}, gain=1.0)
    x = recipes.gaussian(811, rows, dim).to(DEV)
    w = (recipes.gaussian(812, rows, dim).to(DEV) / rows, recipes.gaussian(813, rows, 1)[:, 0].to(DEV) / rows)
    k_fwd, k_bwd, node, on = step(build(amd, dim, hs, n, {}, sds, True), x, loss, w)
    assert (k_fwd, k_bwd) == ("ahf_stack_rt", "ahf_bwd_stack_rt") and "_AffineRunFn" in node, (loss, k_fwd, k_bwd, node)
    k_fwd, k_bwd, node, off = step(build(amd, dim, hs, n, {}, sds, False), x, loss, w)
    assert (k_fwd, k_bwd) == ("ahf_rt", "ahf_bwd_rt") and "_AffineRunFn" not in node, (loss, k_fwd, k_bwd, node)
    from helpers import normwise_err

    print(f"switch on vs off, {loss}: x.grad {int((bits(on['x']) != bits(off['x'])).sum())} of {on['x'].numel()} elements "
          f"differ, normwise {normwise_err(on['x'].cpu().numpy(), off['x'].cpu().numpy()):.2e}; parameters "
          f"{max(normwise_err(on[k].cpu().numpy(), off[k].cpu().numpy()) for k in off if k != 'x'):.2e}")
    same_gradients(amd, on, off, f"switch on vs off, {loss}")


@pytest.mark.parametrize("case", ["few_rows", "force_generic_1", "force_fp32_mfma", "layer_events"])
def test_the_switch_changes_nothing_where_the_route_does_not_apply(amd, case):
    dim, hs, n = 64, (24, 24), 3
    rows = 1000 if case == "few_rows" else 4096
    sds = state_dicts(dim, hs, n, {}, gain=1.0)
    x = recipes.gaussian(821, rows, dim).to(DEV)
    w = (recipes.gaussian(822, rows, dim).to(DEV) / rows, recipes.gaussian(823, rows, 1)[:, 0].to(DEV) / rows)
    got = []
    for switch in (True, False):
        model = build(amd, dim, hs, n, {}, sds, switch)
        if case == "force_generic_1":
            model.flows[1].force_generic = 1
        elif case == "force_fp32_mfma":
            model.flows[2].force_fp32_mfma = True
        elif case == "layer_events":
            model.layer_events = []
        for loss in ("nll", "inverse"):
            got.append((switch, loss, step(model, x, loss, w)))
    for (_, loss, a), (_, _, b) in zip(got[:2], got[2:]):
        assert a[:3] == b[:3] and "stack" not in a[0] + a[1] and "_AffineRunFn" not in a[2], (case, loss, a[:3], b[:3])
        same_bits(a[3]["x"], b[3]["x"], f"{case} {loss} x.grad")
        # (only the layer_events case stays on kernels with fixed-order sums under MNF_DETERMINISTIC=1; the others run
        #  at least one layer on the VALU gradient kernel, whose atomic sums differ from one run to the next in any mode)
        exact = amd.deterministic() and case == "layer_events"
        for k in b[3]:
            if k != "x":
                (same_bits if exact else lambda p, q, s: assert_close(p, q, 1e-6, s))(a[3][k], b[3][k], f"{case} {loss} {k}")


def test_unaligned_rows_and_an_odd_storage_offset(amd):
    """dim = 10 (rows 40 bytes apart) and a 64-wide input that starts one float into its storage."""
    for dim, hs in ((10, (16, 40)), (64, (24, 24))):
        n, rows = 3, 3000
        sds = state_dicts(dim, hs, n, {}, gain=1.0)
        buf = torch.zeros(rows * dim + 1, device=DEV)
        x = buf[1:].view(rows, dim)
        x.copy_(recipes.gaussian(831, rows, dim).to(DEV))
        assert x.data_ptr() % 16 != 0 and x.is_contiguous()
        w = (recipes.gaussian(832, rows, dim).to(DEV) / rows, recipes.gaussian(833, rows, 1)[:, 0].to(DEV) / rows)
        got = []
        for switch in (True, False):
            model = build(amd, dim, hs, n, {}, sds, switch)
            xg = buf[1:].view(rows, dim).requires_grad_(True)
            zs, ld = model.inverse(xg)
            ((zs[-1] * w[0]).sum() + (ld * w[1]).sum()).backward()
            got.append((amd.last_kernel(), grads_of(model, xg)))
        assert got[0][0] == "ahf_bwd_stack_rt" and got[1][0] == "ahf_bwd_rt"
        same_gradients(amd, got[0][1], got[1][1], f"odd offset d={dim}")


def test_a_cotangent_on_an_intermediate_falls_back_inside_the_node(amd):
    dim, hs, n, rows = 64, (24, 24), 3, 4096
    sds = state_dicts(dim, hs, n, {}, gain=1.0)
    x = recipes.gaussian(841, rows, dim).to(DEV)
    w = (recipes.gaussian(842, rows, dim).to(DEV) / rows, recipes.gaussian(843, rows, 1)[:, 0].to(DEV) / rows)
    k_fwd, k_bwd, node, on = step(build(amd, dim, hs, n, {}, sds, True), x, "inverse", w, mid=1)
    assert k_fwd == "ahf_stack_rt" and k_bwd == "ahf_bwd_rt" and "_AffineRunFn" in node, (k_fwd, k_bwd, node)
    _, k_bwd, _, off = step(build(amd, dim, hs, n, {}, sds, False), x, "inverse", w, mid=1)
    assert k_bwd == "ahf_bwd_rt"
    same_gradients(amd, on, off, "cotangent on zs[1]")


def test_frozen_parameters_only_the_input_gradient(amd):
    """Only x wants a gradient: the launch goes out with grad_flats == NULL and leaves the x.grad of the same pass with
    trainable parameters, bit for bit; no parameter receives a gradient."""
    dim, hs, n, rows = 64, (24, 24), 3, 4096
    sds = state_dicts(dim, hs, n, {}, gain=1.0)
    x = recipes.gaussian(851, rows, dim).to(DEV)
    w = (recipes.gaussian(852, rows, dim).to(DEV) / rows, recipes.gaussian(853, rows, 1)[:, 0].to(DEV) / rows)
    for loss in ("nll", "inverse"):
        got = []
        for frozen in (True, False):
            model = build(amd, dim, hs, n, {}, sds, True)
            for p in model.parameters():
                p.requires_grad_(not frozen)
            k_fwd, k_bwd, node, g = step(model, x, loss, w)
            assert (k_fwd, k_bwd) == ("ahf_stack_rt", "ahf_bwd_stack_rt") and "_AffineRunFn" in node
            assert all((q.grad is None) == frozen for q in model.parameters())
            got.append(g["x"])
        same_bits(got[0], got[1], f"x.grad with frozen parameters, {loss}")


def test_flat_parameters_and_fused_adam(amd):
    """Parameters in a FlatParameters buffer: the gradient sums land in flat.grad in place, and the pass after a FusedAdam
    step reads the updated weights."""
    dim, hs, n, rows = 64, (24, 24), 3, 4096
    sds = state_dicts(dim, hs, n, {}, gain=1.0)
    x = recipes.gaussian(861, rows, dim).to(DEV)
    grads = []
    for switch in (True, False):
        model = build(amd, dim, hs, n, {}, sds, switch)
        opt = amd.FusedAdam(amd.FlatParameters(model), lr=1e-3)
        losses = []
        for it in range(3):
            opt.zero_grad()
            lp = model.log_prob(x)
            loss = -lp.mean()
            loss.backward()
            assert amd.last_kernel() == ("ahf_bwd_stack_rt" if switch else "ahf_bwd_rt")
            if it == 0:
                grads.append(opt.flat.grad.clone())
                assert float(grads[-1].abs().max()) > 0 and all(p.grad is not None for p in model.parameters())
            elif switch:  # this pass read the weights the step before it left: the no-grad launch on them, same bits
                with torch.no_grad():
                    same_bits(lp.detach(), model.log_prob(x), "log_prob after an optimiser step")
            opt.step()
            losses.append(float(loss.detach()))
        assert losses[2] < losses[1] < losses[0], losses
    # (the lp form: the run's one gradient scale is not the layers' own, see test_the_route -- same sums to 1e-6)
    assert_close(grads[0], grads[1], 1e-6, "flat.grad, switch on vs off")


def test_a_run_followed_by_another_layer(amd):
    """[run of three, NSF_CL]: log_prob meets the NSF_CL layer first, then the run closes the pass in its general form
    (cotangents on its last output AND on log_det); forward, the run opens the pass."""
    dim, hs, n, rows = 64, (24, 24), 3, 4096
    sds = state_dicts(dim, hs, n, {}, gain=1.0)
    x = recipes.gaussian(871, rows, dim, scale=0.7).to(DEV)
    w = (recipes.gaussian(872, rows, dim).to(DEV) / rows, recipes.gaussian(873, rows, 1)[:, 0].to(DEV) / rows)

    def model_of(switch):
        nsf = amd.NSF_CL(dim, K=8, B=3, n_h=8)
        nsf.load_state_dict(recipes.nsf_cl_params(42, dim, 8, 8))
        return build(amd, dim, hs, n, {}, sds, switch, tail=nsf)

    for loss in ("nll", "forward"):
        k_fwd, k_bwd, _, on = step(model_of(True), x, loss, w)
        # (the pass ends with the NSF_CL layer in one direction, with the run in the other)
        assert (k_fwd if loss == "nll" else k_bwd) == ("ahf_stack_rt" if loss == "nll" else "ahf_bwd_stack_rt"), (k_fwd, k_bwd)
        k_fwd, k_bwd, _, off = step(model_of(False), x, loss, w)
        assert (k_fwd if loss == "nll" else k_bwd) == ("ahf_rt" if loss == "nll" else "ahf_bwd_rt"), (k_fwd, k_bwd)
        for k in off:
            assert_close(on[k], off[k], 1e-6, f"run + NSF_CL {loss} {k}")


def test_fused_affine_stack_trains_on_the_route(amd):
    dim, hs, n, rows = 64, (24, 24), 3, 4096
    sds = state_dicts(dim, hs, n, {}, gain=1.0)
    x = recipes.gaussian(881, rows, dim).to(DEV)
    w = (recipes.gaussian(882, rows, dim).to(DEV) / rows, recipes.gaussian(883, rows, 1)[:, 0].to(DEV) / rows)
    k_fwd, k_bwd, _, on = step(build(amd, dim, hs, n, {}, sds, True, stack=True), x, "inverse", w)
    assert (k_fwd, k_bwd) == ("ahf_stack_rt", "ahf_bwd_stack_rt")
    k_fwd, k_bwd, _, off = step(build(amd, dim, hs, n, {}, sds, False, stack=True), x, "inverse", w)
    assert (k_fwd, k_bwd) == ("ahf_rt", "ahf_bwd_rt")
    same_bits(on["x"], off["x"], "FusedAffineStack x.grad")
    for k in off:
        if k != "x":
            (same_bits if amd.deterministic() else lambda p, q, s: assert_close(p, q, 1e-6, s))(on[k], off[k], k)


def test_graphed_training_step(amd):
    """One GraphedStep of -log_prob(x).mean() with the switch on: three replayed batches give the eager steps' losses
    and parameters (bit for bit under MNF_DETERMINISTIC=1; else the figures of test_hip_round6.py's graphed step)."""
    dim, hs, n, rows = 64, (24, 24), 3, 4096
    sds = state_dicts(dim, hs, n, {}, gain=1.0)

    def make():
        model = build(amd, dim, hs, n, {}, sds, True)
        return model, amd.FusedAdam(amd.FlatParameters(model), lr=1e-3, capturable=True)

    batches = [recipes.gaussian(890 + i, rows, dim).to(DEV) for i in range(4)]
    model_e, opt_e = make()
    losses_e = []
    for x in [batches[0]] * 3 + batches[1:]:
        opt_e.zero_grad()
        loss = -model_e.log_prob(x).mean()
        assert amd.last_kernel() == "ahf_stack_rt"
        loss.backward()
        assert amd.last_kernel() == "ahf_bwd_stack_rt"
        opt_e.step()
        losses_e.append(float(loss.detach()))
    del loss
    model_g, opt_g = make()
    graphed = amd.GraphedStep(opt_g, lambda x: -model_g.log_prob(x).mean(), batches[0])
    losses_g = [float(graphed(x)) for x in batches[1:]]
    if amd.deterministic():
        assert losses_g == losses_e[3:], (losses_g, losses_e[3:])
        same_bits(opt_g.flat.data, opt_e.flat.data, "parameters after the replayed steps")
    else:
        for a, b in zip(losses_e[3:], losses_g):
            assert abs(a - b) <= 2e-4 * max(1.0, abs(a)), (a, b)
        assert_close(opt_g.flat.data, opt_e.flat.data, 2e-3, "parameters after the replayed steps")
