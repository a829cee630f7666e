"""Fixture G17 (the reference's own autograd gradients, tests/golden/g17_cases.py) from the tests' side: the oracle's
gradients of the same losses, the fixture's arrays per case, the HIP modules of a case, and the shapes of every
reference-fixture test that runs on the run-time-shaped tier (tests/test_rt_golden_host.py asks the library's own
queries about them).  Shared by tests/test_oracle_golden.py, tests/test_rt_golden_host.py, tests/test_hip_rt_golden.py
and tests/rt_deterministic_child.py."""
from __future__ import annotations

import torch

import g17_cases as C
import recipes
from helpers import t
from oracle import flow_oracle as O

DEV = "cuda"
SINGLE_TAGS = [tag for kind in C.SINGLE_LAYER_KINDS for tag in C.KINDS[kind]]
RUN_TAG, BLOCK_TAG = next(iter(C.RUN)), next(iter(C.BLOCK))


def fixture_grads(golden, tag):
    """({name: fp32 gradient}, {name: float64 gradient}, loss, loss64) of the reference, as CPU tensors"""
    fx = golden(C.part_of(tag))
    names = C.grad_names(tag)
    return ({k: t(fx[f"{tag}.grad.{k}"]) for k in names}, {k: t(fx[f"{tag}.grad64.{k}"]).double() for k in names},
            float(fx[f"{tag}.loss"]), float(fx[f"{tag}.loss64"]))


def _leaf(sd, dt):
    return {k: (v.to(dt) if k == "P" else v.to(dt).clone().requires_grad_(True)) for k, v in sd.items()}


def oracle_grads(tag, dt):
    """(loss, {name: gradient}) by torch.autograd through the CPU oracle in dtype ``dt``, names as the fixture's"""
    kind, inp, p = C.kind_of(tag), C.inputs(tag), C.params(tag)
    spec = C.KINDS[kind][tag]
    x = inp["x"].to(dt).requires_grad_(True)
    if kind in C.SINGLE_LAYER_KINDS:
        q = _leaf(p, dt)
        if kind == "ahf":
            _, _, kw, parity, inverse = spec
            y, ld = O.affine_half(x, q, parity, inverse, **kw)
        elif kind == "nsf":
            y, ld = O.nsf_cl(x, q, spec[1], 3.0, spec[3])
        elif kind == "rnvp":
            y, ld = O.rnvp(x, q, inp["mask"].to(dt))
        else:
            y, ld = O.glow(x, q["P"], q["L"], q["S"], q["U"], spec[1])
        loss = (y * inp["w_y"].to(dt)).sum() + (ld * inp["w_l"].to(dt)).sum()
        named = {k: v for k, v in q.items() if k != "P"}
    else:
        qs = [_leaf(sd, dt) for sd in p]
        zs, ld = O.flow_stack(x, oracle_layers(tag, qs), inverse=True)
        loss = -(O.std_normal_log_prob(zs[-1]) + ld).mean()
        named = {f"flows.{i}.{k}": v for i, q in enumerate(qs) for k, v in q.items() if k != "P"}
    loss.backward()
    grads = {"x": x.grad, **{k: v.grad for k, v in named.items()}}
    assert list(grads) == C.grad_names(tag)
    return float(loss.detach()), grads


def oracle_layers(tag, qs):
    if C.kind_of(tag) == "run":
        return [{"kind": "affine_half", "parity": bool(i % 2), "params": q} for i, q in enumerate(qs)]
    _, K, _ = C.BLOCK[tag]
    return [{"kind": "affine_const", "params": qs[0]}, {"kind": "glow", "params": qs[1]},
            {"kind": "nsf_cl", "K": K, "B": 3.0, "params": qs[2]}]


# --------------------------------------------------------------------------------------------------- the HIP side
def _glow(amd, gp, dim):
    gl = amd.Glow(dim)
    gl.P = gp["P"]
    gl.load_state_dict({k: gp[k] for k in ("L", "S", "U")})
    return gl


def hip_module(amd, tag, force):
    """The case's layer (or model) on the GPU, every layer with ``force_generic = force``"""
    kind, p = C.kind_of(tag), C.params(tag)
    spec = C.KINDS[kind][tag]
    if kind == "ahf":
        dim, hs, kw, parity, _ = spec
        m = amd.AffineHalfFlow(dim, parity, h_sizes=hs, **kw)
        m.load_state_dict(p)
    elif kind == "nsf":
        dim, K, n_h, _ = spec
        m = amd.NSF_CL(dim, K=K, B=3, n_h=n_h)
        m.load_state_dict(p)
    elif kind == "rnvp":
        m = amd.RNVP(spec[0], h_sizes=spec[1])
        m.load_state_dict(p)
    elif kind == "glow":
        m = _glow(amd, p, spec[0])
    elif kind == "run":
        dim, hs, _ = spec
        flows = []
        for i, sd in enumerate(p):
            f = amd.AffineHalfFlow(dim, bool(i % 2), h_sizes=hs)
            f.load_state_dict(sd)
            flows.append(f)
        m = amd.NormalizingFlowModel(amd.StandardNormal(dim), flows)
    else:
        dim, K, n_h = spec
        an = amd.ActNormFlow(dim)
        an.load_state_dict(p[0])
        an.data_dep_init_done = True
        sp = amd.NSF_CL(dim, K=K, B=3, n_h=n_h)
        sp.load_state_dict(p[2])
        m = amd.NormalizingFlowModel(amd.StandardNormal(dim), [an, _glow(amd, p[1], dim), sp])
    for f in (m.flows if hasattr(m, "flows") else [m]):
        f.force_generic = force
    return m.to(DEV)


def hip_layer_grads(amd, tag, m):
    """Gradients of the single-layer loss through the HIP module ``m``: ({name: gradient}, kernel family of the last
    launch -- the gradient kernel's)"""
    kind, inp = C.kind_of(tag), C.inputs(tag)
    x = inp["x"].to(DEV).requires_grad_(True)
    if kind == "rnvp":
        y, ld = m.forward(x, mask=inp["mask"].to(DEV))
    else:
        y, ld = (m.inverse if C.KINDS[kind][tag][-1] else m.forward)(x)
    ((y * inp["w_y"].to(DEV)).sum() + (ld * inp["w_l"].to(DEV)).sum()).backward()
    torch.cuda.synchronize()
    return {"x": x.grad, **{k: q.grad for k, q in m.named_parameters()}}, amd.last_kernel()


# ---------------------------------------------------------------- every shape the reference fixtures put on the rt tier
def ahf_shapes():
    """(what, dim, h_sizes, scale, shift, layers in a run or 0, gradients wanted) of every AffineHalfFlow that
    tests/test_hip_parity.py's "rt" parametrisations and tests/test_hip_rt_golden.py force onto the run-time-shaped tier"""
    out = [(f"g2 d{d}", d, (24, 24, 24), True, True, 0, False) for d in (64, 256)]
    out += [(f"g2 {tag}", 10, kw.get("h_sizes", (24, 24, 24)), kw.get("scale", True), kw.get("shift", True), 0, False)
            for tag, kw in (("nice", dict(scale=False)), ("noshift", dict(shift=False)), ("h2", dict(h_sizes=(16, 40))),
                            ("h1", dict(h_sizes=(7,))))]
    out += [(f"g10 {tag}", dim, kw.get("h_sizes", (24, 24, 24)), kw.get("scale", True), kw.get("shift", True), 0, False)
            for tag, (dim, kw) in recipes.G10_AHF.items()]
    out += [("g1", 2, (24, 24, 24), True, True, 9, False), ("g3 d64", 64, (24, 24, 24), True, True, 9, False),
            ("g3 d256", 256, (24, 24, 24), True, True, 9, False), ("g9", 4, (24, 24, 24), True, True, 0, False)]
    out += [(tag, dim, hs, kw.get("scale", True), kw.get("shift", True), 0, True) for tag, (dim, hs, kw, _, _) in C.AHF.items()]
    out += [(tag, dim, hs, True, True, n, True) for tag, (dim, hs, n) in C.RUN.items()]
    return out


def nsf_shapes():
    """(what, dim, K, n_h, gradients wanted)"""
    out = [(f"g5 d{d}_K{K}_h{n_h}", d, K, n_h, False) for d, K, n_h in ((32, 8, 8), (32, 8, 16), (2, 8, 16), (6, 5, 8))]
    out += [("g6", 32, 8, 8, False), ("g9", 4, 5, 8, False)]
    out += [(tag, dim, K, n_h, True) for tag, (dim, K, n_h, _) in C.NSF.items()]
    out += [(tag, dim, K, n_h, True) for tag, (dim, K, n_h) in C.BLOCK.items()]
    return out


def rnvp_shapes():
    """(what, dim, h_sizes, gradients wanted)"""
    out = [(f"g7 d{d}", d, (50,), False) for d in (50, 800, 784)]
    out += [(f"g10 {tag}", dim, (hid,), False) for tag, (dim, hid) in recipes.G10_RNVP.items()]
    out += [("g9", 4, (30,), False)]
    out += [(tag, dim, hs, True) for tag, (dim, hs) in C.RNVP.items()]
    return out


def glow_dims():
    """(what, dim) of every Glow on linear_rows_rt"""
    return [("g6", 32), ("g9", 4)] + [(tag, dim) for tag, (dim, _) in C.GLOW.items()] + [(tag, spec[0]) for tag, spec in C.BLOCK.items()]


# ------------------------------------------------------------------------- gradient checks shared with the child process
class _Families(list):
    """the names in order; ``fresh``: without the leading entries that repeat the name the library reported BEFORE the
    block (a call that launches no named kernel leaves mnf_last_kernel's answer as it was: those entries are stale)"""

    def __init__(self):
        super().__init__()
        self.fresh = []


class recorded_families:
    """``with recorded_families(amd) as seen``: the kernel family behind every library call inside the block, in order
    (the ``families`` fixture of tests/test_hip_glow_actnorm_rt.py for code that has no fixtures).  Ask ``seen`` whether a
    family ran, ``seen.fresh`` whether one did NOT (see _Families)."""

    def __init__(self, amd):
        self.lib, self.amd, self.seen = amd._lib, amd, _Families()

    def __enter__(self):
        self.check = self.lib.check
        stale = self.amd.last_kernel()

        def recording_check(name, rc):
            k = self.amd.last_kernel()
            self.seen.append(k)
            if self.seen.fresh or k != stale:
                self.seen.fresh.append(k)
            return self.check(name, rc)

        self.lib.check = recording_check
        return self.seen

    def __exit__(self, *exc):
        self.lib.check = self.check
        return False


BWD_RT_FAMILY = {"ahf": "ahf_bwd_rt", "nsf": "nsf_bwd_rt", "rnvp": "rnvp_bwd_rt"}
FWD_RT_FAMILY = {"ahf": "ahf_rt", "nsf": "nsf_rt", "rnvp": "rnvp_rt"}
TIER_NAME = {0: "default", 1: "valu", 2: "rt"}
def record(tier, family, what, err, budget):
    """one line per comparison of tests/test_hip_rt_golden.py (pytest -s): profiles/r12/rt_golden.txt"""
    print(f"rt_golden  {tier:8s} {family:28s} err {err:9.2e}  budget {budget:9.2e}  used {100 * err / budget:5.1f} %  {what}")


def check_grads(got, golden, tag, tier, family, prefix=""):
    """Every gradient of the case against the fixture with tests/test_hip_autograd.py's check_vs_float64 rule: GBASE plus
    twice the fixture's own fp32-vs-float64 distance, measured against the reference's float64 gradient."""
    from helpers import GRAD_LOG
    from test_hip_autograd import check_vs_float64

    g32, g64, _, _ = fixture_grads(golden, tag)
    assert list(got) == list(g32), (list(got), list(g32))
    for k in g32:
        assert got[k] is not None and got[k].shape == g32[k].shape, (tag, k)
        try:
            check_vs_float64(got[k], g32[k], g64[k], f"{prefix}g17 {tag} [{tier}: {family}] grad {k}")
        finally:
            r = GRAD_LOG[-1]
            record(tier, family, f"{prefix}{tag} grad {k}", r["err"], r["budget"])


def layer_case(amd, golden, tag, force, prefix=""):
    """One single-layer case of G17 on the tier ``force`` names; returns the families of the pass"""
    kind = C.kind_of(tag)
    m = hip_module(amd, tag, force)
    with recorded_families(amd) as seen:
        got, last = hip_layer_grads(amd, tag, m)
    if force == 2 and kind != "glow":
        assert last == BWD_RT_FAMILY[kind] and FWD_RT_FAMILY[kind] in seen, (tag, last, seen)
    if force == 1:
        assert all("generic" in k or not k.startswith(("ahf", "nsf", "rnvp")) for k in seen.fresh), (tag, seen.fresh)
    if kind == "glow":
        assert {"linear_rows_rt", "linear_rows_bwd_weight_rt"} <= set(seen), (tag, seen)
        last = "linear_rows_rt+bwd_weight_rt"
    check_grads(got, golden, tag, TIER_NAME[force], last, prefix)
    return seen


def run_case(amd, golden, fused, prefix=""):
    """The 4-layer AffineHalfFlow run of G17 under -mean log p, every layer on the run-time-shaped tier: layer by layer
    (ahf_rt / ahf_bwd_rt per layer) or, with fuse_rt_training, as one autograd node (ahf_stack_rt / ahf_bwd_stack_rt,
    the last layer's cotangents formed in the kernel)."""
    tag = RUN_TAG
    model = hip_module(amd, tag, 2)
    model.fuse_rt_training = fused
    x = C.inputs(tag)["x"].to(DEV).requires_grad_(True)
    with recorded_families(amd) as seen:
        if fused:
            loss = -model.log_prob(x).mean()
        else:
            zs, ld = model.inverse(x)
            loss = -(model.base.log_prob(zs[-1]) + ld).mean()
        loss.backward()
        torch.cuda.synchronize()
    want = {"ahf_stack_rt", "ahf_bwd_stack_rt"} if fused else {"ahf_rt", "ahf_bwd_rt"}
    # (one node: the gradient scales come from walking at most 512 sample rows through the layers first, n - 1 small
    #  grad_x-only ahf_bwd_rt launches -- flows._rt_layer_scales -- before the ONE ahf_bwd_stack_rt launch)
    allowed = want | ({"ahf_bwd_rt"} if fused else set())
    assert want <= set(seen) and {k for k in seen.fresh if k.startswith("ahf")} <= allowed, (seen, sorted(want))
    assert not fused or seen.count("ahf_bwd_stack_rt") == 1, seen
    assert amd.last_kernel() == ("ahf_bwd_stack_rt" if fused else "ahf_bwd_rt")
    got = {"x": x.grad, **{k: q.grad for k, q in model.named_parameters()}}
    check_grads(got, golden, tag, "rt", "ahf_bwd_stack_rt" if fused else "ahf_bwd_rt", prefix)
    return float(loss.detach())
