#!/usr/bin/env python3
"""Launch transcript of the Python host path: every library entry a fixed script of layer calls reaches, in order.

After ``_lib.load()`` the loaded library (``torch_mnf_amd._lib._lib``) is swapped for a forwarding proxy.  For every call
it writes one line: the entry's name, its integer and float arguments, ``ptr`` / ``null`` for each pointer argument, the
contents of the small int arrays handed IN (hidden sizes, parities; an ``*_index`` entry's table is an output: its length)
and the value the entry returned (the status code, or a count -- which is how the element count of every workspace shows:
as the answer of its ``*_workspace`` query and again as the count argument next to the workspace pointer).  No address and no
stream handle is written.  After every layer call a ``=`` line holds ``last_kernel()``; an exception is a ``!`` line.

The script covers every flow class and MNFLinear / MNFConv2d, under no_grad and with backward(), with force_generic 0 / 1 /
2, with and without accum (a two-layer NormalizingFlow), the fp32 request, row counts on both sides of every row constant
flows.py reads from _dispatch, the smallest shape of each tier, and each opt-in route opened once.  Two versions of the
Python package on the same built library must give the same transcript; table queries (the ``?`` lines: pure host
functions that build an index table, no launch) are marked so that a comparison can tell them from launches:

    python tools/launch_transcript.py --out new.txt
    PYTHONPATH=/path/to/other/package/parent MNF_LIB_PATH=.../libmnf_hip.so python tools/launch_transcript.py --out old.txt
    python tools/launch_transcript.py --diff old.txt new.txt

``--diff`` prints the differing lines, the table-query counts per entry, and both transcripts in short (per group of layer
calls: launches and queries of each side, a hash of each side's lines, the kernels that ran) -- the record to keep.
"""
from __future__ import annotations

import argparse
import ctypes
import difflib
import hashlib
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if not os.environ.get("PYTHONPATH"):  # (PYTHONPATH set: the package to record is the one it names)
    sys.path.insert(0, ROOT)

SILENT = {"mnf_last_kernel", "mnf_deterministic", "mnf_error_string", "mnf_last_hip_error", "mnf_abi_version"}
QUERY_ENDS = ("_index", "_layout", "_image_floats", "_index_ints", "_flat_floats")


def is_query(name: str) -> bool:
    return name.endswith(QUERY_ENDS)


class Proxy:
    """Forwards every attribute to the library; calls of its entries are written to ``lines`` first."""

    def __init__(self, real, signatures, lines):
        self.__dict__.update(_real=real, _sig=signatures, _lines=lines, _made={})

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name in SILENT or name not in self._sig:
            return fn
        wrapped = self._made.get(name)
        if wrapped is None:
            argtypes = self._sig[name][1]

            def wrapped(*args, _fn=fn, _name=name, _types=argtypes):
                shown = [self._show(_name, a, t) for a, t in zip(args, _types)]
                out = _fn(*args)
                self._lines.append(f"{'?' if is_query(_name) else ' '} {_name}({', '.join(shown)}) -> {out}")
                return out
            self._made[name] = wrapped
        return wrapped

    @staticmethod
    def _show(name, arg, argtype) -> str:
        if isinstance(arg, ctypes.Array):
            return f"out[{len(arg)}]" if name.endswith("_index") else "[" + " ".join(str(int(v)) for v in arg) + "]"
        if argtype is ctypes.c_void_p or (isinstance(argtype, type) and issubclass(argtype, ctypes._Pointer)):
            if arg is None or (isinstance(arg, int) and arg == 0):
                return "null"
            return "ptr" if isinstance(arg, int) else "out"
        if argtype in (ctypes.c_float, ctypes.c_double):
            return repr(float(arg))
        return str(int(arg))


def record(out_path: str) -> None:
    import torch

    import torch_mnf_amd as amd
    from torch_mnf_amd import _dispatch, _lib, flows

    real = _lib.load()
    print("package:", os.path.dirname(os.path.abspath(amd.__file__)))
    lines: list[str] = []
    _lib._lib = Proxy(real, _lib.SIGNATURES, lines)
    dev = torch.device("cuda")
    RT, SPLIT, PAD = _dispatch.RT_MIN_ROWS, _dispatch.BWD_SPLIT_MIN_ROWS, _dispatch.NSF_PAD_MIN_ROWS
    ROWS = (1, 128, RT - 1, RT, 4096, SPLIT)

    def step(label, fn):
        lines.append(f"# {label}")
        try:
            fn()
        except Exception as err:  # noqa: BLE001 (an error path is part of the transcript)
            lines.append(f"! {type(err).__name__}: {' '.join(str(err).split())[:120]}")
        lines.append(f"= {(real.mnf_last_kernel() or b'').decode()}")

    def data(rows, dim, grad=False):
        g = torch.Generator(device="cpu").manual_seed(rows * 131 + dim)
        x = (0.5 * torch.randn(rows, dim, generator=g)).to(dev)
        return x.requires_grad_(True) if grad else x

    def both_ways(name, layer, dim, rows, two_way=True):
        for inverse in ((False, True) if two_way else (False,)):
            way = "inverse" if inverse else "forward"
            call = (lambda x: layer.inverse(x)) if inverse else (lambda x: layer.forward(x))

            def plain():
                with torch.no_grad():
                    call(data(rows, dim))

            def train():
                y, ld = call(data(rows, dim, grad=True))
                (y.sum() + ld.sum()).backward()
            step(f"{name} rows={rows} {way} no_grad", plain)
            step(f"{name} rows={rows} {way} backward", train)

    def sweep(name, make, dim, two_way=True, rows=ROWS):
        torch.manual_seed(0)
        layer = make().to(dev)
        for r in rows:
            both_ways(name, layer, dim, r, two_way)
        for force in (1, 2):
            layer.force_generic = force
            for r in (128, 4096):
                both_ways(f"{name} force_generic={force}", layer, dim, r, two_way)
        layer.force_generic = 0
        return layer

    # ---- every class, the smallest shape of each tier, rows on both sides of every row constant
    sweep("AHF d=64 h=(24,24,24)", lambda: amd.AffineHalfFlow(64, False), 64)
    ahf6 = sweep("AHF d=6 h=(16,16)", lambda: amd.AffineHalfFlow(6, True, h_sizes=(16, 16)), 6)
    sweep("AHF d=6 h=(128,)", lambda: amd.AffineHalfFlow(6, False, h_sizes=(128,)), 6)
    sweep("AHF d=6 h=(2,) scale only", lambda: amd.AffineHalfFlow(6, False, h_sizes=(2,), shift=False), 6, rows=(128, 4096))
    sweep("NSF_CL d=32 K=8", lambda: amd.NSF_CL(32, K=8), 32)
    sweep("NSF_CL d=2", lambda: amd.NSF_CL(2), 2, rows=(1, 128, RT, PAD - 1, PAD))
    sweep("NSF_CL d=6 K=5", lambda: amd.NSF_CL(6, K=5), 6, rows=(128, RT, PAD))
    sweep("RNVP d=128 h=(50,)", lambda: amd.RNVP(128, (50,)), 128, two_way=False)
    sweep("RNVP d=6 h=(16,)", lambda: amd.RNVP(6, (16,)), 6, two_way=False, rows=(1, 2, 128, 4096))
    sweep("MAF d=6 h=(16,16)", lambda: flows.MAF(6, False, h_sizes=(16, 16)), 6, rows=(1, 128, RT - 1, RT, 4096))
    sweep("IAF d=6 h=(16,16)", lambda: flows.IAF(6, True, h_sizes=(16, 16)), 6, rows=(128, RT))
    sweep("NSF_AR d=6 K=5", lambda: amd.NSF_AR(6, K=5), 6, rows=(1, 128, RT - 1, RT, 4096))
    sweep("Glow d=32", lambda: amd.Glow(32), 32, rows=ROWS + (_dispatch.GLOW_RT_MIN_ROWS,))
    sweep("Glow d=48", lambda: amd.Glow(48), 48, rows=ROWS + (_dispatch.GLOW_RT_MIN_ROWS,))
    sweep("AffineConstantFlow d=6", lambda: amd.AffineConstantFlow(6), 6, rows=(1, 128, 4096))
    sweep("ActNormFlow d=6", lambda: amd.ActNormFlow(6), 6, rows=(128, 4096))

    # ---- error paths and the empty batch: the order the checks fire in
    for name, layer in (("AHF", ahf6), ("NSF_AR", amd.NSF_AR(6).to(dev)), ("MAF", flows.MAF(6, False, h_sizes=(16, 16)).to(dev))):
        for label, x in (("wrong dim", lambda: data(8, 4)), ("cpu", lambda: torch.zeros(8, 6)), ("empty", lambda: data(0, 6)),
                         ("float64", lambda: data(8, 6).double()), ("wrong dim, grad", lambda: data(8, 4, grad=True))):
            step(f"{name} {label}", lambda layer=layer, x=x: layer.inverse(x()))
    maf_perm = flows.MAF(6, False, net=flows.MADE(6, (16, 16), 12, natural_ordering=False)).to(dev)
    step("MAF permuted order, sequential, grad", lambda: maf_perm.forward(data(8, 6, grad=True)))
    step("MAF permuted order, sequential, grad, wrong dim", lambda: maf_perm.forward(data(8, 4, grad=True)))

    # ---- the fp32 request on one coupling layer
    for name, make, dim in (("AHF d=64", lambda: amd.AffineHalfFlow(64, False), 64), ("AHF d=6", lambda: amd.AffineHalfFlow(6, False, h_sizes=(16, 16)), 6),
                            ("NSF_CL d=32 K=8", lambda: amd.NSF_CL(32, K=8), 32)):
        torch.manual_seed(0)
        layer = make().to(dev)
        layer.force_fp32_mfma = True
        for r in (128, 4096, SPLIT):
            both_ways(f"{name} fp32 request", layer, dim, r)

    # ---- with and without accum: NormalizingFlow / NormalizingFlowModel, runs, blocks and pairs
    def model_steps(name, flows_of, dim, rows=(128, 4096, SPLIT), **switches):
        torch.manual_seed(0)
        model = amd.NormalizingFlowModel(amd.StandardNormal(dim, dev), flows_of()).to(dev)
        for k, v in switches.items():
            setattr(model, k, v)
        for r in rows:
            def plain():
                with torch.no_grad():
                    model.inverse(data(r, dim))
                    model.forward(data(r, dim))
                    model.log_prob(data(r, dim), return_sum=True)

            def train():
                model.zero_grad()
                (-model.log_prob(data(r, dim)).mean()).backward()
                zs, ld = model.forward(data(r, dim, grad=True))
                (zs[-1].sum() + ld.sum()).backward()
            step(f"model {name} rows={r} no_grad", plain)
            step(f"model {name} rows={r} backward", train)
        return model

    model_steps("2xAHF d=64", lambda: [amd.AffineHalfFlow(64, i % 2 == 1) for i in range(2)], 64)
    model_steps("2xAHF d=64 unfused", lambda: [amd.AffineHalfFlow(64, i % 2 == 1) for i in range(2)], 64, fuse_affine_runs=False)
    model_steps("3xAHF d=6 h=(16,16)", lambda: [amd.AffineHalfFlow(6, i % 2 == 1, h_sizes=(16, 16)) for i in range(3)], 6)
    model_steps("3xAHF d=6 h=(16,16) fuse_rt_training", lambda: [amd.AffineHalfFlow(6, i % 2 == 1, h_sizes=(16, 16)) for i in range(3)], 6,
                fuse_rt_training=True)
    model_steps("[AHF, NSF_CL] d=32", lambda: [amd.AffineHalfFlow(32, False), amd.NSF_CL(32, K=8)], 32)
    model_steps("[ActNorm, Glow, NSF_CL] d=32 K=8", lambda: [amd.ActNormFlow(32), amd.Glow(32), amd.NSF_CL(32, K=8)], 32)
    model_steps("[ActNorm, Glow, NSF_CL] d=6", lambda: [amd.ActNormFlow(6), amd.Glow(6), amd.NSF_CL(6)], 6, rows=(128, 4096))
    model_steps("[MAF, NSF_AR, AffineConstantFlow] d=6", lambda: [flows.MAF(6, False, h_sizes=(16, 16)), amd.NSF_AR(6), amd.AffineConstantFlow(6)], 6,
                rows=(128, 4096))
    model_steps("FusedAffineStack 3xAHF d=64", lambda: [amd.FusedAffineStack([amd.AffineHalfFlow(64, i % 2 == 1) for i in range(3)])], 64)
    model_steps("FusedSplineBlock d=32 K=8", lambda: [amd.FusedSplineBlock(amd.ActNormFlow(32), amd.Glow(32), amd.NSF_CL(32, K=8))], 32,
                rows=(128, 4096))
    torch.manual_seed(0)
    rn = amd.NormalizingFlow([amd.RNVP(128, (50,)), amd.RNVP(128, (50,))]).to(dev)
    for r in (1, 128, 4096):
        def plain():
            with torch.no_grad():
                rn.forward(data(r, 128))

        def train():
            zs, ld = rn.forward(data(r, 128, grad=True))
            (zs[-1].sum() + ld.sum()).backward()
        step(f"model 2xRNVP d=128 rows={r} no_grad", plain)
        step(f"model 2xRNVP d=128 rows={r} backward", train)
    step("rqs", lambda: flows.rqs(data(64, 1).reshape(-1), data(64, 5), data(64, 5) + 1, data(64, 4)))

    # ---- each opt-in route opened once
    saved = {k: getattr(_dispatch, k) for k in ("MAF_SEQ_BWD_RT_MIN_ROWS", "NSF_AR_RT_MIN_ROWS", "NSF_AR_BWD_RT_MIN_ROWS",
                                               "NSF_AR_SEQ_RT_MIN_ROWS", "AHF_BWD_RT_WIDE_MIN_ROWS", "GLOW_ACTNORM_RT",
                                               "MNF_CONV_FUSED", "NO_FUSED_LOGPROB", "BWD_FP32", "NSF_BWD_KERNEL",
                                               "RNVP_BWD_GENERIC", "RNVP_BWD_FEW_GRID_OFF")}

    def opened(const, value, name, make, dim, rows=(RT, 4096), two_way=True):
        setattr(_dispatch, const, value)
        torch.manual_seed(0)
        layer = make().to(dev)
        for r in rows:
            both_ways(f"{name} with {const}={value}", layer, dim, r, two_way)
        setattr(_dispatch, const, saved[const])

    opened("MAF_SEQ_BWD_RT_MIN_ROWS", 0, "MAF d=6", lambda: flows.MAF(6, False, h_sizes=(16, 16)), 6)
    opened("NSF_AR_RT_MIN_ROWS", 0, "NSF_AR d=6", lambda: amd.NSF_AR(6, K=5), 6)
    opened("NSF_AR_BWD_RT_MIN_ROWS", 0, "NSF_AR d=6", lambda: amd.NSF_AR(6, K=5), 6)
    opened("NSF_AR_SEQ_RT_MIN_ROWS", 0, "NSF_AR d=6", lambda: amd.NSF_AR(6, K=5), 6)
    opened("AHF_BWD_RT_WIDE_MIN_ROWS", 0, "AHF d=6 h=(128,)", lambda: amd.AffineHalfFlow(6, False, h_sizes=(128,)), 6)
    opened("BWD_FP32", True, "AHF d=64", lambda: amd.AffineHalfFlow(64, False), 64, rows=(SPLIT,))
    opened("NSF_BWD_KERNEL", "generic", "NSF_CL d=32 K=8", lambda: amd.NSF_CL(32, K=8), 32, rows=(4096,))
    opened("RNVP_BWD_GENERIC", True, "RNVP d=128", lambda: amd.RNVP(128, (50,)), 128, rows=(128, 4096), two_way=False)
    opened("RNVP_BWD_FEW_GRID_OFF", True, "RNVP d=128", lambda: amd.RNVP(128, (50,)), 128, rows=(128, 4096), two_way=False)
    _dispatch.GLOW_ACTNORM_RT = True
    model_steps("[ActNorm, Glow] d=48 with GLOW_ACTNORM_RT", lambda: [amd.ActNormFlow(48), amd.Glow(48)], 48, rows=(4096, _dispatch.GLOW_RT_MIN_ROWS))
    _dispatch.GLOW_ACTNORM_RT = saved["GLOW_ACTNORM_RT"]
    _dispatch.NO_FUSED_LOGPROB = True
    model_steps("2xAHF d=64 with NO_FUSED_LOGPROB", lambda: [amd.AffineHalfFlow(64, i % 2 == 1) for i in range(2)], 64, rows=(SPLIT,))
    _dispatch.NO_FUSED_LOGPROB = saved["NO_FUSED_LOGPROB"]

    # ---- the MNF layers, both directions; the conv layer's fused forward opened once
    def mnf_steps(name, layer, x_of):
        def plain():
            with torch.no_grad():
                layer(x_of())
                layer.kl_div()

        def train():
            layer.zero_grad()
            (layer(x_of().requires_grad_(True)).sum() + layer.kl_div()).backward()
        step(f"{name} no_grad", plain)
        step(f"{name} backward", train)
        step(f"{name} backward again", train)

    torch.manual_seed(0)
    for n_in, n_out in ((20, 10), (800, 50), (12, 70)):
        lin = amd.MNFLinear(n_in, n_out).to(dev)
        for r in (1, 128):
            mnf_steps(f"MNFLinear({n_in},{n_out}) rows={r}", lin, lambda r=r, n_in=n_in: data(r, n_in))
    conv = amd.MNFConv2d(1, 20, 5).to(dev)
    mnf_steps("MNFConv2d(1,20,5)", conv, lambda: data(8, 28 * 28).reshape(8, 1, 28, 28))
    _dispatch.MNF_CONV_FUSED = True
    mnf_steps("MNFConv2d(1,20,5) with MNF_CONV_FUSED", conv, lambda: data(8, 28 * 28).reshape(8, 1, 28, 28))
    _dispatch.MNF_CONV_FUSED = saved["MNF_CONV_FUSED"]

    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)) or ".", exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(f"# package: {'MNF_DETERMINISTIC=1' if _lib.deterministic() else 'atomic sums'}, "
                 f"{sum(1 for ln in lines if ln[0] == ' ')} calls, {sum(1 for ln in lines if ln[0] == '?')} table queries\n")
        fh.write("\n".join(lines) + "\n")
    print(f"{out_path}: {len(lines)} lines")


def diff(old_path: str, new_path: str) -> int:
    """Line-for-line comparison; returns the number of differing launch / result lines outside the table queries.  The
    table queries are compared as counts per entry: a host cache that asks the library less often shows there."""
    old, new = (open(p).read().splitlines()[1:] for p in (old_path, new_path))
    # the one renaming both sides may show: mnf_affine_half(x, y, ld, ...) IS mnf_affine_half_sq(x, y, ld, null, ...)
    # (csrc/mnf_generic.hip), so both spellings are compared as the latter
    plain, renamed = "  mnf_affine_half(ptr, ptr, ptr, ", "  mnf_affine_half_sq(ptr, ptr, ptr, null, "
    for side, ls in (("old", old), ("new", new)):
        hits = [i for i, ln in enumerate(ls) if ln.startswith(plain)]
        for i in hits:
            ls[i] = renamed + ls[i][len(plain):]
        print(f"{side}: {len(hits)} mnf_affine_half calls read as mnf_affine_half_sq with a null y_sqnorm")
    strip = lambda ls: [ln for ln in ls if not ln.startswith("?")]  # noqa: E731
    delta = [ln for ln in difflib.unified_diff(strip(old), strip(new), old_path, new_path, lineterm="", n=1)]
    changed = [ln for ln in delta if ln[:1] in "+-" and ln[:3] not in ("+++", "---")]
    print(f"launches, results and last_kernel lines: {len(strip(old))} old, {len(strip(new))} new, {len(changed)} differing")
    print("\n".join(delta))
    count = lambda ls: {n: sum(1 for ln in ls if ln.startswith("? " + n + "(")) for n in sorted({ln[2:].split("(")[0] for ln in ls if ln.startswith("?")})}  # noqa: E731
    c_old, c_new = count(old), count(new)
    print(f"table queries: {sum(c_old.values())} old, {sum(c_new.values())} new")
    for n in sorted(set(c_old) | set(c_new)):
        if c_old.get(n, 0) != c_new.get(n, 0):
            print(f"  {n}: {c_old.get(n, 0)} -> {c_new.get(n, 0)}")
    # both transcripts in short: per group of layer calls (a label without its row count, direction and mode) the number
    # of calls, of launch lines and of table queries, a hash of everything but the queries, and the kernels that ran
    print(f"\n{'group':58s} calls  launches old/new  queries old/new  sha1 old     sha1 new     kernels")
    g_old, g_new = _groups(old), _groups(new)
    for key in dict.fromkeys(list(g_old) + list(g_new)):
        a, b = g_old.get(key, _EMPTY), g_new.get(key, _EMPTY)
        print(f"{key:58s} {b['calls']:5d}  {a['launches']:7d} {b['launches']:7d}  {a['queries']:7d} {b['queries']:7d}  "
              f"{a['sha'].hexdigest()[:10]}   {b['sha'].hexdigest()[:10]}   {' '.join(sorted(b['kernels'] - {''}))}")
    return len(changed)


_EMPTY = {"calls": 0, "launches": 0, "queries": 0, "sha": hashlib.sha1(), "kernels": set()}


def _groups(lines) -> dict:
    out, cur = {}, None
    for ln in lines:
        if ln.startswith("# "):
            key = re.sub(r"( rows=\d+)?( (forward|inverse))?( (no_grad|backward( again)?))?$", "", ln[2:])
            cur = out.setdefault(key, {"calls": 0, "launches": 0, "queries": 0, "sha": hashlib.sha1(), "kernels": set()})
            cur["calls"] += 1
        elif ln.startswith("?"):
            cur["queries"] += 1
            continue
        elif ln.startswith("= "):
            cur["kernels"].add(ln[2:])
        elif ln.startswith("  "):
            cur["launches"] += 1
        cur["sha"].update(ln.encode() + b"\n")
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="launch_transcript.txt")
    ap.add_argument("--diff", nargs=2, metavar=("OLD", "NEW"))
    args = ap.parse_args()
    if args.diff:
        raise SystemExit(1 if diff(*args.diff) else 0)
    record(args.out)


if __name__ == "__main__":
    main()
