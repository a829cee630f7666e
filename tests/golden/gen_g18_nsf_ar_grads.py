"""Write fixture G18 by running the REAL reference (janosh/torch-mnf): its own autograd gradients through NSF_AR.inverse.

Run in the build container only (needs the reference checkout, MNF_REFERENCE or /root/reference; it never travels):

    python tests/golden/gen_g18_nsf_ar_grads.py

The fixture is data: ``{tag}.g32`` / ``{tag}.g64`` -- the gradients of x and of every state_dict tensor, flattened and
joined in the order of g18_cases.grad_names (g18_cases.split takes them apart) -- and ``{tag}.loss`` / ``{tag}.loss64`` for
the cases of g18_cases.py.  No reference source text is copied."""
import os
import sys

sys.dont_write_bytecode = True
REF = os.environ.get("MNF_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import g18_cases as C  # noqa: E402
import torch_mnf.flows as nf  # noqa: E402  (the reference)

torch.set_num_threads(8)


def reference_grads(tag, dtype):
    dim, K, n_h, _ = C.CASES[tag]
    sd, x, w, v = C.inputs(tag)
    layer = nf.NSF_AR(dim, K=K, B=3, n_h=n_h).to(dtype)
    layer.load_state_dict({k: t.to(dtype) for k, t in sd.items()})
    xg = x.to(dtype).requires_grad_(True)
    z, log_det = layer.inverse(xg)
    loss = (z * w.to(dtype)).sum() + (log_det * v.to(dtype)).sum()
    loss.backward()
    grads = {"x": xg.grad, **{name: p.grad for name, p in layer.named_parameters()}}
    assert set(grads) == set(C.grad_names(tag)), sorted(set(grads) ^ set(C.grad_names(tag)))
    return float(loss.detach()), {k: g.detach().numpy() for k, g in grads.items()}


def main():
    out = {}
    for tag in C.CASES:
        sd, x, _, _ = C.inputs(tag)
        outside = float((x.abs() > C.B).float().mean())
        loss32, g32 = reference_grads(tag, torch.float32)
        loss64, g64 = reference_grads(tag, torch.float64)
        out[f"{tag}.loss"], out[f"{tag}.loss64"] = np.float32(loss32), np.float64(loss64)
        names = C.grad_names(tag)
        out[f"{tag}.g32"] = np.concatenate([g32[k].reshape(-1) for k in names]).astype(np.float32)
        out[f"{tag}.g64"] = np.concatenate([g64[k].reshape(-1) for k in names]).astype(np.float64)
        print(f"{tag}: {100 * outside:.1f} % of the elements outside +-B, loss {loss32:.6f} / {loss64:.12f}")
    path = os.path.join(HERE, "g18_nsf_ar_grads.npz")
    np.savez_compressed(path, **out)
    print(f"g18_nsf_ar_grads.npz  {os.path.getsize(path) / 1024:.0f} KiB  keys={len(out)}")


if __name__ == "__main__":
    main()
