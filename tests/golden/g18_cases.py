"""Cases of fixture G18 (g18_nsf_ar_grads.npz): the reference's own autograd gradients of
``sum(z * w) + sum(log_det * v)`` through ``NSF_AR.inverse`` (spline_flow.py:218-235), for x and every parameter, in fp32
and from its ``.double()`` run.  The file holds gradients and the two loss values only: inputs, parameters and cotangents
are recipe draws, rebuilt here by the generator (gen_g18_nsf_ar_grads.py) and by the tests alike."""
import recipes

B = 3.0
# tag -> (dim, K, n_h, rows): the reference's test shape | its default K | three groups, a last group of one | the narrowest nets
CASES = {"d2_k8": (2, 8, 16, 33), "d6_k5": (6, 5, 8, 49), "d9_k8": (9, 8, 6, 97), "d13_k5": (13, 5, 4, 35)}


def inputs(tag):
    """(state_dict, x, w, v) of a case; with scale = 1.4 a few percent of the elements lie outside +-B"""
    dim, K, n_h, rows = CASES[tag]
    seed = 1800 + 10 * dim + K
    sd = recipes.nsf_ar_params(seed, dim, K, n_h)
    x = recipes.gaussian(seed + 1, rows, dim, scale=1.4)
    w = recipes.gaussian(seed + 2, rows, dim)
    v = recipes.gaussian(seed + 3, rows, 1)[:, 0]
    return sd, x, w, v


def grad_names(tag):
    return ["x", *inputs(tag)[0].keys()]


def split(tag, flat):
    """{name: array} of a fixture vector ``{tag}.g32`` / ``{tag}.g64``"""
    sd, x, _, _ = inputs(tag)
    out, at = {}, 0
    for name, shape in [("x", tuple(x.shape)), *((k, tuple(t.shape)) for k, t in sd.items())]:
        n = 1
        for s in shape:
            n *= s
        out[name] = flat[at:at + n].reshape(shape)
        at += n
    assert at == flat.size, (tag, at, flat.size)
    return out
