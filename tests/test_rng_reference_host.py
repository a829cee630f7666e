"""The DEFINITION of the in-kernel random streams (tests/rng_reference.py, a restatement of mnf_device.h) is a sound
generator: moments, Kolmogorov-Smirnov distance, tails, serial / cross-seed / cross-stream correlations of the two normal
streams and of the Bernoulli(0.5) mask, at fixed seeds and one fixed shape.  The streams are stateless, so every
statistic below is the same number on every run: nothing here can flake.  tests/test_hip_rng.py ties the device to this
definition, which carries these statistics over to it.

Bounds (conditions, not measurements): every z-score |z| <= 5 (two-sided 5.7e-7 each, ~4e-4 over the few hundred
statistics of this file), KS * sqrt(n) <= 2.5 (asymptotic p 7.5e-6), the popcount chi-square p >= 1e-6.  Measured at these
seeds and this shape: worst |z| 4.08 (mask, seed 3 against seed 4), worst KS * sqrt(n) 1.84 (ml_normal, seed 7,
4096 x 256), worst bit-position |z| 3.31, smallest popcount p 0.095 (profiles/r13/rng_stream.txt).

Three deliberately wrong variants of the reference are run through the same battery at the same bounds and must be
rejected: a battery that cannot tell them from the real thing is not finished.
"""
import numpy as np
import pytest
from scipy import special, stats

import rng_reference as R

SEEDS = [0, 1, 2, 3, 7, 0xFFFFFFFF, 0x100000000, 0x9E3779B97F4A7C15, 0x123456789ABCDEF0, 0xFFFFFFFFFFFFFFFF,
         0x8000000000000000, 0x5BD1E995]
ROWS, COLS = 32768, 128
Z_MAX, KS_MAX, P_MIN, X_MAX = 5.0, 2.5, 1e-6, 5.8871


class Reference:
    """The three streams as the battery sees them: normals without their hashes."""
    name = "reference"

    @staticmethod
    def ml(seed, rows, cols):
        return R.ml_normal(seed, rows, cols)[0]

    @staticmethod
    def z0(seed, rows, cols):
        return R.z0_normal(seed, rows, cols)[0]

    @staticmethod
    def mask(seed, rows, cols):
        return R.mask(seed, rows, cols)


# ---------------------------------------------------------------------------------------------------- wrong variants
class BothCosine(Reference):
    """n1 = r cos instead of r sin: the two columns of a z0 pair are the same number."""
    name = "n1 = r cos"

    @staticmethod
    def z0(seed, rows, cols):
        x = R.z0_normal(seed, rows, cols + (cols & 1))[0].copy()
        x[:, 1::2] = x[:, 0::2]
        return x[:, :cols]


class NoColumnTerm(Reference):
    """The column (word, pair) term dropped from the hash: every column of a row draws from the same hash."""
    name = "column term dropped"

    @staticmethod
    def _h1(seed, rows, n_idx, k):
        a = R.row_hash(seed, rows)
        seed_lo = ((int(seed) & R.M32) ^ k) & R.M32
        return np.repeat(R.mix32(a ^ np.uint32(seed_lo))[:, None], n_idx, axis=1)

    @classmethod
    def ml(cls, seed, rows, cols):
        h1 = cls._h1(seed, rows, cols, 0)
        h2 = R.mix32(h1 ^ np.uint32(R.H2_XOR))
        return R.radius(h1) * np.cos(2 * np.pi * R.uniform24(h2).astype(np.float64))

    @classmethod
    def z0(cls, seed, rows, cols):
        pairs = (cols + 1) // 2
        h1 = cls._h1(seed, rows, pairs, R.Z0_XOR)
        ph = 2 * np.pi * R.uniform24(R.mix32(h1 ^ np.uint32(R.H2_XOR))).astype(np.float64)
        x = np.empty((rows, 2 * pairs))
        x[:, 0::2], x[:, 1::2] = R.radius(h1) * np.cos(ph), R.radius(h1) * np.sin(ph)
        return x[:, :cols]

    @classmethod
    def mask(cls, seed, rows, cols):
        w = cls._h1(seed, rows, (cols + 31) // 32, 0)
        d = np.arange(cols)
        return ((w[:, d >> 5] >> (d & 31).astype(np.uint32)[None, :]) & np.uint32(1)).astype(np.float32)


class NoHalf(Reference):
    """u1 taken without the + 0.5: u1 = 0 is reachable, and its logarithm is not finite."""
    name = "u1 without + 0.5"

    @staticmethod
    def _r(h1):
        u1 = (h1 >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
        with np.errstate(divide="ignore"):
            return np.sqrt(-2.0 * np.log(u1.astype(np.float64)))

    @classmethod
    def ml(cls, seed, rows, cols):
        _, h1, h2 = R.ml_normal(seed, rows, cols)
        return cls._r(h1) * np.cos(2 * np.pi * R.uniform24(h2).astype(np.float64))

    @classmethod
    def z0(cls, seed, rows, cols):
        _, h1, h2 = R.z0_normal(seed, rows, cols)
        ph = 2 * np.pi * R.uniform24(h2).astype(np.float64)
        return cls._r(h1) * np.where(np.arange(cols)[None, :] & 1, np.sin(ph), np.cos(ph))


# ---------------------------------------------------------------------------------------------------------- statistics
def _prod_z(a, b, var=1.0):
    """z-score of sum(a b) for independent a, b with E = 0 and Var(a b) = var."""
    with np.errstate(invalid="ignore"):  # (inf / NaN of a wrong variant gives a NaN z-score, which violations() reports)
        return float(np.sum(a * b, dtype=np.float64) / np.sqrt(var * a.size))


def ks_sqrt_n(x):
    """Kolmogorov-Smirnov distance of the sample to the standard normal, times sqrt(n)."""
    s = np.sort(x, axis=None)
    n = s.size
    cdf = special.ndtr(s)
    i = np.arange(1, n + 1, dtype=np.float64)
    return float(max((i / n - cdf).max(), (cdf - (i - 1) / n).max()) * np.sqrt(n))


def normal_stats(x, tag, out):
    n = x.size
    out["finite"][tag] = bool(np.isfinite(x).all())
    with np.errstate(invalid="ignore"):  # (a wrong variant may hold inf / NaN: reported through "finite")
        out["max"][tag] = float(np.abs(x).max())
    if not out["finite"][tag]:  # the moments of a stream with an infinity in it say nothing more
        return
    z = out["z"]
    for k, (mean, var) in enumerate([(0.0, 1.0), (1.0, 2.0), (0.0, 15.0), (3.0, 96.0)], start=1):
        z[f"{tag} moment {k}"] = float((np.mean(x ** k) - mean) / np.sqrt(var / n))
    out["ks"][tag] = ks_sqrt_n(x)
    ax = np.abs(x)
    for t in (2.0, 3.0, 4.0):
        lam = n * special.erfc(t / np.sqrt(2.0))
        z[f"{tag} tail |x| > {t:g}"] = float((np.count_nonzero(ax > t) - lam) / np.sqrt(lam))
    z[f"{tag} columns lag 1"] = _prod_z(x[:, :-1], x[:, 1:])
    z[f"{tag} columns lag 2"] = _prod_z(x[:, :-2], x[:, 2:])
    z[f"{tag} rows lag 1"] = _prod_z(x[:-1], x[1:])
    y = x * x - 1.0
    z[f"{tag} x^2-1 columns lag 1"] = _prod_z(y[:, :-1], y[:, 1:], 4.0)
    z[f"{tag} x^2-1 rows lag 1"] = _prod_z(y[:-1], y[1:], 4.0)
    rows, cols = x.shape
    z[f"{tag} column means chi2"] = float((rows * np.sum(x.mean(axis=0) ** 2) - cols) / np.sqrt(2.0 * cols))
    z[f"{tag} row means chi2"] = float((cols * np.sum(x.mean(axis=1) ** 2) - rows) / np.sqrt(2.0 * rows))


def mask_stats(m, out):
    z = out["z"]
    rows, cols = m.shape
    assert set(np.unique(m).tolist()) <= {0.0, 1.0}
    s = 2.0 * m.astype(np.float64) - 1.0  # +-1
    z["mask mean"] = float(s.sum() / np.sqrt(s.size))
    for b in range(32):
        sb = s[:, b::32]
        z[f"mask bit {b}"] = float(sb.sum() / np.sqrt(sb.size))
    z["mask columns lag 1"] = _prod_z(s[:, :-1], s[:, 1:])
    z["mask columns lag 32"] = _prod_z(s[:, :-32], s[:, 32:])
    z["mask rows lag 1"] = _prod_z(s[:-1], s[1:])
    # per-row popcount against Binomial(cols, 1/2): bins 50 .. 78, the two tails pooled
    pop = m.sum(axis=1).astype(np.int64)
    k = np.arange(cols + 1)
    pmf = stats.binom.pmf(k, cols, 0.5)
    obs = np.bincount(pop, minlength=cols + 1).astype(np.float64)
    lo, hi = 50, 78
    obs_b = np.concatenate([[obs[:lo].sum()], obs[lo:hi + 1], [obs[hi + 1:].sum()]])
    exp_b = rows * np.concatenate([[pmf[:lo].sum()], pmf[lo:hi + 1], [pmf[hi + 1:].sum()]])
    chi2 = float(np.sum((obs_b - exp_b) ** 2 / exp_b))
    out["p"]["mask popcount"] = float(stats.chi2.sf(chi2, obs_b.size - 1))
    return s


def battery(G, seed, rows=ROWS, cols=COLS):
    """Every statistic of the issue for one seed -> {"z": {...}, "ks": {...}, "p": {...}, "finite": {...}, "max": {...}}."""
    assert cols == 128, "the popcount bins are those of Binomial(128, 1/2)"
    out = {"z": {}, "ks": {}, "p": {}, "finite": {}, "max": {}}
    z = out["z"]
    xs = {}
    for tag, gen in (("ml", G.ml), ("z0", G.z0)):
        x = xs[tag] = gen(seed, rows, cols)
        normal_stats(x, tag, out)
        if not out["finite"][tag]:
            continue
        for what, other in (("s + 1", (seed + 1) & R.M64), ("s ^ 1 << 32", seed ^ (1 << 32)),
                            ("s + 0x9E37..7C15", (seed + R.SLAB_STEP) & R.M64)):
            z[f"{tag} seed s against {what}"] = _prod_z(x, gen(other, rows, cols))
    s = mask_stats(G.mask(seed, rows, cols), out)
    z["mask seed s against s + 1"] = _prod_z(s, 2.0 * G.mask((seed + 1) & R.M64, rows, cols) - 1.0)
    if out["finite"]["ml"] and out["finite"]["z0"]:
        z["ml x z0"] = _prod_z(xs["ml"], xs["z0"])
        z["mask x ml"] = _prod_z(s, xs["ml"])
        z["mask x z0"] = _prod_z(s, xs["z0"])
        z["mask x (ml^2 - 1)"] = _prod_z(s, xs["ml"] ** 2 - 1.0, 2.0)
    return out


def extremes(G):
    """The largest magnitude of each normal stream, reached on purpose: under seed_for(h1 >> 8 == 0) element (3, 2) of
    a 4 x 4 call -> {stream: value}."""
    return {tag: float(gen(R.seed_for(0xAB, 0, 3, 2, tag), 4, 4)[3, 2]) for tag, gen in (("ml", G.ml), ("z0", G.z0))}


def violations(out) -> list[str]:
    bad = [f"{k}: not finite" for k, ok in out["finite"].items() if not ok]
    bad += [f"{k}: max |x| {v:.4f} > {X_MAX}" for k, v in out["max"].items() if not v <= X_MAX]
    bad += [f"{k}: |z| = {abs(v):.2f} > {Z_MAX}" for k, v in out["z"].items() if not abs(v) <= Z_MAX]
    bad += [f"{k}: KS sqrt(n) = {v:.2f} > {KS_MAX}" for k, v in out["ks"].items() if not v <= KS_MAX]
    bad += [f"{k}: p = {v:.2e} < {P_MIN}" for k, v in out["p"].items() if not v >= P_MIN]
    return bad


def summary(out) -> str:
    kz, vz = max(out["z"].items(), key=lambda kv: abs(kv[1]))
    bits = max(abs(v) for k, v in out["z"].items() if k.startswith("mask bit"))
    return (f"{len(out['z'])} z-scores, worst |z| {abs(vz):.2f} ({kz}); KS sqrt(n) "
            + ", ".join(f"{k} {v:.2f}" for k, v in out["ks"].items())
            + f"; worst bit-position |z| {bits:.2f}; popcount p {out['p']['mask popcount']:.3f}; max |x| "
            + ", ".join(f"{k} {v:.4f}" for k, v in out["max"].items()))


# --------------------------------------------------------------------------------------------------------------- tests
def test_mix32_constants_and_inverse():
    """mix32 is murmur3's 32-bit finaliser (its published vectors), and unmix32 inverts it."""
    assert R.mix32(0) == 0 and R.mix32(1) == 0x514E28B7 and R.mix32(0xFFFFFFFF) == 0x81F16F39
    h = np.array([0, 1, 2, 0x80000000, 0xFFFFFFFF, 0xDEADBEEF, 0x12345678], dtype=np.uint32)
    assert [R.unmix32(int(v)) for v in R.mix32(h)] == h.tolist()
    assert [R.mix32(R.unmix32(int(v))) for v in h] == h.tolist()
    rng = np.random.default_rng(0).integers(0, 1 << 32, 1000, dtype=np.uint64)
    assert all(R.unmix32(R.mix32(int(v))) == int(v) for v in rng)


def test_uniform_is_the_float32_expression():
    """(float)(h >> 8) + 0.5f rounds to even from 2**23 on; the top hash gives exactly 1.0, the bottom one 2**-25."""
    u = R.uniform24(np.array([0, 0xFF, 0x100, 0x7FFFFFFF, 0x80000000, 0x80000100, 0xFFFFFD00, 0xFFFFFE00, 0xFFFFFFFF],
                             dtype=np.uint32))
    assert u.dtype == np.float32
    two24 = 2.0 ** 24
    assert (u.astype(np.float64) * two24).tolist() == [0.5, 0.5, 1.5, 2 ** 23 - 0.5, 2 ** 23, 2 ** 23 + 2, 2 ** 24 - 2,
                                                       2 ** 24 - 2, 2 ** 24]
    assert float(R.radius(np.uint32(0xFFFFFFFF))) == 0.0
    assert abs(float(R.radius(np.uint32(0))) - R.R_MAX) < 1e-12 and abs(R.R_MAX - 5.88705) < 1e-5


def test_stream_indexing():
    """Element (row, col) does not depend on the call's shape; the z0 pair shares its hash; the mask word serves 32
    columns; the row >> 32 term and both seed halves enter; the three streams differ under one seed."""
    seed = 0x123456789ABCDEF0
    x, h1, h2 = R.ml_normal(seed, 40, 70)
    xs, h1s, _ = R.ml_normal(seed, 7, 9)
    assert np.array_equal(x[:7, :9], xs) and np.array_equal(h1[:7, :9], h1s)
    assert np.array_equal(R.ml_normal(seed, 5, 9, row0=35)[0], x[35:, :9])
    zf, g1, g2 = R.z0_normal(seed, 40, 71)
    assert np.array_equal(zf[:, :33], R.z0_normal(seed, 40, 33)[0])
    assert np.array_equal(g1[:, 0:70:2], g1[:, 1:70:2]) and np.array_equal(g2[:, 0:70:2], g2[:, 1:70:2])
    r = R.radius(g1)
    assert np.allclose(zf[:, 0:70:2] ** 2 + zf[:, 1:70:2] ** 2, r[:, 0:70:2] ** 2, rtol=1e-12, atol=1e-300)
    m = R.mask(seed, 40, 70)
    w = R.mask_words(seed, 40, 70)
    assert w.shape == (40, 3) and m.shape == (40, 70) and m.dtype == np.float32
    for d in (0, 1, 31, 32, 33, 63, 64, 69):
        assert np.array_equal(m[:, d], ((w[:, d >> 5] >> np.uint32(d & 31)) & np.uint32(1)).astype(np.float32))
    # the mask word and ml_normal's h1 are the same hash at (seed, row, index): the streams read different bits of it
    assert np.array_equal(w, h1[:, :3])
    assert not np.array_equal(g1[:, 0:6:2], h1[:, :3])
    big = np.array([5, 5 + (1 << 32), 5 + (2 << 32)], dtype=np.int64)
    a = R.row_hash(seed, big)
    assert len(set(a.tolist())) == 3 and a[0] == R.row_hash(seed, 6)[5]
    assert R.row_hash(seed, 4).tolist() != R.row_hash(seed ^ (1 << 32), 4).tolist()
    assert not np.array_equal(R.ml_normal(seed, 4, 4)[1], R.ml_normal(seed ^ 1, 4, 4)[1])


def test_slab_seeds():
    """MNFLinear._slab_seed: seed + k * 0x9E3779B97F4A7C15 mod 2**64, the column index restarting in each slab."""
    assert R.slab_seed(5, 0) == 5 and R.slab_seed(5, 1) == 5 + 0x9E3779B97F4A7C15
    assert R.slab_seed(0xFFFFFFFFFFFFFFFF, 2) == (0xFFFFFFFFFFFFFFFF + 2 * 0x9E3779B97F4A7C15) % (1 << 64)
    x, h1, _ = R.mnf_linear_noise(77, 9, 150)
    assert x.shape == (9, 150)
    assert np.array_equal(x[:, :64], R.ml_normal(77, 9, 64)[0])
    assert np.array_equal(x[:, 64:128], R.ml_normal(R.slab_seed(77, 1), 9, 64)[0])
    assert np.array_equal(x[:, 128:], R.ml_normal(R.slab_seed(77, 2), 9, 22)[0])
    assert np.array_equal(R.mnf_linear_noise(77, 9, 64)[0], R.ml_normal(77, 9, 64)[0])


@pytest.mark.parametrize("stream", ["ml", "z0", "mask"])
def test_seed_for_places_a_chosen_hash(stream):
    gen = {"ml": lambda s, r, c: R.ml_normal(s, r, c)[1], "z0": lambda s, r, c: R.z0_normal(s, r, c)[1],
           "mask": lambda s, r, c: np.repeat(R.mask_words(s, r, c), 32, axis=1)[:, :c]}[stream]
    for target, hi, row, col in [(0, 0, 3, 2), (0xFFFFFFFF, 0, 16, 2), (0xDEADBEEF, 0x9E3779B9, 16, 37),
                                 (0x00000100, 0xFFFFFFFF, 0, 0), (0x80000000, 1, 332, 49)]:
        seed = R.seed_for(target, hi, row, col, stream)
        assert seed >> 32 == hi
        assert int(gen(seed, row + 1, col + 1)[row, col]) == target, (stream, hex(target), row, col)


def test_largest_magnitude_of_the_generator():
    """Under seed_for(h1 >> 8 == 0): r = sqrt(50 ln 2) = 5.88705, the largest the generator can produce, and with the
    h2 that this h1 implies the ml_normal element is r cos = 5.3171."""
    seed = R.seed_for(0xAB, 0, 3, 2, "ml")  # (the low 8 bits of h1 do not reach u1; they do reach h2)
    x, h1, _ = R.ml_normal(seed, 4, 4)
    assert h1[3, 2] == 0xAB and abs(float(R.radius(h1)[3, 2]) - 5.88705) < 1e-5
    assert abs(x[3, 2] - 5.3171) < 1e-4
    assert R.mix32(R.h1_for_h2(0x12345678) ^ R.H2_XOR) == 0x12345678
    ex = extremes(Reference)
    assert all(np.isfinite(v) and abs(v) <= X_MAX for v in ex.values()), ex


@pytest.mark.parametrize("seed", SEEDS, ids=[hex(s) for s in SEEDS])
def test_battery_at_the_stated_bounds(seed):
    out = battery(Reference, seed)
    print(f"\nseed {seed:#x}: {summary(out)}")
    assert not violations(out), violations(out)


def test_ks_ml_normal_seed_7_at_4096_by_256():
    """The worst Kolmogorov-Smirnov case on record: 1.84."""
    ks = ks_sqrt_n(Reference.ml(7, 4096, 256))
    print(f"\nKS sqrt(n), ml_normal, seed 7, 4096 x 256: {ks:.3f}")
    assert ks <= KS_MAX


@pytest.mark.parametrize("variant,seed,expect", [
    (BothCosine, 7, ["z0 columns lag 1:"]),
    (NoColumnTerm, 7, ["ml columns lag 1:", "z0 columns lag 2:", "mask columns lag 32:"]),
    # seed 0: element (0, 0) of ml_normal has h1 == 0 (a_row = mix32(0) = 0, column 0, seed 0), so u1 = 0 without the half
    (NoHalf, 0, ["ml: not finite"]),
], ids=["both-cosine", "no-column-term", "u1-without-half"])
def test_battery_rejects_a_wrong_variant(variant, seed, expect):
    """Each wrong variant through battery() and violations(), the path and the bounds that hold the reference."""
    bad = violations(battery(variant, seed))
    print(f"\n{variant.name}: {len(bad)} violations, e.g. {bad[:4]}")
    for e in expect:
        assert any(b.startswith(e) for b in bad), (variant.name, e, bad)


def test_extreme_element_is_finite_only_with_the_half():
    """The element with h1 >> 8 == 0, placed with seed_for: 5.3171 under the definition, not finite with u1 = k / 2**24."""
    ex = extremes(Reference)
    assert all(np.isfinite(v) and abs(v) <= X_MAX for v in ex.values()), ex
    assert not any(np.isfinite(v) for v in extremes(NoHalf).values())


# ------------------------------------------------------------------------------------------- a KNOWN dependence
def test_known_dependence_the_mask_word_is_ml_normals_h1():
    """A weakness of the DEFINITION, recorded and asserted, not fixed here (changing it changes every seeded result):

    * rnvp_mask_word(seed, row, w) IS ml_normal's h1 at (seed, row, column w): the same hash.  Bits 8..31 of mask word w
      are the 24-bit integer of that element's u1, so under ONE seed mask column 32 w + 31 is the indicator u1 >= 1/2 of
      ml_normal column w: E[(2 m - 1)(x^2 - 1)] = -ln 2, correlation -0.49, z = -0.49 sqrt(rows) = -88.7 at 32768 rows
      (column 32 w + 30: about -55).  The battery's same-seed cross-stream statistics multiply element (r, c) by element
      (r, c) and cannot see it (mask x (ml^2 - 1): |z| < 5).
    * z0_normal under seed s draws pair p from the hash of ml_normal column p under seed s ^ 0x5BD1E995:
      z0_normal(s ^ 0x5BD1E995, r, 2 p) == ml_normal(s, r, p) exactly.

    The library's callers draw a separate seed from torch's generator for every RNVP mask, every sample_z prologue and
    every MNFLinear noise launch, so no caller pairs the streams this way; a change of constants that removes or moves
    the dependence fails here and is seen."""
    seed, rows, cols = 7, ROWS, COLS
    x, h1, _ = R.ml_normal(seed, rows, cols)
    w = R.mask_words(seed, rows, cols)
    assert np.array_equal(w, h1[:, :cols // 32])
    m = R.mask(seed, rows, cols)
    y = x * x - 1.0
    for word in range(cols // 32):
        z31 = _prod_z(2.0 * m[:, 32 * word + 31] - 1.0, y[:, word], 2.0)
        z30 = _prod_z(2.0 * m[:, 32 * word + 30] - 1.0, y[:, word], 2.0)
        print(f"\nmask column {32 * word + 31} x (ml column {word})^2 - 1: z = {z31:.1f}; column {32 * word + 30}: z = {z30:.1f}")
        assert abs(z31 + np.log(2.0) / np.sqrt(2.0) * np.sqrt(rows)) < 5.0, z31  # -88.7 +- chance
        assert -65.0 < z30 < -45.0, z30
        for b in range(8):  # the low byte of the hash does not reach u1
            assert abs(_prod_z(2.0 * m[:, 32 * word + b] - 1.0, y[:, word], 2.0)) <= Z_MAX
    assert abs(_prod_z(2.0 * m - 1.0, y, 2.0)) <= Z_MAX  # the elementwise statistic of the battery: blind to it
    z0 = R.z0_normal(seed ^ R.Z0_XOR, 64, 2 * 50)[0]
    assert np.array_equal(z0[:, 0::2], x[:64, :50])
