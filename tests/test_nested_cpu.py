"""CPU: the nested sampler's bookkeeping, its volume formula and error estimate ("perfect" nested sampling), the Prior, and the
random-stream keys -- all without a GPU."""
import math

import numpy as np
import pytest
from scipy import integrate, special, stats

import nested_reference as ref


@pytest.fixture(scope="module")
def nested(pkg):
    return pkg.nested


# ---- bookkeeping against an independent loop ------------------------------------------------------------------------
def _restated(iterations, live, n):
    """Plain-Python statement of step 3 and of the results over a hand-made run: iterations = the sorted dead log L of each
    iteration, live = the final live log L in index order."""
    ln_x, lw, ll = 0.0, [], []
    for dead in iterations:
        for j, l in enumerate(dead):
            a = 1.0 / (n - j)
            lw.append(-math.inf if l == -math.inf else l + ln_x + math.log(-math.expm1(-a)))
            ll.append(l)
            ln_x = ln_x - a
    for l in live:
        lw.append(l + ln_x - math.log(n))
        ll.append(l)
    mx = max(lw)
    log_z = mx + math.log(math.fsum(math.exp(w - mx) for w in lw))
    p = [math.exp(w - log_z) for w in lw]
    h = math.fsum(pi * li for pi, li in zip(p, ll) if pi > 0) - log_z
    return dict(ln_w=np.array(lw), ln_x=ln_x, log_z=log_z, h=h, log_z_err=math.sqrt(h / n),
                n_eff=math.fsum(p) ** 2 / math.fsum(pi * pi for pi in p))


HAND_RUNS = [
    # n, dead log L per iteration (sorted: ties at L*, -inf deaths, a dead set larger than k), final live log L (index order)
    (8, [[-math.inf, -math.inf, -math.inf], [-7.0, -6.5, -6.5], [-5.0, -4.0]], [-3.0, -1.0, -2.5, -0.5, -1.5, -2.0, -0.75, -3.5]),
    (6, [[-20.0, -19.0, -19.0, -19.0], [-3.0, -2.0]], [-1.0, -1.0, -0.2, -0.9, -0.3, -0.4]),
    (10, [[-math.inf], [-9.0, -8.0, -7.5], [-5.0, -5.0]], list(np.linspace(-4.0, -0.1, 10))),
]


@pytest.mark.parametrize("case", range(len(HAND_RUNS)))
def test_bookkeeping_matches_an_independent_loop(nested, case):
    n, iterations, live = HAND_RUNS[case]
    want = _restated(iterations, live, n)
    ln_x, lw = 0.0, []
    for dead in iterations:
        w, ln_x = nested.kill(np.array(dead), ln_x, n)
        lw.append(w)
    lw.append(nested.live_log_weights(np.array(live), ln_x, n))
    lw = np.concatenate(lw)
    assert ln_x == want["ln_x"]
    fin = np.isfinite(want["ln_w"])
    assert np.array_equal(np.isfinite(lw), fin)
    np.testing.assert_allclose(lw[fin], want["ln_w"][fin], rtol=1e-15, atol=0)
    got = nested.summarize(lw, np.concatenate([np.array(d, float) for d in iterations] + [np.array(live)]), n)
    for key in ("log_z", "h", "log_z_err", "n_eff"):
        assert got[key] == pytest.approx(want[key], rel=1e-15, abs=0), key


def test_termination_fraction_matches_its_definition(nested):
    rng = np.random.default_rng(5)
    for _ in range(50):
        n = int(rng.integers(4, 40))
        live = rng.normal(-3, 2, n)
        dead = rng.normal(-12, 3, int(rng.integers(0, 30)))
        ln_x = -float(rng.uniform(0, 10))
        z_live = math.exp(ln_x) * math.fsum(np.exp(live)) / n
        z_dead = math.fsum(np.exp(dead))
        assert nested.live_fraction(ln_x, live, dead, n) == pytest.approx(z_live / (z_dead + z_live), rel=1e-13)
    assert nested.live_fraction(0.0, [-1.0, -2.0], [], 2) == 1.0  # nothing dead yet: never stops
    assert nested.live_fraction(-5.0, [-math.inf] * 4, [-1.0], 4) == 0.0


# ---- "perfect" nested sampling: exact shrinkages through the bookkeeping ---------------------------------------------
def test_batch_deletion_volume_and_error_on_exact_shrinkages(nested):
    """L(X) of a d-dimensional Gaussian (width s) as a function of the enclosed volume X; the live set is simulated exactly
    (uniform volumes, the k = n/2 largest die, replacements uniform below X*), so the only errors are the ones nested
    sampling itself makes: mean log Z within 3 standard errors of the quadrature, reported error ~ the scatter."""
    d, s, n, f_live = 3, 0.05, 100, 0.01
    k = n // 2
    ln_vd = (d / 2) * math.log(math.pi) - special.gammaln(d / 2 + 1)

    def log_l(x):
        ln_r = (np.log(x) - ln_vd) / d
        return -0.5 * np.exp(2 * ln_r) / s**2

    r_max = math.exp(-ln_vd / d)
    z = integrate.quad(lambda r: math.exp(-0.5 * r * r / s**2) * d * math.exp(ln_vd) * r ** (d - 1), 0, r_max,
                       epsabs=0, epsrel=1e-12, limit=200, points=[s, 3 * s])[0]
    truth = math.log(z)
    rng = np.random.default_rng(20061)
    log_z, err = [], []
    for _ in range(200):
        x = rng.uniform(size=n)
        ln_x, lw, ll = 0.0, [], []
        while True:
            order = np.argsort(-x, kind="stable")  # lowest L first = largest X first
            live_sorted = log_l(x[order])
            if nested.live_fraction(ln_x, live_sorted, np.concatenate(lw) if lw else [], n) < f_live:
                break
            w, ln_x = nested.kill(live_sorted[:k], ln_x, n)
            lw.append(w)
            ll.append(live_sorted[:k])
            x[order[:k]] = rng.uniform(size=k) * x[order[k - 1]]
        lw.append(nested.live_log_weights(log_l(x), ln_x, n))
        ll.append(log_l(x))
        out = nested.summarize(np.concatenate(lw), np.concatenate(ll), n)
        log_z.append(out["log_z"])
        err.append(out["log_z_err"])
    log_z, err = np.array(log_z), np.array(err)
    scatter = log_z.std(ddof=1)
    assert abs(log_z.mean() - truth) < 3 * scatter / math.sqrt(log_z.size), (log_z.mean(), truth, scatter)
    assert 0.7 <= err.mean() / scatter <= 1.4, (err.mean(), scatter)


# ---- Prior --------------------------------------------------------------------------------------------------------
def test_prior_rejects_what_it_cannot_sample(nested):
    P = nested.Prior
    for bad in [(1.0, 1.0), (2.0, 1.0), (0.0, math.inf), (math.nan, 1.0), [0.0, 1.0], (0.0, 1.0, 2.0), stats.uniform(0, 1),
                stats.norm(0.0, -1.0), stats.norm(0.0, 0.0), 3.0, "x"]:
        p = P()
        with pytest.raises(ValueError):
            p.add_parameter("a", dist=bad)
    p = P()
    p.add_parameter("a", dist=(0, 1))
    with pytest.raises(ValueError):
        p.add_parameter("a", dist=(0, 1))
    for i in range(15):
        p.add_parameter(f"b{i}", dist=(0, 1))
    with pytest.raises(ValueError):
        p.add_parameter("c", dist=(0, 1))


def test_prior_transform_restates_scipy_ppf(nested):
    p = nested.Prior()
    p.add_parameter("dM", dist=(-1, +1))
    p.add_parameter("H0", dist=stats.norm(73.04, 1.04))
    p.add_parameter("om", dist=(0.1, 0.7))
    p.add_parameter("rd", dist=stats.norm(loc=147.05, scale=0.3))
    assert p.keys == ["dM", "H0", "om", "rd"] and p.dimensionality() == 4
    u = np.random.default_rng(1).uniform(1e-9, 1 - 1e-9, (1000, 4))
    got = p.unit_to_physical(u)
    want = np.stack([stats.uniform(-1, 2).ppf(u[:, 0]), stats.norm(73.04, 1.04).ppf(u[:, 1]),
                     stats.uniform(0.1, 0.6).ppf(u[:, 2]), stats.norm(147.05, 0.3).ppf(u[:, 3])], axis=1)
    np.testing.assert_allclose(got, want, rtol=1e-15, atol=1e-15)
    c = p.c_struct()
    assert c.ndim == 4 and list(c.kind[:4]) == [0, 1, 0, 1] and (c.a[1], c.b[1]) == (73.04, 1.04)


# ---- random streams -------------------------------------------------------------------------------------------------
def test_keys_are_distinct_from_the_ensembles(nested, pkg):
    E = pkg.ensemble
    ens = {E.stream_key(seed, step, half, s) for seed in (0, 1, 42) for step in range(64) for half in (0, 1, 2)
           for s in range(E.MAX_STREAMS)}
    ns = {(nested.ns_key(seed, it, step) + s) & ref._U64 for seed in (0, 1, 42) for it in range(40) for step in range(97)
          for s in range(2 + 2 * 16)}
    assert len(ns) == 3 * 40 * 97 * 34  # no two (seed, iteration, step, stream) share a key either
    assert not ens & ns
    assert nested.ns_key(42, 3, 5) == nested.ns_key(42, 3, 5) != nested.ns_key(43, 3, 5)


def test_scalar_generator_restates_the_array_one(nested, pkg):
    key = nested.ns_key(7, 2, 11)
    c = np.arange(0, 5000, 37)
    np.testing.assert_array_equal(ref.uniform(key, 3, c), [pkg.ensemble.uniform01_scalar(key + 3, int(i)) for i in c])
    u = ref.uniform_open(key, 0, c)
    np.testing.assert_array_equal(u, [nested.uniform_open_scalar(key, int(i)) for i in c])
    assert np.all((u > 0) & (u < 1))
