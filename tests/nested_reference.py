"""numpy restatement of the nested sampler's kernels (csrc/cosmofit_nested.hip) for tests/test_gpu_nested.py: the generator on
uint64 arrays, the prior draw and one full iteration (deaths, walk start, n_walk DE steps, fill of the dead slots).  The
likelihood of the restated walk is the sampler's own torch callable, called on the same rows."""
import math

import numpy as np

G = np.uint64(0x9E3779B97F4A7C15)
_U64 = 0xFFFFFFFFFFFFFFFF


def mix(x):
    with np.errstate(over="ignore"):
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def bits(key, stream, counter):
    c = np.asarray(counter, dtype=np.int64).astype(np.uint64)
    with np.errstate(over="ignore"):
        x = mix(c * G + np.uint64((key + stream) & _U64))
        return mix(x + G)


def uniform(key, stream, counter):
    return (bits(key, stream, counter) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def uniform_open(key, stream, counter):
    return ((bits(key, stream, counter) >> np.uint64(11)) | np.uint64(1)).astype(np.float64) * (1.0 / 9007199254740992.0)


def normal(key, stream, counter):
    u1 = 1.0 - uniform(key, stream, counter)
    u2 = uniform(key, stream + 1, counter)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos((2.0 * math.pi) * u2)


def prior_draw(nested, prior, n, seed):
    key = nested.ns_key(seed, 0, 0)
    i = np.arange(n)
    u = np.stack([uniform_open(key, k, i) for k in range(prior.dimensionality())], axis=1)
    return u, prior.unit_to_physical(u)


def iteration(nested, prior, loglike, u, th, logl, *, seed, it, n_batch, n_walk, gamma, sigma):
    """One iteration on host copies of the live set; loglike(theta [W, d] numpy) -> numpy [W].  Returns the new live set,
    the dead rows (death order) and the walk counters (accepted, out of the cube, non-finite)."""
    u, th, logl = u.copy(), th.copy(), logl.copy()
    n, d = u.shape
    order = np.lexsort((np.arange(n), logl))  # log L ascending, index ascending
    sl = logl[order]
    lstar = sl[n_batch - 1]
    m = int(np.searchsorted(sl, lstar, side="right"))
    dead, slots, surv = order[:m], np.sort(order[:m]), np.sort(order[m:])
    su, sth, sll = u[surv], th[surv], logl[surv]
    ns = surv.size
    i = np.arange(m)
    j = np.minimum((uniform(nested.ns_key(seed, it, 0), 0, i) * ns).astype(np.int64), ns - 1)
    wu, wth, wl = su[j].copy(), sth[j].copy(), sll[j].copy()
    counts = np.zeros(3, dtype=np.int64)
    for s in range(1, n_walk + 1):
        key = nested.ns_key(seed, it, s)
        a = np.minimum((uniform(key, 0, i) * ns).astype(np.int64), ns - 1)
        b = np.minimum((uniform(key, 1, i) * (ns - 1)).astype(np.int64), ns - 2)
        b = b + (b >= a)
        pu = np.empty((m, d))
        for k in range(d):
            pu[:, k] = wu[:, k] + gamma * (su[a, k] - su[b, k]) + sigma * normal(key, 2 + 2 * k, i)
        inside = np.all((pu > 0.0) & (pu < 1.0), axis=1)
        with np.errstate(invalid="ignore"):
            pth = np.where(inside[:, None], prior.unit_to_physical(np.clip(pu, 1e-300, 1.0 - 1e-16)), wth)
        pl = loglike(pth)
        fin = np.isfinite(pl)
        acc = inside & fin & (pl > lstar)
        counts += [int(acc.sum()), int((~inside).sum()), int((inside & ~fin).sum())]
        wu[acc], wth[acc], wl[acc] = pu[acc], pth[acc], pl[acc]
    dead_th, dead_l = th[dead].copy(), sl[:m].copy()
    u[slots], th[slots], logl[slots] = wu, wth, wl
    return dict(u=u, th=th, logl=logl, dead_th=dead_th, dead_l=dead_l, m=m, counts=counts)
