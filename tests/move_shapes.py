"""The cases of the ensemble-move and nested-walk kernel sweep: one builder for tests/test_move_shapes_cpu.py (which proves on
the host that the cases are well conditioned, reach every listed value and that the bars see a defect) and for
tests/test_gpu_move_shapes.py / tests/test_gpu_nested_kernels.py (which run them on the device through the C entry points).

A case is plain data.  The judge is tests/moves_reference.py (np.longdouble); the nested proposal's long-double statement
and its bound are here, next to the float64 statement of tests/nested_reference.py that the kernel matches bit for bit
where no device libm call enters (sigma = 0, uniform priors).
"""
import functools
import math

import numpy as np

import moves_reference as mr
import nested_reference as nr

LD = np.longdouble
U = LD(2) ** -53  # unit roundoff of float64

# ---- ensemble moves ------------------------------------------------------------------------------------------------------
# (ndim, w_total, n_splits) of the KDE fit and proposal
FIT_CASES = ([(d, 4 * d if d > 1 else 4, 2) for d in range(1, 17)]                       # nc = 2 ndim: the smallest regular sets
             + [(d, w, 2) for d in (3, 5, 7, 8, 9, 16) for w in (514, 600)]              # nc = 257, 300: a second pass of the 256-thread loops
             + [(8, 100, 3), (9, 100, 3)])                                               # three splits, the last triple cut (100 mod 3 = 1)
CHUNK = 2048  # 256 x CF_ENS_KDE_CHUNK complementary walkers per pass of ens_kde_logfactor_kernel
CHUNK_CASES = [(2, 2048), (4, 2049), (16, 2049), (9, 4100), (2, 4100)]                   # (ndim, nc): one, two and three chunks
N_IDS = 96
FAR = [3, 20, 50, 70, 90]  # positions in the ids list of the walkers displaced by 1e3
PROPOSE_NDIM = [1, 2, 9, 16]
PROPOSE_W = [4, 6, 8, 130, 514]
ACCEPT_N = [1, 63, 64, 65, 255, 256, 257, 1000]
ACCEPT_NDIM = [1, 16]
RANDOM_SPLIT_SEED = 2024


def propose_cases():
    """(ndim, w_total, n_splits) of the stretch and DE sweep: both split counts where ens_check allows (three need 6 walkers)."""
    return [(d, w, S) for d in PROPOSE_NDIM for w in PROPOSE_W for S in (2, 3) if not (S == 3 and w < 6)]


def cloud(seed, n, d):
    """n points of a correlated cloud: a random correlation matrix a a^T + d I, normalised; widths geomspace(0.3, 3, d); means
    linspace(-5, 70, d) with coordinate 0 at 147.05 +- 0.3, the workload's largest mean-to-width ratio (r_d of the CMB scripts)."""
    rng = np.random.default_rng(51000 + seed)
    a = rng.standard_normal((d, d))
    c = a @ a.T + d * np.eye(d)
    s = np.sqrt(np.diagonal(c))
    corr = c / np.outer(s, s)
    widths, means = np.geomspace(0.3, 3.0, d), np.linspace(-5.0, 70.0, d)
    widths[0], means[0] = 0.3, 147.05
    return (rng.standard_normal((n, d)) @ np.linalg.cholesky(corr).T) * widths + means


def split_keys():
    """The fixed classes and one re-drawn partition."""
    E = mr._ensemble()
    return (0, E.stream_key(RANDOM_SPLIT_SEED, 7, 0, E._SPLIT_STREAM))


COND_MAX = 6e2  # what the recipe gives at regular sizes; a draw of 2 ndim points can fall above it and is drawn again


@functools.lru_cache(maxsize=None)
def fit_positions(ndim, w_total, n_splits):
    """The cloud of a fit case: the first draw whose complementary sets (both split keys, every split) all have a covariance of
    condition number <= COND_MAX."""
    for attempt in range(200):
        pos = np.ascontiguousarray(cloud(1000 * ndim + w_total + n_splits + 100000 * attempt, w_total, ndim))
        if all(np.linalg.cond(np.cov(pos[mr.comp_ids(key, n_splits, s, w_total)].T).reshape(ndim, ndim)) <= COND_MAX
               for key in split_keys() for s in range(n_splits)):
            pos.setflags(write=False)
            return pos
    raise AssertionError(f"no well-conditioned cloud for ndim={ndim} w_total={w_total}")


def chunk_case(ndim, nc):
    """Positions of 2 nc walkers (n_splits = 2, split_key = 0, split 0: complementary row m is walker 2 m + 1, the active walkers
    are the even ones), and a list of N_IDS active walkers in no particular order.  Complementary rows from CHUNK on form a
    second cluster, displaced by +6 in every coordinate.  Half of the listed walkers lie in each cluster; five are displaced
    by 1e3; for a lone last row (nc = CHUNK + 1) one listed walker sits next to it."""
    rng = np.random.default_rng(61000 + 100 * ndim + nc)
    pos = cloud(7000 + 100 * ndim + nc, 2 * nc, ndim)
    pos[2 * CHUNK + 1::2] += 6.0
    ids = 2 * rng.permutation(nc)[:N_IDS]
    if nc > CHUNK:
        pos[ids[N_IDS // 2:]] += 6.0
        if nc == CHUNK + 1:
            pos[ids[N_IDS // 2]] = pos[2 * CHUNK + 1] + 0.01 * np.geomspace(0.3, 3.0, ndim)
    pos[ids[FAR]] += 1e3
    return np.ascontiguousarray(pos), np.ascontiguousarray(ids.astype(np.int64))


def accept_case(n_active, ndim, start):
    """One accept call on a shard that starts at walker `start`: the active walkers are every second walker of the shard (local
    index 2 i + 1), the others are inactive.  Planted rows (positions in the active list, as far as n_active reaches):
      0 lp_new NaN, 1 lp_new +inf, 2 lp_new -inf, 3 old -inf and lp_new finite, 4 old -inf and lp_new -inf, 5 log factor NaN,
      6 lp_new equal to the old value with factor 0 (always accepted), 7 old -inf and lp_new +inf."""
    rng = np.random.default_rng(71000 + 10 * n_active + ndim + start)
    w_local = 2 * n_active + 3
    c = dict(n=n_active, ndim=ndim, start=start, w_local=w_local)
    c["local_idx"] = 2 * np.arange(n_active, dtype=np.int64) + 1
    c["ids"] = c["local_idx"] + start
    c["x"] = rng.standard_normal((w_local, ndim))
    c["logp"] = -rng.chisquare(ndim, w_local)
    c["y"] = rng.standard_normal((n_active, ndim)) + 10.0
    c["lp_new"] = -rng.chisquare(ndim, n_active)
    c["lf"] = 0.3 * rng.standard_normal(n_active)
    plant = [("lp_new", math.nan), ("lp_new", math.inf), ("lp_new", -math.inf), ("logp", -math.inf), ("both", -math.inf),
             ("lf", math.nan), ("same", 0.0), ("inf_over_minf", 0.0)]
    for i, (what, v) in enumerate(plant[:n_active]):
        li = c["local_idx"][i]
        if what in ("lp_new", "lf"):
            c[what][i] = v
        elif what == "logp":
            c["logp"][li] = v
        elif what == "both":
            c["logp"][li] = c["lp_new"][i] = v
        elif what == "same":
            c["lp_new"][i], c["lf"][i] = c["logp"][li], 0.0
        else:
            c["logp"][li], c["lp_new"][i] = -math.inf, math.inf
    c["planted"] = min(len(plant), n_active)
    return c


# ---- nested walk ---------------------------------------------------------------------------------------------------------
NS_NDIM = [1, 2, 8, 16]
NS_SURV = [1, 2, 3, 64, 1000]  # 1: the walk start only (a proposal needs two distinct partners)
NS_M = [1, 63, 64, 65, 255, 256, 257, 1000]
NS_PRIOR = ["uniform", "normal", "alternating"]
NS_GS = [("de", 1e-6), ("de", 0.0), (0.0, 0.0), (0.5, 0.05)]  # (gamma, sigma); "de" = 2.38 / sqrt(2 ndim), the sampler's scale
NS_DEFAULT = 24


def ns_prior(kind, d):
    """(kind [d] 0 uniform / 1 normal, a [d], b [d]): uniform lo = a < hi = b, normal loc = a, scale = b."""
    k = np.arange(d)
    normal = {"uniform": np.zeros(d, bool), "normal": np.ones(d, bool), "alternating": k % 2 == 1}[kind]
    a = np.where(normal, 0.3 * k - 1.0, -2.0 - k)
    b = np.where(normal, 0.5 + 0.1 * k, 3.0 + 0.5 * k)
    return normal.astype(np.int32), a.astype(np.float64), b.astype(np.float64)


def ns_case(seed, **force):
    """The case of a seed: for the first NS_DEFAULT seeds every list is walked by index."""
    rng = np.random.default_rng(81000 + seed)

    def pick(name, lst, k):
        if name in force:
            return force[name]
        return lst[k % len(lst)] if seed < NS_DEFAULT else lst[int(rng.integers(len(lst)))]

    c = dict(seed=seed)
    c["ndim"] = d = pick("ndim", NS_NDIM, seed)
    c["n_surv"] = ns = pick("n_surv", NS_SURV, seed)
    c["m"] = m = pick("m", NS_M, seed + seed // 8)
    c["prior_kind"] = pick("prior_kind", NS_PRIOR, seed)
    g, s = pick("gs", NS_GS, seed // 3)  # a stride of its own: every ndim meets jitter-free, jittered and wide proposals
    c["gamma"], c["sigma"] = (2.38 / math.sqrt(2.0 * d) if g == "de" else g), s
    c["gs"] = (g, s)
    c["prior"] = ns_prior(c["prior_kind"], d)
    c["key"] = int(rng.integers(1, 2**63 - 1))
    c["su"] = rng.uniform(0.02, 0.98, (ns, d))
    c["stheta"] = rng.standard_normal((ns, d)) * 3.0 + 7.0
    c["slogl"] = rng.standard_normal(ns)
    c["wu"] = rng.uniform(0.05, 0.95, (m, d))
    c["wtheta"] = rng.standard_normal((m, d)) - 40.0
    c["wlogl"] = rng.standard_normal(m)
    return c


def ns_partners(key, m, n_surv):
    i = np.arange(m)
    a = np.minimum((nr.uniform(key, 0, i) * float(n_surv)).astype(np.int64), n_surv - 1)
    b = np.minimum((nr.uniform(key, 1, i) * float(n_surv - 1)).astype(np.int64), n_surv - 2)
    return a, b + (b >= a)


def ns_propose_f64(key, gamma, sigma, su, wu):
    """The kernel's expression in float64, in its order: (u + gamma (u_a - u_b)) + sigma N."""
    m, d = wu.shape
    a, b = ns_partners(key, m, su.shape[0])
    i = np.arange(m)
    pu = np.empty((m, d))
    for k in range(d):
        pu[:, k] = wu[:, k] + gamma * (su[a, k] - su[b, k]) + sigma * nr.normal(key, 2 + 2 * k, i)
    return pu


def ns_propose_ld(key, gamma, sigma, su, wu, drop=None, shift_b=0):
    """The same proposal in long double and the bound on a float64 evaluation of it, from its own terms.

    The sum: v = u + gamma u_a - gamma u_b + sigma N is a sum of four products that a float64 evaluation reaches through five
    rounded operations (the difference of the partners, two products, two sums), so by the standard bound for a sum of
    products it is within gamma_5 = 5 u (u = 2^-53) of v relative to the sum of the terms' magnitudes:
        5 u (|u| + |gamma u_a| + |gamma u_b| + |sigma N|).
    The normal: N = r cos(t), r = sqrt(-2 ln u1), t = 2 pi u2.  A float64 t carries the rounding of the product and of 2 pi,
    2 u |t| together, which moves cos(t) by as much: an ABSOLUTE error, not one relative to N.  OpenCL's accuracy limits for
    the device library (log 3 ulp, cos 4 ulp, sqrt correctly rounded; an ulp is at most 2 u relative) give r within 4 u r,
    cos within 8 u, and the product rounds once more:
        |dN| <= r (8 u + 2 u t) + 5 u |N|,   which enters v as |sigma| |dN|.
    drop = "de" / "noise" leaves a term out, shift_b moves the second partner by one row (the defects the bound must see)."""
    m, d = wu.shape
    ns = su.shape[0]
    a, b = ns_partners(key, m, ns)
    b = (b + shift_b) % ns
    i = np.arange(m)
    g, s = LD(gamma), LD(sigma)
    pu, bound = np.empty((m, d), dtype=LD), np.empty((m, d), dtype=LD)
    for k in range(d):
        u1 = LD(1) - nr.uniform(key, 2 + 2 * k, i).astype(LD)
        t = LD(2) * mr.PI * nr.uniform(key, 3 + 2 * k, i).astype(LD)
        r = np.sqrt(LD(-2) * np.log(u1))
        n = r * np.cos(t)
        diff = su[a, k].astype(LD) - su[b, k].astype(LD)
        p1 = LD(0) * diff if drop == "de" else g * diff
        p2 = LD(0) * n if drop == "noise" else s * n
        s1 = wu[:, k].astype(LD) + p1
        v = s1 + p2
        dn = r * (8 * U + 2 * U * t) + 5 * U * np.abs(n)
        pu[:, k] = v
        terms = np.abs(wu[:, k].astype(LD)) + np.abs(g) * (su[a, k].astype(LD) + su[b, k].astype(LD)) + np.abs(s * n)
        bound[:, k] = 5 * U * terms + np.abs(s) * dn
    return pu, bound


def ns_inside(pu):
    return np.all((pu > 0.0) & (pu < 1.0), axis=1)


def ns_tail_u():
    """The arguments of the Phi^-1 tail check: both tails beyond what the prior draw and the walk usually reach."""
    return np.unique(np.concatenate([np.geomspace(1e-300, 1e-9, 60), [2.0 ** -53], 1.0 - np.geomspace(1e-16, 1e-9, 30),
                                     [1.0 - 2.0 ** -53]]))  # sorted


def ns_tail_reference(u):
    """Phi^-1(u) from mpmath at 30 digits: Newton on the normal CDF from scipy's value; the upper tail by symmetry, through
    1 - u, which is exact for a float64 u at this precision."""
    import mpmath as mp
    from scipy.special import ndtri

    out = []
    with mp.workdps(30):
        for v in u:
            p = mp.mpf(float(v))
            upper = p > 0.5
            if upper:
                p = 1 - p
            x = mp.mpf(float(ndtri(float(p))))
            for _ in range(4):
                x -= (mp.ncdf(x) - p) / mp.npdf(x)
            out.append(-x if upper else x)
    return out
