"""
The cases of the growth-rate sweep, stated once for tests/test_growth_shapes_cpu.py (which shows that they are fair and that
they reach what they claim to reach) and tests/test_gpu_growth_shapes.py (which runs them): plain data from seeded generators.

A ``Case`` names one value per axis -- (ez_model, fde), the step count REQUESTED and the effective one the header's rule makes of
it (include/cosmofit.h: rounded up to 256, 512, 1024 (0 = default) or 2048; stated here, never read back from the library),
n_fs8, a_init, fs8_n_agrid, the block that shares the likelihood, the number of walkers -- and ``build(pkg, case)`` turns it into
the keyword arguments of ``LikelihoodEngine``, the theta rows, the redshifts of the ``fs8_theory_at`` requests and the numpy
oracle's keyword arguments for the blocks that are not the growth block.

The data redshifts are unsorted and hold one duplicate pair.  From n_fs8 = 4 on they hold the a = 1 end, the a = a_init end to
the last ulp cf_create accepts, and a datum on an RK4 step boundary; from 5 on one on the boundary between two lanes' step ranges;
from 56 on one in each wave's quarter of the steps and, with an a-grid, one in its first interval, one in its last, one exactly on
a node and (N <= 7) one in every interval.  ``val`` departs from the theory of row 0 by 10-20 % per datum, so that chi^2 has no
cancellation; with five data or fewer by 25-35 %, and the rows (and the box) stay within 3 % of row 0: a row's few residuals
could otherwise all cancel, and chi^2 would not be conditioned well enough to be judged at 1e-10.

The a = 1 datum.  At z = 0 the Alcock-Paczynski factor q = H D_M / fid is 0 by the equations (D_M(0) = 0), so chi^2 of a data
set that holds z = 0 is not finite on either side and cannot be compared at 1e-10.  The cases flagged ``z0_exact`` hold z = 0
itself: their theory is compared, their chi^2 must be non-finite on both sides.  Every other case holds z = 1e-300 there:
1 / (1 + z) is exactly 1.0 in float64, so the growth kernel sees the a = 1 end (last step, t = 1, the a-grid's last node) while
D_M, fid and q stay finite.  ``fs8_theory_at`` has no q: its requests hold z = 0 itself in every case.
"""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

import derived_reference as R
import growth_reference as G

PAIRS = [(model, fde) for model in (R.LATE_FLAT, R.PHYSICAL) for fde in (R.LCDM, R.WCDM, R.THAWING, R.CPL)]
STEPS_REQUESTED = (1, 256, 257, 512, 513, 0, 1024, 1025, 2048)
STEPS_EFFECTIVE = (256, 256, 512, 512, 1024, 1024, 1024, 2048, 2048)   # by the header's rule
N_FS8 = (1, 4, 5, 56, 63, 64)
A_INIT = (10**-2.15, 10**-2.7, 1 / 201, 0.3)
A_GRID = (0, 4, 5, 7, 1000)
BLOCKS = ("alone", "bao", "cc", "sn")
WALKERS = (1, 3, 70)
AT_N = (0, 1, 63, 64, 65, 130)
Z_ONE = 1e-300   # 1 / (1 + Z_ONE) == 1.0: the a = 1 end with a finite Alcock-Paczynski factor
BOX = dict(H0=(60, 80), Om=(0.15, 0.5), obh2=(0.02, 0.025), och2=(0.09, 0.14), s8=(0.7, 0.9), w0=(-1.4, -0.5), wa=(-1.0, 0.5),
           fs8err=(0.6, 1.7), rd=(130, 160), fcc=(0.5, 2.0), offset=(-19.6, -19.0), v=(-3, 3))
# the dark-energy parameters of rows 0 and 2 (row 2 takes the other entry): wCDM on both sides of -1, thawing away from -1, CPL
# with w_a of both signs
DARK = {R.WCDM: ((-0.7, 0.0), (-1.3, 0.0)), R.THAWING: ((-0.6, 0.0), (-1.2, 0.0)), R.CPL: ((-0.8, -0.9), (-1.2, 0.4))}


@dataclass(frozen=True)
class Case:
    index: int
    ez_model: int
    fde: int
    steps: int        # requested
    S: int            # effective, by the header's rule
    n_fs8: int
    a_init: float
    a_grid: int
    block: str
    W: int
    n_grid: int
    ferr_free: bool
    z0_exact: bool
    logl_const: float

    @property
    def C(self):
        return self.S // 256

    @property
    def name(self):
        return (f"{self.index:02d}-{'LP'[self.ez_model]}{('lcdm', 'wcdm', 'thaw', 'cpl')[self.fde]}-s{self.steps}-n{self.n_fs8}"
                f"-a{self.a_init:.3g}-g{self.a_grid}-{self.block}-W{self.W}")


def _cases():
    out = []
    c_class = {1: (1, 256), 2: (257, 512), 4: (513, 0, 1024), 8: (1025, 2048)}
    for i in range(56):
        pair, rnd = i % 8, i // 8
        model, fde = PAIRS[pair]
        if rnd < 4:   # every (MODEL, FDE, C): the pair meets C = 1, 2, 4, 8 in its first four rounds
            members = c_class[(1, 2, 4, 8)[(rnd + pair) % 4]]
            steps = members[(pair // 4 + rnd) % len(members)]
        else:
            steps = STEPS_REQUESTED[(5 * i + rnd) % 9]
        a_init = A_INIT[(i + rnd + i // 3) % 4]
        if steps in (257, 513) and a_init == 0.3:
            a_init = A_INIT[i % 3]   # from a_init = 0.3 every scheme is converged below 1e-10: no telling 256 from 512 steps
        if steps == 1025:
            # the S = 1024 and S = 2048 schemes must differ by more than 1e-10 with room (test_growth_shapes_cpu.py): only a long
            # integration does that, 1 / 201 only with w0 < -1
            a_init = A_INIT[2 if fde == R.WCDM and rnd >= 4 else 1]
        block = BLOCKS[(3 * i + rnd) % 4]
        if block == "cc" and model == R.PHYSICAL:
            block = "bao"
        n_fs8 = N_FS8[(i + 2 * rnd) % 6]
        out.append(Case(index=i, ez_model=model, fde=fde, steps=steps, S=STEPS_EFFECTIVE[STEPS_REQUESTED.index(steps)], n_fs8=n_fs8,
                        a_init=a_init, a_grid=A_GRID[(2 * i + rnd) % 5], block=block, W=WALKERS[i % 3],
                        n_grid=(513, 4000)[(i + rnd) % 2], ferr_free=i % 5 != 1, z0_exact=n_fs8 >= 4 and i % 7 == 3,
                        logl_const=(0.0, -12.5)[i % 2]))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
ROUNDING = [c for c in CASES if c.steps in (257, 513, 1025)]   # requested one above a power of two: must run the next scheme
HZ_N = (1, 255, 256, 257, 1000)


# ---- the data points -----------------------------------------------------------------------------------------------------------
def z_edge(a_init):
    """the largest z whose a = 1 / (1 + z) cf_create's own check ``1 / (1 + z) >= a_init`` accepts"""
    z = 1.0 / a_init - 1.0
    z = np.nextafter(z, np.inf)
    while 1.0 / (1.0 + z) >= a_init:
        z = np.nextafter(z, np.inf)
    while not 1.0 / (1.0 + z) >= a_init:
        z = np.nextafter(z, 0.0)
    return float(z)


def z_on_node(nodes):
    """(z, j): a redshift whose float64 a = 1 / (1 + z) IS an interior node of the a-grid"""
    for j in range(1, len(nodes) - 1):
        z = 1.0 / nodes[j] - 1.0
        for cand in [z] + [np.nextafter(z, s) for s in (0.0, np.inf)]:
            if 1.0 / (1.0 + cand) == nodes[j]:
                return float(cand), j
    raise AssertionError("no a-grid node is the reciprocal of a float64 1 + z")


def window_of(a, nodes):
    """(li, flags) of the four-node window around a, by the rule of interp_pchip's interval (left searchsorted, clamped) and of
    csrc/cosmofit_api.hip's header comment: nodes i - 1 .. i + 2 shifted inside the grid, flags 1 / 2 = the window holds the
    grid's first / last node."""
    n = len(nodes)
    i = np.clip(np.searchsorted(nodes, a, side="left") - 1, 0, n - 2)
    j0 = np.clip(i - 1, 0, n - 4)
    return i - j0, (j0 == 0) * 1 + (j0 + 3 == n - 1) * 2


def step_of(a, a_init, S):
    x0 = np.log(a_init)
    return np.clip(np.floor((np.log(a) - x0) / (-x0 / S)).astype(np.int64), 0, S - 1)


def _z_at_step(a_init, S, i):
    x0 = np.log(a_init)
    return float(np.expm1(-(x0 + i * (-x0 / S))))


def _interior(rng, a_init, n):
    """n redshifts with ln a uniform inside (ln a_init, 0)"""
    return np.expm1(-np.log(a_init) * rng.uniform(0.02, 0.98, n))


def data_redshifts(case: Case, rng):
    c, S, C = case, case.S, case.C
    if c.n_fs8 == 1:
        return _interior(rng, c.a_init, 1)
    boundary = _z_at_step(c.a_init, S, 3 * S // 8 + (1 if C > 1 else 0))            # a step boundary inside a lane's range
    z = [0.0 if c.z0_exact else Z_ONE, z_edge(c.a_init), boundary, boundary]          # ... twice: the duplicate pair
    if c.n_fs8 >= 5:
        z.append(_z_at_step(c.a_init, S, C * (128 if c.index % 2 else 77)))           # between two lanes (odd cases: two waves)
    if c.n_fs8 >= 56:
        z += [_z_at_step(c.a_init, S, (64 * v + 29) * C + C // 2) * (1 + 1e-3) for v in range(4)]   # inside each wave's quarter
        if c.a_grid:
            nodes = G.a_grid(c.a_init, c.a_grid)
            mids = np.sqrt(nodes[:-1] * nodes[1:])
            pick = range(len(mids)) if c.a_grid <= 7 else (0, len(mids) - 1)
            z += [float(1.0 / mids[j] - 1.0) for j in pick]
            z.append(z_on_node(nodes)[0])
    z = np.array(z + list(_interior(rng, c.a_init, c.n_fs8 - len(z))))
    assert z.size == c.n_fs8
    z = z[rng.permutation(z.size)]
    while not (np.any(np.diff(z) < 0) and np.any(np.diff(z) > 0)):   # unsorted, in either direction
        z = np.roll(z, 1)
    return z


def at_redshifts(case: Case, rng):
    """130 unsorted redshifts of the fs8_theory_at requests: the a_init end first, z = 0 second, a step boundary, a node; a
    request of n takes the first n."""
    z = [z_edge(case.a_init), 0.0, _z_at_step(case.a_init, case.S, 5 * case.S // 8)]
    if case.a_grid:
        z.append(z_on_node(G.a_grid(case.a_init, case.a_grid))[0])
    return np.array(z + list(_interior(rng, case.a_init, 130 - len(z))))


# ---- engines -------------------------------------------------------------------------------------------------------------------
def _physical(comp):
    return {k: comp[k] for k in ("or_h2", "omnu_h2", "o_gamma_h2", "nu_m0", "nu_rho0", "nu_qs_sq", "nu_ws")}


def names_of(case: Case):
    names = ["H0"] + (["obh2", "och2"] if case.ez_model == R.PHYSICAL else ["Om"]) + ["s8"]
    names += (["w0"] if case.fde else []) + (["wa"] if case.fde == R.CPL else []) + (["fs8err"] if case.ferr_free else [])
    if case.block == "bao" and case.ez_model == R.LATE_FLAT:
        names.append("rd")
    return names + {"cc": ["fcc"], "sn": ["offset", "v"]}.get(case.block, [])


def thetas(case: Case, rng):
    names = names_of(case)
    box = np.array([BOX[n] for n in names], dtype=float)
    th = rng.uniform(box[:, 0], box[:, 1], (case.W, len(names)))
    if case.steps == 1025:
        # row 0 at low matter density: there the S = 1024 and S = 2048 schemes differ by well over 1e-10 (test_growth_shapes_cpu.py)
        for n, v in dict(Om=0.16, H0=79.0, obh2=0.0205, och2=0.092).items():
            if n in names and (n != "H0" or case.ez_model == R.PHYSICAL):
                th[0, names.index(n)] = v
    if case.n_fs8 <= 5:
        # a handful of data: every row -- the one outside the box too -- stays within a few per cent of row 0, or some row's few
        # residuals would all cancel; the box shrinks with them (the dark-energy parameters keep theirs for the rows set below)
        near = np.sort(th[0][:, None] * (1 + 0.03 * np.array([-1.0, 1.0])), axis=1)
        keep = np.array([n in ("w0", "wa") for n in names])
        box = np.where(keep[:, None], box, np.stack([np.maximum(near[:, 0], box[:, 0]), np.minimum(near[:, 1], box[:, 1])], axis=1))
        eps = 1e-3 * (box[:, 1] - box[:, 0])
        th[1:] = np.clip(th[0] * (1 + 0.02 * rng.uniform(-1, 1, th[1:].shape)), box[:, 0] + eps, box[:, 1] - eps)
    first = 1 if case.steps == 1025 else case.index // 8 % 2   # (1025 steps: w0 < -1, where the truncation error is largest)
    for row, which in ((0, first), (2, 1 - first)):
        if case.fde and row < case.W:
            w0, wa = DARK[case.fde][which]
            th[row, names.index("w0")] = w0
            if case.fde == R.CPL:
                th[row, names.index("wa")] = wa
    if case.W >= 3:
        th[1, 0] = box[0, 1] * 1.01 if case.n_fs8 <= 5 else 95.0   # one row outside the box
    return box, th


@lru_cache(maxsize=None)
def _build(pkg, name):
    case = BY_NAME[name]
    rng = np.random.default_rng(4200 + case.index)
    P, comp = pkg.Param, pkg.cmb_data.PLANCK_ACT
    names = names_of(case)
    idx = {n: i for i, n in enumerate(names)}
    box, th = thetas(case, rng)
    z = data_redshifts(case, rng)
    z_hi = float(min(2.3, z.max())) if z.max() > 0.3 else 0.3
    z_max = float(max(z.max(), z_hi)) + 0.1
    eng = dict(ndim=len(names), z_max=z_max, n_grid=case.n_grid, fde=case.fde, ez_model=case.ez_model, bounds=box,
               params={n: P(i) for n, i in idx.items()}, logl_const=case.logl_const)
    olk = dict(ndim=len(names), z_max=z_max, n_grid=case.n_grid, fde=case.fde, ez_model=case.ez_model, bounds=box, slots=dict(idx))
    if case.ez_model == R.PHYSICAL:
        eng["physical"] = _physical(comp)
        olk.update(_physical(comp))
    if case.block == "bao":
        nb = 5
        bz = np.sort(rng.uniform(0.05, z_hi, nb))
        M = rng.standard_normal((nb, nb))
        bao = dict(z=bz, val=rng.uniform(5, 30, nb), qty=rng.integers(0, 4, nb).astype(np.int32), inv_cov=M @ M.T + nb * np.eye(nb),
                   dh_exact=True)
        olk.update(bao_z=bz, bao_val=bao["val"], bao_qty=bao["qty"], bao_inv_cov=bao["inv_cov"], bao_dh_exact=True)
        if case.ez_model == R.PHYSICAL:
            bao["rd_fit"] = comp["rd_fit"]
            olk["rd_fit"] = comp["rd_fit"]
        eng["bao"] = bao
    elif case.block == "cc":
        nc = 9
        cz = np.sort(rng.uniform(0.05, z_hi, nc))
        ccov = np.diag(rng.uniform(5, 20, nc) ** 2)
        cc = dict(z=cz, h=70 * np.sqrt(0.3 * (1 + cz) ** 3 + 0.7) + 5 * rng.standard_normal(nc), inv_cov=np.linalg.inv(ccov),
                  logdet=float(np.linalg.slogdet(ccov)[1]))
        eng["cc"] = cc
        olk.update(cc_z=cz, cc_h=cc["h"], cc_inv_cov=cc["inv_cov"], cc_logdet=cc["logdet"])
    elif case.block == "sn":
        ns = 17
        sz = np.sort(rng.uniform(0.01, z_hi, ns))
        zh = sz * (1 + 1e-3 * rng.standard_normal(ns))
        A = 0.02 * rng.standard_normal((ns, 12))
        chol = np.linalg.cholesky(np.diag(rng.uniform(0.1, 0.3, ns) ** 2) + A @ A.T)
        obs = 25 + 5 * np.log10((1 + zh) * 4283.0 * sz * (1 + 0.4 * sz)) - 19.3 + 0.15 * rng.standard_normal(ns)
        eng["sn"] = dict(z_cmb=sz, z_hel=zh, obs=obs, chol=chol, z_turn=0.15)
        olk.update(z_cmb=sz, z_hel=zh, obs=obs, chol=chol, z_turn=0.15)
    # the growth data: fid = (H D_M)(row 0) (1 +- 5 %), val = theory(row 0) / q (1 +- 10..20 %; 25..35 % for a handful of data,
    # whose chi^2 has no other terms to lean on) -- chi^2 has no cancellation; inv_cov dense and positive definite
    n = case.n_fs8
    fs8 = dict(z=z, a_init=case.a_init, steps=case.steps, a_grid=case.a_grid)
    model = R.model_of(dict(eng, fs8=fs8), comp=eng.get("physical"))
    hd = np.asarray(R.curves(model, th[:1], z, "H")[0] * R.curves(model, th[:1], z, "DM")[0], dtype=np.float64)
    fs8["fid"] = np.where(hd > 0, hd, 1.0) * (1 + 0.05 * rng.uniform(-1, 1, n))
    t0 = G.theory(model, th[:1], z, a_init=case.a_init, S=case.S, n_agrid=case.a_grid, dt=np.float64)[0]
    q0 = np.where(hd > 0, hd / fs8["fid"], 1.0)
    fs8["val"] = t0 / q0 * (1 + rng.choice([-1.0, 1.0], n) * (rng.uniform(0.1, 0.2, n) if n >= 56 else rng.uniform(0.25, 0.35, n)))
    M = rng.standard_normal((n, n))
    fs8["inv_cov"] = (M @ M.T / n + np.eye(n)) / 0.05**2
    eng["fs8"] = fs8
    return dict(case=case, engine=eng, oracle=olk, theta=th, model=R.model_of(eng, comp=eng.get("physical")),
                z_at=at_redshifts(case, rng))


def build(pkg, case: Case):
    """dict(case, engine: LikelihoodEngine's keyword arguments, oracle: oracle_np.Likelihood's for the OTHER blocks (``slots``:
    name -> theta index), theta [W, ndim], model: the restatement's Model, z_at [130])"""
    return _build(pkg, case.name)


def model_of_oracle(lk) -> R.Model:
    """the restatement's Model of an oracle_np.Likelihood (the five scripts' fixtures are stated that way in tests/test_fs8.py)"""
    params = {}
    for name in ("H0", "Om", "obh2", "och2", "w0", "wa", "s8", "fs8err", "rd"):
        s = getattr(lk, name)
        if s.idx >= 0 or s.fixed != 0.0:
            params[name] = (s.idx, s.scale) if s.idx >= 0 else ("fixed", s.fixed)
    comp = None
    if lk.ez_model == R.PHYSICAL:
        comp = {k: getattr(lk, k) for k in ("or_h2", "omnu_h2", "o_gamma_h2", "nu_m0", "nu_rho0", "nu_qs_sq", "nu_ws")}
    return R.Model(ndim=lk.ndim, params=params, z_max=lk.z_max, ez_model=lk.ez_model, fde=lk.fde, n_grid=lk.n_grid, om_mode=lk.om_mode,
                   rd_fit=lk.rd_fit, dh_exact=lk.bao_dh_exact, comp=comp, c=lk.c)


def hz_redshifts(n, z_max):
    rng = np.random.default_rng(n)
    return np.concatenate([[0.0], rng.uniform(0.0, z_max, n - 1)])[rng.permutation(n)]
