"""
Mock-data ensembles on the device: calibrate a Delta chi^2 significance, and the goodness of fit of chi^2_min, by simulation.

Every result of the reference is a best fit plus a Delta chi^2 read through Wilks' theorem ("delta chi2 = 11.7 -> 3.4 sigma",
sn/pantheon_dipole.py:172; 28.76 - 22.15 -> 2.57 sigma, sn/union3_1.py:145,161).  The theorem fails where those scripts work:
parameters on box faces, parameters without meaning under the null.  The honest conversion is a Monte-Carlo one: draw data sets
from the null, fit both models to each, see where the observed Delta chi^2 falls.

All data enter the residual linearly, so the likelihood of the data ``data + d_k`` is

    chi2_k(theta) = chi2(theta) + 2 r(theta) . g_k + c_k,      g_k = C^-1 d_k,   c_k = d_k . g_k

and one engine serves every mock (csrc/cosmofit_mock.hip, ``cf_mock_eval_device``): a row of a likelihood call names its mock.

* ``MockSet.from_shifts(engine, sn=, bao=, cmb=)``: a set from data shifts d [K, n_b]; g and c are computed with torch on the
  device (two triangular solves with the SN factor, products with the small inverse covariances).
* ``MockSet.draw(engine, theta_fid, n_mocks, seed)``: mock data = model(theta_fid) + noise of the blocks' covariances, the
  normals from ``cf_mock_normals`` under ``mock_key(seed, block)``.
* ``.log_prob(theta, mock)``, ``.chi2(theta, mock)``: the likelihood of rows theta [S, ndim] on the mocks mock [S] (int32).
* ``.best_fits(...)``: n_starts maximizations per mock in one batch of ``optimize.maximize(problem_index=True)``.
* ``.delta_chi2(fixed, ...)``: nested minus full chi^2_min per mock.
* ``significance(observed, null)``, ``goodness_of_fit(observed_chi2_min, mock_chi2_min)``: the Monte-Carlo p-value, its
  Clopper-Pearson interval, its sigma, and Wilks' sigma beside it.

The tensors live on the engine's MI355X; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from . import optimize as opt
from ._args import require_gpu, single_device_engine, stream_of
from .ensemble import _U64, _mix_int

BLOCKS = ("sn", "bao", "cmb")
_MOCK_TAG = 0x4D4F434B53455431  # "MOCKSET1": the mock draws' domain tag (the optimizer's is "OPTIMIZ1")
_GOLDEN = 0x9E3779B97F4A7C15

__all__ = ["MockSet", "MockFits", "mock_key", "significance", "goodness_of_fit", "set_library_chunk", "BLOCKS"]


def mock_key(seed: int, block: str) -> int:
    """Unsigned 64-bit key of the normals of (seed, block): seed and block each pass through a hash round of their own, as in
    ``ensemble.stream_key``; the draw uses streams 0 and 1 of it (Box-Muller) and the counter k n + i."""
    if block not in BLOCKS:
        raise ValueError(f"block must be one of {BLOCKS}")
    return _mix_int(_mix_int((seed * _GOLDEN + _MOCK_TAG) & _U64) ^ BLOCKS.index(block))


def set_library_chunk(engine, rows: int = 0):
    """Rows per chunk of the library's loop over the workspace (0: the default, ``_lib.CF_MOCK_CHUNK``).  No result depends
    on it; tests lower it to cross chunk boundaries with few rows."""
    L.check(L.lib().cf_mock_set_chunk(engine._h, int(rows)))


# ---- checks that need no device (the CPU tests reach them) -------------------------------------------------------------
def _mock_data(engine, what: str) -> dict:
    """``engine.mock_data`` of an engine that passes the gate (one without it is refused as no LikelihoodEngine)."""
    md = getattr(engine, "mock_data", None)
    single_device_engine(engine if md is not None else None, what)
    return md


def _present(engine, md: dict) -> list:
    return [b for b, has in zip(BLOCKS, (engine.n_sn > 0, engine.n_bao > 0, md["cmb_mode"] != 0)) if has]


def _check_unshiftable(md: dict, keep_observed: Sequence[str]):
    keep = set(keep_observed or ())
    left = [b for b in md["unshiftable"] if b not in keep]
    if left:
        raise ValueError(f"this likelihood has blocks whose data a mock set cannot shift: {left} (their theory vectors are not "
                         f"exported); name them in keep_observed= to keep their observed data in every mock")


def _sym_inverse(md: dict, block: str) -> np.ndarray:
    """The matrix A of the block's quadratic form r^T A r as the kernels evaluate it, symmetrised (g = A_sym d): the BAO
    inverse covariance; the CMB one, of which mode 2 uses the l_A entry alone (bao/desi_des5y_bbn_theta_star.py:110-111)."""
    if block == "bao":
        A = np.asarray(md["bao_inv_cov"], dtype=np.float64)
    else:
        A = np.asarray(md["cmb_inv_cov"], dtype=np.float64).reshape(3, 3)
        if md["cmb_mode"] == 2:
            A = np.diag([0.0, A[1, 1], 0.0])
    return 0.5 * (A + A.T)


def active_components(A: np.ndarray) -> np.ndarray:
    """Indices whose row of the inverse covariance is not all zero: the recipes with ``components=`` zero the others, which
    carry no information and stay unshifted."""
    return np.nonzero(np.any(np.asarray(A) != 0.0, axis=1))[0]


def noise_factor(A: np.ndarray):
    """(active, L): the active components of an inverse covariance and the Cholesky factor of the covariance restricted to
    them, inverse(A[active][:, active]) = L L^T."""
    act = active_components(A)
    if act.size == 0:
        raise ValueError("the inverse covariance is all zero: nothing to draw")
    cov = np.linalg.inv(A[np.ix_(act, act)])
    return act, np.linalg.cholesky(0.5 * (cov + cov.T))


# ---- the Monte-Carlo arithmetic (pure host) ------------------------------------------------------------------------------
def sigma_of_p(p: float) -> float:
    """The two-sided normal quantile of a tail probability: the conversion of ``optimize.sigma_from_delta_chi2``
    (sigma_from_delta_chi2(d, k) = sigma_of_p(chi2.sf(d, k)))."""
    from scipy import stats

    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError("p must be in [0, 1]")
    return float(stats.norm.isf(0.5 * p))


def clopper_pearson(x: int, n: int, level: float = 0.6827):
    """The exact binomial interval of x successes in n trials at confidence `level`."""
    from scipy import stats

    x, n = int(x), int(n)
    if not (n >= 1 and 0 <= x <= n and 0.0 < level < 1.0):
        raise ValueError("need n >= 1, 0 <= x <= n and 0 < level < 1")
    a = 0.5 * (1.0 - level)
    lo = 0.0 if x == 0 else float(stats.beta.ppf(a, x, n - x + 1))
    hi = 1.0 if x == n else float(stats.beta.ppf(1.0 - a, x + 1, n - x))
    return lo, hi


def _tail(observed: float, null, level: float) -> dict:
    null = np.asarray(null, dtype=np.float64).reshape(-1)
    observed = float(observed)
    if null.size < 1 or not np.all(np.isfinite(null)) or not math.isfinite(observed):
        raise ValueError("the observed value and the mock values must be finite, at least one mock")
    K, x = int(null.size), int(np.sum(null >= observed))
    p = (1 + x) / (K + 1)
    lo, hi = clopper_pearson(x, K, level)
    return dict(p=p, p_interval=(lo, hi), n_mocks=K, n_exceed=x, sigma=sigma_of_p(p), sigma_interval=(sigma_of_p(hi), sigma_of_p(lo)),
                level=level)


def significance(observed: float, null, k: int = 1, level: float = 0.6827) -> dict:
    """The observed Delta chi^2 against the Delta chi^2 of mocks drawn from the null: p = (1 + #{Delta_k >= observed}) / (K + 1)
    (never 0: the observed data count as one draw), p_interval = the Clopper-Pearson interval of #{...} / K at `level`, sigma =
    the two-sided normal quantile of p, sigma_interval, and wilks_p / wilks_sigma = what Wilks' theorem gives for k extra
    parameters (``optimize.sigma_from_delta_chi2``)."""
    from scipy import stats

    out = _tail(observed, null, level)
    out["wilks_sigma"] = opt.sigma_from_delta_chi2(observed, k)
    out["wilks_p"] = float(stats.chi2.sf(max(float(observed), 0.0), int(k)))
    return out


def goodness_of_fit(observed_chi2_min: float, mock_chi2_min, dof: Optional[int] = None, level: float = 0.6827) -> dict:
    """The same for chi^2_min: the fraction of mocks that fit worse than the data.  dof: the ``DOF`` the scripts print beside
    chi^2_min; with it wilks_p = the chi^2(dof) tail probability and wilks_sigma."""
    from scipy import stats

    out = _tail(observed_chi2_min, mock_chi2_min, level)
    if dof is not None:
        if int(dof) < 1:
            raise ValueError("dof must be >= 1")
        out["wilks_p"] = float(stats.chi2.sf(float(observed_chi2_min), int(dof)))
        out["wilks_sigma"] = sigma_of_p(out["wilks_p"])
    return out


# ---- the set ---------------------------------------------------------------------------------------------------------------
@dataclass
class MockFits:
    """The best problem of every mock: x [K, ndim], chi2 [K] (the set's own chi^2 at x), status [K] and converged [K] of the
    picked problems, status_counts over all K n_starts problems, n_like (likelihood rows), problems (``OptimizeResult``)."""
    x: np.ndarray
    chi2: np.ndarray
    status: np.ndarray
    converged: np.ndarray
    status_counts: dict
    n_like: int
    problems: object


def _device_rows(a, n: int, what: str, dev) -> torch.Tensor:
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))
    if t.dtype != torch.float64 or t.dim() != 2 or t.shape[1] != n or t.shape[0] < 1:
        raise ValueError(f"{what} must be float64 [K, {n}] with K >= 1")
    return t.to(dev).contiguous()


class MockSet:
    """K mock data sets of one engine: g [K, n_b] per shifted block and c [K] on the device (``from_shifts`` / ``draw``)."""

    def __init__(self, engine, g: dict, c: torch.Tensor, shifts: dict, theta_fid=None):
        self.engine, self.g, self.c, self.shifts = engine, g, c, shifts
        self.theta_fid = None if theta_fid is None else np.asarray(theta_fid, dtype=np.float64).reshape(-1).copy()
        self.n_mocks, self.device = int(c.shape[0]), c.device
        s = L.cf_mock_set()
        s.struct_size, s.n_mocks = C.sizeof(L.cf_mock_set), self.n_mocks
        for b in BLOCKS:
            t = g.get(b)
            setattr(s, "n_" + b, 0 if t is None else int(t.shape[1]))
            setattr(s, "g_" + b, None if t is None else t.data_ptr())
        s.c = c.data_ptr()
        self._c = s

    # -- construction --
    @classmethod
    def from_shifts(cls, engine, sn=None, bao=None, cmb=None, theta_fid=None) -> "MockSet":
        """The set whose mock k has the data ``obs + sn[k]``, ``val + bao[k]``, ``prior + cmb[k]`` (arrays or tensors [K, n_b];
        None: the block keeps its observed data).  theta_fid: the start ``best_fits`` gives every mock (optional)."""
        md = _mock_data(engine, "MockSet.from_shifts")
        given = {b: d for b, d in zip(BLOCKS, (sn, bao, cmb)) if d is not None}
        if not given:
            raise ValueError("MockSet.from_shifts needs the shifts of at least one block")
        have = _present(engine, md)
        for b in given:
            if b not in have:
                raise ValueError(f"this engine has no {b.upper()} block")
        L.lib()  # raises if the HIP library is missing
        if not torch.cuda.is_available():
            raise L.CosmofitError(-2, "mocks.MockSet lives on the device: no GPU is visible (there is no CPU fallback)")
        dev = torch.device("cuda", torch.cuda.current_device())
        n_of = dict(sn=engine.n_sn, bao=engine.n_bao, cmb=3)
        shifts = {b: _device_rows(d, n_of[b], f"the {b} shifts", dev) for b, d in given.items()}
        K = {int(d.shape[0]) for d in shifts.values()}
        if len(K) != 1:
            raise ValueError("every block's shifts must have the same number of mocks")
        g, c = {}, torch.zeros(K.pop(), dtype=torch.float64, device=dev)
        for b, d in shifts.items():
            if b == "sn":
                Lf = cls._factor(engine, dev)
                y = torch.linalg.solve_triangular(Lf, d.T, upper=False)
                g[b] = torch.linalg.solve_triangular(Lf.T, y, upper=True).T.contiguous()
            else:
                A = torch.from_numpy(_sym_inverse(md, b)).to(dev)
                g[b] = (d @ A).contiguous()  # A symmetric
            c = c + (d * g[b]).sum(dim=1)
        return cls(engine, g, c.contiguous(), shifts, theta_fid)

    @staticmethod
    def _factor(engine, dev) -> torch.Tensor:
        """The SN factor on the device, lower triangle only (the strict upper triangle of the caller's array is never read);
        uploaded once per engine and device, released by ``engine.close()``."""
        cache = engine.__dict__.setdefault("_mock_factor_dev", {})
        if dev not in cache:
            cache[dev] = torch.tril(torch.from_numpy(engine.mock_data["sn_chol"]).to(dev))
        return cache[dev]

    @classmethod
    def draw(cls, engine, theta_fid, n_mocks: int, seed: int = 0, blocks: Optional[Sequence[str]] = None,
             keep_observed: Sequence[str] = ()) -> "MockSet":
        """n_mocks data sets drawn from the model at theta_fid: for every block of `blocks` (default: every SN / BAO / CMB block
        the engine has) delta_k = L_b n_k with L_b L_b^T the block's covariance, and the shift d_k = delta_k - r_b(theta_fid), so
        that the mock data are model(theta_fid) + noise.  Components of the BAO / CMB blocks whose row of the inverse covariance
        is zero stay unshifted.  A likelihood with cosmic chronometers, a growth-rate block or ``chi2_gauss`` terms raises unless
        keep_observed names them ("cc", "fs8", "chi2_gauss"): those keep their observed data in every mock."""
        md = _mock_data(engine, "MockSet.draw")
        _check_unshiftable(md, keep_observed)
        have = _present(engine, md)
        blocks = list(have) if blocks is None else list(blocks)
        for b in blocks:
            if b not in BLOCKS:
                raise ValueError(f"blocks must be among {BLOCKS}")
            if b not in have:
                raise ValueError(f"this engine has no {b.upper()} block")
        if not blocks:
            raise ValueError("MockSet.draw needs at least one block to shift")
        K = int(n_mocks)
        if K < 1:
            raise ValueError("n_mocks must be >= 1")
        th = np.asarray(theta_fid, dtype=np.float64).reshape(-1)
        if th.size != engine.ndim or not np.all(np.isfinite(th)):
            raise ValueError(f"theta_fid must be {engine.ndim} finite numbers")
        L.lib()  # raises if the HIP library is missing
        if not torch.cuda.is_available():
            raise L.CosmofitError(-2, "mocks.MockSet lives on the device: no GPU is visible (there is no CPU fallback)")
        dev = torch.device("cuda", torch.cuda.current_device())
        parts = engine.parts(th)
        shifts = {}
        for b in blocks:
            if b == "sn":
                n, act = engine.n_sn, None
                r = parts["delta"][0]
                Lb = cls._factor(engine, dev)
            else:
                act, Lh = noise_factor(_sym_inverse(md, b))
                n = int(act.size)
                r = (md["bao_val"] - parts["bao_theory"][0]) if b == "bao" else (md["cmb_prior"] - parts["cmb_vector"][0])
                Lb = torch.from_numpy(Lh).to(dev)
            z = normals(mock_key(seed, b), K, n, device=dev)
            delta = z @ Lb.T
            rt = torch.from_numpy(np.ascontiguousarray(r)).to(dev)
            if act is None:
                shifts[b] = delta - rt[None, :]
            else:
                d = torch.zeros((K, rt.shape[0]), dtype=torch.float64, device=dev)
                idx = torch.from_numpy(act).to(dev)
                d[:, idx] = delta - rt[idx][None, :]
                shifts[b] = d
        return cls.from_shifts(engine, theta_fid=th, **shifts)

    # -- evaluation --
    def _eval(self, theta: torch.Tensor, mock: torch.Tensor, kind: int, want_cross: bool):
        what = "MockSet.log_prob"
        if not isinstance(theta, torch.Tensor) or not theta.is_cuda or theta.dtype != torch.float64:
            raise ValueError(f"{what} takes theta as a float64 tensor on the set's device")
        if theta.dim() != 2 or theta.shape[1] != self.engine.ndim:
            raise ValueError(f"{what} takes theta [S, {self.engine.ndim}]")
        if not isinstance(mock, torch.Tensor) or mock.dtype != torch.int32 or mock.shape != (theta.shape[0],):
            raise ValueError(f"{what} takes mock as an int32 tensor [S]")
        if theta.device != self.device or mock.device != self.device:
            raise ValueError(f"{what}: theta and mock must be on the device of the set")
        theta, mock = theta.contiguous(), mock.contiguous()
        S = theta.shape[0]
        out = torch.empty(S, dtype=torch.float64, device=self.device)
        cross = torch.empty((S, 3), dtype=torch.float64, device=self.device) if want_cross else None
        if S:
            with torch.cuda.device(self.device):
                stream = stream_of(self.device)
                L.check(L.lib().cf_mock_eval_device(self.engine._h, C.byref(self._c), theta.data_ptr(), S, mock.data_ptr(), int(kind),
                                                    out.data_ptr(), None if cross is None else cross.data_ptr(), stream))
        return out, cross

    def log_prob(self, theta: torch.Tensor, mock: torch.Tensor, kind: int = L.CF_OUT_LOGL, cross: bool = False):
        """The engine's value of `kind` for the rows theta [S, ndim] on the data of mocks mock [S] (int32; -1: the observed
        data), asynchronous on torch's current stream.  cross=True: (values, x [S, 3]) with x_b = r_b . g_b per block."""
        out, x = self._eval(theta, mock, kind, cross)
        return (out, x) if cross else out

    def chi2(self, theta: torch.Tensor, mock: torch.Tensor):
        return self._eval(theta, mock, L.CF_OUT_CHI2, False)[0]

    # -- fits --
    def best_fits(self, bounds=None, fixed=None, n_starts: int = 4, seed: int = 0, theta_fid=None, kind: int = L.CF_OUT_LOGL,
                  **options) -> MockFits:
        """The best fit of every mock: K n_starts problems of ``optimize.maximize`` in one batch, problem p on mock
        p // n_starts.  Start 0 of a mock is theta_fid (the set's, unless given), the others are uniform random starts drawn as
        ``optimize.best_fit`` draws them (counter = problem index).  fixed = {index: value} holds coordinates (the nested model);
        with every coordinate fixed the result is the chi^2 at that point.
        bounds: default the engine's box.  options: those of ``optimize.maximize``."""
        if bounds is None and self.engine.bounds is None:
            raise ValueError("best_fits needs bounds (the engine has no prior box)")
        b = opt._bounds(self.engine.bounds if bounds is None else bounds)
        ndim = b.shape[0]
        if ndim != self.engine.ndim:
            raise ValueError(f"bounds must be [{self.engine.ndim}, 2]")
        all_fixed = fixed is not None and len({opt._index(k, ndim) for k in fixed}) == ndim
        fx = {opt._index(k, ndim): float(v) for k, v in fixed.items()} if all_fixed else opt._fixed(fixed, ndim, b)
        o = opt._options(**{**opt.DEFAULTS, **options})
        n_starts = int(n_starts)
        if n_starts < 1:
            raise ValueError("n_starts must be >= 1")
        fid = self.theta_fid if theta_fid is None else np.asarray(theta_fid, dtype=np.float64).reshape(-1)
        if fid is None or fid.size != ndim:
            raise ValueError(f"best_fits needs theta_fid [{ndim}] (given here, to from_shifts or to draw)")
        fid = fid.copy()
        for i, v in fx.items():
            fid[i] = v
        if not np.all((fid > b[:, 0]) & (fid < b[:, 1])):
            raise ValueError("theta_fid (with the fixed values) must lie strictly inside the bounds")
        Lm, lib = require_gpu("optimize.maximize")
        K, P = self.n_mocks, self.n_mocks * n_starts
        if all_fixed:  # a nested model without a free parameter: nothing to maximise, its chi^2 is the chi^2 at the point
            x = np.tile(fid, (K, 1))
            chi2 = self.chi2(torch.from_numpy(x).to(self.device), torch.arange(K, dtype=torch.int32, device=self.device)).cpu().numpy()
            return MockFits(x=x, chi2=chi2, status=np.full(K, opt.CONVERGED), converged=np.ones(K, dtype=bool), status_counts={},
                            n_like=K, problems=None)
        fr = [i for i in range(ndim) if i not in fx]
        p = opt._params(b, fr, o)
        x0 = np.tile(fid, (P, 1))
        u, th = opt._starts(p, x0, opt.opt_key(seed, opt.PURPOSE_BEST_FIT), Lm, lib)
        u0, th0 = opt._starts(p, x0[::n_starts], None, Lm, lib)
        u[::n_starts], th[::n_starts] = u0, th0

        def objective(theta, problem):
            return self.log_prob(theta, torch.div(problem, n_starts, rounding_mode="floor").to(torch.int32), kind)

        res = opt._run(objective, p, u.contiguous(), th.contiguous(), Lm, lib, True)
        pick = np.array([opt._best_of(res, np.arange(k * n_starts, (k + 1) * n_starts))[0] for k in range(K)])
        x = res.x[pick]
        chi2 = self.chi2(torch.from_numpy(np.ascontiguousarray(x)).to(self.device),
                         torch.arange(K, dtype=torch.int32, device=self.device)).cpu().numpy()
        return MockFits(x=x, chi2=chi2, status=res.status[pick], converged=res.converged[pick], status_counts=res.status_counts(),
                        n_like=res.n_like + K, problems=res)

    def delta_chi2(self, fixed, bounds=None, n_starts: int = 4, seed: int = 0, tol: float = 1e-6, theta_fid=None, **options) -> dict:
        """chi^2_min of the nested model (the coordinates of `fixed` held) minus chi^2_min of the full model, per mock, as
        computed: dict(delta_chi2 [K], chi2_full [K], chi2_nested [K], n_below = the number of mocks with Delta chi^2 < -tol (a
        nested model cannot fit better: these are optimizer failures, shown and not clipped away), full, nested (``MockFits``),
        n_like)."""
        if not fixed:
            raise ValueError("delta_chi2 needs the coordinates the nested model holds fixed")
        full = self.best_fits(bounds=bounds, n_starts=n_starts, seed=seed, theta_fid=theta_fid, **options)
        nested = self.best_fits(bounds=bounds, fixed=fixed, n_starts=n_starts, seed=seed, theta_fid=theta_fid, **options)
        d = nested.chi2 - full.chi2
        return dict(delta_chi2=d, chi2_full=full.chi2, chi2_nested=nested.chi2, n_below=int(np.sum(d < -float(tol))), tol=float(tol),
                    full=full, nested=nested, n_like=full.n_like + nested.n_like)


def normals(key: int, K: int, n: int, k0: int = 0, device=None) -> torch.Tensor:
    """Standard normals [K, n] of mocks k0 .. k0 + K - 1 on the device (``cf_mock_normals``): the value of (key, k, i) does not
    depend on how a set is cut into pieces."""
    K, n, k0 = int(K), int(n), int(k0)
    if K < 0 or n < 1 or k0 < 0:
        raise ValueError("normals needs K >= 0, n >= 1, k0 >= 0")
    lib = L.lib()
    if not torch.cuda.is_available():
        raise L.CosmofitError(-2, "mocks.normals runs in the library's HIP kernel: no GPU is visible")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    out = torch.empty((K, n), dtype=torch.float64, device=dev)
    if K:
        with torch.cuda.device(dev):
            L.check(lib.cf_mock_normals(key & _U64, k0, K, n, out.data_ptr(), stream_of(dev)))
    return out
