"""
Quasar Hubble-diagram likelihoods: the five emcee fits of the reference's quasars/ directory (Risaliti-Lusso quasars as
standard candles with a free intrinsic scatter, alone or joint with SNe and DESI BAO), on the GPU.

These scripts use an older distance algorithm than the rest of the engine (a 3000-node cumulative trapezoid of 1 / E to
max(z_qsr), LINEAR interpolation, a per-datum trapezoid for BAO) and a dark energy of their own,
f_DE = (n X / (1 + (n - 1) X))^(p (1 + w0)), X = (1 + z)^k.  The arithmetic lives in csrc/cosmofit_quasar.hip behind
``cf_create_quasar`` (include/cosmofit.h); a recipe here is a description: the theta order, (n, k, p), which blocks, the box.

    lk = quasars.build("quasars/qsr_union3.py", qsr=(z, mu, sigma_mu), sn=(z_cmb, z_hel, mu_sn, cov_sn))
    lk.log_probability(theta_batch)          # the script's log_posterior, batched on the GPU
    lk.chi2_parts(theta_batch)               # (chi2_sn, chi2_quasars, chi2_bao) per row

``lk.engine`` is an ordinary ``LikelihoodEngine``: ``engine.torch_log_prob()`` drives ``ensemble.ShardedEnsemble``.
The data arrays are what the scripts' own loaders return; BAO data is the structured array of y2025BAO (fields z, value,
quantity) or a dict with the same keys.
"""
from dataclasses import dataclass
from typing import Sequence, Tuple

import numpy as np

from .engine import LikelihoodEngine, Param, solve_mode_of

H0 = 70.0        # fixed in every quasar script
N_GRID = 3000    # np.linspace(0, max z, num=3000)
BAO_QTY = {"DV_over_rs": 0, "DM_over_rs": 1, "DH_over_rs": 2}


@dataclass(frozen=True)
class QuasarRecipe:
    theta: Sequence[str]             # parameter order: dM_qsr, s, offset (SN M or dM), rd, Om, w0
    nkp: Tuple[float, float, float]  # (n, k, p) of f_DE
    bounds: Sequence[Tuple[float, float]]  # strict box of log_prior, 0 inside
    sn: bool = False                 # SN block (the descriptor's Cholesky solve)
    sn_grid: bool = False            # the SN block has a grid of its own, to max z_sn (else the quasar grid)
    sn_zhel: bool = False            # (1 + z_hel) in the SN luminosity distance
    bao: bool = False                # DESI BAO, one trapezoid per datum


RECIPES = {
    "quasars/qsr_pantheon.py": QuasarRecipe(("dM_qsr", "s", "offset", "Om", "w0"), (2, 2, 3),
                                            ((-0.5, 0.5), (0, 3), (-20, -19), (0, 1), (-4, 0)), sn=True),
    "quasars/qsr_des5y.py": QuasarRecipe(("dM_qsr", "s", "offset", "Om", "w0"), (2, 2, 3),
                                         ((-0.5, 0.5), (0, 3), (-0.6, 0.6), (0, 0.8), (-2, 0)), sn=True),
    "quasars/qsr_union3.py": QuasarRecipe(("dM_qsr", "s", "offset", "Om", "w0"), (4, 3, 4),
                                          ((-0.5, 0.5), (0, 2.5), (-0.4, 0.3), (0, 1), (-3, 0)), sn=True),
    "quasars/qsr_desi.py": QuasarRecipe(("dM_qsr", "s", "rd", "Om", "w0"), (4, 3, 4),
                                        ((-0.6, 0.5), (0, 1.5), (110, 155), (0, 0.6), (-1.6, 0)), bao=True),
    # no bounds array in the script: the inequalities of its log_prior
    "quasars/qsr_des5y_desi.py": QuasarRecipe(("dM_qsr", "s", "offset", "rd", "Om", "w0"), (2, 3, 2),
                                              ((-1, 1), (0, 2.5), (-0.6, 0.6), (110, 170), (0, 0.6), (-1.5, 0)),
                                              sn=True, sn_grid=True, sn_zhel=True, bao=True),
}


def bao_arrays(data):
    """(z, value, quantity code) of a y2025BAO structured array or a dict with the keys z, value, quantity."""
    q = data["quantity"]
    qty = np.array([BAO_QTY[str(x)] if not isinstance(x, (int, np.integer)) else int(x) for x in q], dtype=np.int32)
    return np.asarray(data["z"], dtype=np.float64), np.asarray(data["value"], dtype=np.float64), qty


class QuasarLikelihood:
    """One quasar script on the GPU.  Every method takes one theta [ndim] or a batch [W, ndim]."""

    def __init__(self, recipe: QuasarRecipe, *, qsr, sn=None, bao=None, solve="auto", device: int = 0):
        self.recipe = recipe
        self.ndim = len(recipe.theta)
        self.bounds = np.asarray(recipe.bounds, dtype=np.float64)
        if (sn is not None) != recipe.sn or (bao is not None) != recipe.bao:
            raise ValueError("this recipe needs " + ", ".join(n for n, f in (("sn", recipe.sn), ("bao", recipe.bao)) if f)
                             + " besides qsr, and nothing else")
        qz, qmu, qsig = (np.ascontiguousarray(a, dtype=np.float64) for a in qsr)
        idx = {name: k for k, name in enumerate(recipe.theta)}
        params = {"H0": Param(fixed=H0), "Om": Param(idx["Om"]), "w0": Param(idx["w0"])}
        if "offset" in idx:
            params["offset"] = Param(idx["offset"])
        if "rd" in idx:
            params["rd"] = Param(idx["rd"])
        quasar = dict(z=qz, mu=qmu, sigma=qsig, offset=Param(idx["dM_qsr"]), scatter=Param(idx["s"]), nkp=recipe.nkp,
                      z_top=float(np.max(qz)), sn_zhel=recipe.sn_zhel)
        sn_block = None
        if sn is not None:
            z_cmb, z_hel, obs, cov = sn
            z_cmb = np.ascontiguousarray(z_cmb, dtype=np.float64)
            sn_block = dict(z_cmb=z_cmb, z_hel=np.ascontiguousarray(z_hel, dtype=np.float64),
                            obs=np.ascontiguousarray(obs, dtype=np.float64),
                            chol=np.linalg.cholesky(np.asarray(cov, dtype=np.float64)))
            if recipe.sn_grid:
                quasar["sn_z_top"] = float(np.max(z_cmb))
        if bao is not None:
            data, cov = bao
            bz, bv, bq = bao_arrays(data)
            quasar["bao"] = dict(z=bz, val=bv, qty=bq, inv_cov=np.linalg.inv(np.asarray(cov, dtype=np.float64)))
        self.engine = LikelihoodEngine(ndim=self.ndim, z_max=quasar["z_top"], n_grid=N_GRID, params=params, sn=sn_block,
                                       bounds=self.bounds, prior_normalised=False, solve_mode=solve_mode_of(solve),
                                       device=device, quasar=quasar)

    def log_probability(self, theta):
        """The script's log_posterior: -inf outside the strict box."""
        return self.engine.log_probability(theta)

    log_posterior = log_probability

    def log_likelihood(self, theta):
        """-0.5 (chi2_sn + chi2_bao) - 0.5 (chi2_quasars + sum ln(sigma^2 + s^2))."""
        return self.engine.log_likelihood(theta)

    def chi_squared(self, theta):
        """chi2_sn + chi2_quasars + chi2_bao: the scripts' "chi squared total"."""
        return self.engine.chi_squared(theta)

    def chi2_parts(self, theta):
        """[W, 3] (chi2_sn, chi2_quasars, chi2_bao), 0 for an absent block; [3] for one theta."""
        th = np.asarray(theta, dtype=np.float64)
        out = self.engine.quasar_parts(th)["chi2_blocks"]
        return out[0] if th.ndim == 1 else out

    def theory(self, theta):
        """dict(mu_sn, mu_qsr, bao_theory, chi2_blocks) of a batch: mu at the SN and quasar redshifts and the BAO predictions."""
        return self.engine.quasar_parts(theta)

    def close(self):
        self.engine.close()


def build(script: str, qsr, sn=None, bao=None, solve: str = "auto", device: int = 0) -> QuasarLikelihood:
    """``build("quasars/qsr_desi.py", qsr=(z, mu, sigma), bao=(bao_data, bao_cov))``."""
    if script not in RECIPES:
        raise KeyError(f"no quasar recipe for {script!r}; known: {sorted(RECIPES)}")
    return QuasarLikelihood(RECIPES[script], qsr=qsr, sn=sn, bao=bao, solve=solve, device=device)
