"""
Which data carry a chi^2: per-datum attribution and leave-one-out residuals of a chain that lives on the device.

The reference reads a Delta chi^2 between two models as a statement about individual data (README: the supernovae on either side
of ``z_turn``).  ``fit_report`` divides raw residuals by ``sqrt(C_ii)``; with a dense covariance that is no test statistic --
neighbouring supernovae share calibration modes, so a raw 2-sigma pull may be perfectly predicted by its neighbours.  The
quantities that are one all come from a single vector per sample, ``g = K r`` with ``K = C^-1`` (csrc/cosmofit_infl.hip,
``cf_infl_device``; the residual rows of the likelihood's accessor path never leave the device):

* ``contrib_i = r_i g_i``: ``sum_i contrib_i = chi^2`` exactly, so ``contrib_i(theta_A) - contrib_i(theta_B)`` is an exact
  additive split of a Delta chi^2 over the data (``attribution``);
* ``loo_i = g_i / K_ii``: datum i minus its prediction from all the others, with error ``1 / sqrt(K_ii)`` and z-score
  ``z_i = g_i / sqrt(K_ii)``;
* chi^2 without datum i is ``chi^2 - g_i^2 / K_ii`` -- no refit of the covariance.

* ``Precision(matrix, device, from_factor)``: K on a device (``engine.precision(block)`` builds and keeps the engine's).
* ``rows(engine, theta, block, want)``: the row arrays [S, n] and the per-sample table (``COLUMNS``) on the device.
* ``Accumulator`` / ``report(engine, chain, weights, block, thresholds)``: per datum over a chain, the posterior mean and scatter
  of ``z_i`` and ``contrib_i`` and the fraction of the weight in which ``|z_i|`` lies beyond each threshold; a chain fed in
  pieces gives the same bits as one call.
* ``attribution(engine, theta_a, theta_b, block, order)``: ``delta_i``, its cumulative sum in redshift order, and the total.

block: "sn" or "bao".  The inputs are float64 tensors on the engine's MI355X; there is no CPU fallback.  The per-datum
accumulators run through the fit report's ``resid_datum_kernel`` and inherit its speed.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from . import fit_report as F
from ._args import ptr, row_weights, sample_rows, stream_of

COLUMNS = L.INFL_COLUMNS
WANT = ("contrib", "z", "loo", "g")
_REPORT_KEYS = ("weights", "block", "thresholds")


class Precision:
    """K = C^-1 on one device (``cf_prec``).  matrix: the Cholesky factor of C (lower triangle read; from_factor=True) or the
    precision matrix itself (from_factor=False: symmetrised; a zero row and column is a datum the likelihood ignores)."""

    def __init__(self, matrix, device: int = 0, from_factor: bool = True):
        m = np.ascontiguousarray(matrix, dtype=np.float64)
        if m.ndim != 2 or m.shape[0] != m.shape[1] or m.shape[0] < 1:
            raise ValueError("Precision takes a square matrix")
        self.n, self.device = int(m.shape[0]), int(device)
        self._p = C.c_void_p()
        create = L.lib().cf_prec_create if from_factor else L.lib().cf_prec_create_inv
        L.check(create(ptr(m), self.n, self.n, self.device, C.byref(self._p)))

    def close(self):
        if getattr(self, "_p", None) is not None and self._p.value:
            L.lib().cf_prec_destroy(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def diag(self) -> np.ndarray:
        """K_ii, [n] numpy."""
        out = np.empty(self.n)
        L.check(L.lib().cf_prec_diag(self._p, ptr(out)))
        return out

    def loo_sigma(self) -> np.ndarray:
        """1 / sqrt(K_ii): the error of a datum's leave-one-out residual (inf for a datum the likelihood ignores)."""
        with np.errstate(divide="ignore"):
            return 1.0 / np.sqrt(self.diag())

    def apply(self, rows: torch.Tensor, S: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """g [S, n] = rows[:S, :n] K on the device of this matrix, asynchronous on torch's current stream (``cf_prec_apply_device``).
        rows: float64 [>= S, pitch >= n] with contiguous columns; columns >= n and rows >= S are never read."""
        if not isinstance(rows, torch.Tensor) or rows.dtype != torch.float64 or rows.dim() != 2 or rows.stride(1) != 1:
            raise ValueError("Precision.apply takes a float64 tensor [S, >= n] with contiguous columns")
        if not rows.is_cuda or rows.device.index != self.device:
            raise ValueError("Precision.apply takes rows on the device of the matrix")
        S = rows.shape[0] if S is None else int(S)
        if not 0 <= S <= rows.shape[0] or rows.shape[1] < self.n:
            raise ValueError("Precision.apply: S rows of at least n columns")
        g = torch.empty((S, self.n), dtype=torch.float64, device=rows.device) if out is None else out
        if S:
            with torch.cuda.device(rows.device):
                L.check(L.lib().cf_prec_apply_device(self._p, rows.data_ptr(), rows.stride(0), S, g.data_ptr(), g.stride(0),
                                                     stream_of(rows.device)))
        return g


def _to_device(a: np.ndarray) -> torch.Tensor:
    """A host array on torch's current device (a module attribute so that a test can keep it on the host)."""
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", torch.cuda.current_device()))


def _theta_rows(engine, theta, what: str) -> torch.Tensor:
    """theta as rows [S, ndim] on the device: a tensor as ``fit_report`` takes it, or host numbers (one row or several)."""
    if not isinstance(theta, torch.Tensor):
        th = np.atleast_2d(np.asarray(theta, dtype=np.float64))
        if th.ndim != 2 or th.shape[1] != engine.ndim:
            raise ValueError(f"{what} takes theta [{engine.ndim}] or [S, {engine.ndim}]")
        theta = _to_device(th)
    elif theta.dim() == 1:
        theta = theta[None, :]
    return sample_rows(theta, engine.ndim, what)


def set_library_chunk(engine, rows: int = 0):
    """Rows per chunk of the library's own loop over the workspace (0: the default, ``_lib.CF_INFL_CHUNK``).  No result depends on
    it; tests lower it to cross chunk boundaries with few rows."""
    L.check(L.lib().cf_infl_set_chunk(engine._h, int(rows)))


def _launch(engine, x: torch.Tensor, w: Optional[torch.Tensor], block: str, want: Sequence[str], want_sample: bool,
            thresholds: np.ndarray, acc_z: Optional[F.DatumAcc], acc_contrib: Optional[F.DatumAcc]) -> dict:
    """One cf_infl_device call on torch's current stream (x and w checked by the caller)."""
    n = int(engine.n_sn if block == "sn" else engine.n_bao)
    S, dev = x.shape[0], x.device
    res = {k: torch.empty((S, n), dtype=torch.float64, device=dev) for k in want}
    if want_sample:
        res["sample"] = torch.empty((S, L.CF_INFL_NCOL), dtype=torch.float64, device=dev)
    if S == 0:
        return res
    out = L.cf_infl_out()
    out.struct_size = C.sizeof(L.cf_infl_out)
    for k, t in res.items():
        setattr(out, k, t.data_ptr())
    prec = engine.precision(block)
    with torch.cuda.device(dev):
        L.check(L.lib().cf_infl_device(engine._h, prec._p, x.data_ptr(), S, None if w is None else w.data_ptr(), L.RESID_BLOCKS[block],
                                       ptr(thresholds) if thresholds.size else None, int(thresholds.size),
                                       C.byref(out) if res else None, None if acc_z is None else C.byref(acc_z.c),
                                       None if acc_contrib is None else C.byref(acc_contrib.c), stream_of(dev)))
    return res


def _named(sample: torch.Tensor) -> dict:
    return {name: sample[:, j] for j, name in enumerate(COLUMNS)}


def rows(engine, theta, block: str = "sn", want: Sequence[str] = WANT) -> dict:
    """For every row of theta [S, ndim] (or one theta [ndim]): the arrays named in `want` ("contrib", "z", "loo", "g"), each
    [S, n] on the device, and ``sample``: the per-sample table as named columns [S] (``COLUMNS``: chi2 = sum_i contrib_i, the
    largest |z_i| and its index, the largest deletion drop g_i^2 / K_ii and its index).  Asynchronous on torch's current stream;
    a row's values do not depend on S or on its position."""
    F._check_engine(engine, block, "influence.rows")
    want = tuple(want)
    unknown = set(want) - set(WANT)
    if unknown:
        raise ValueError(f"want must be among {WANT}, got {sorted(unknown)}")
    x = _theta_rows(engine, theta, "influence.rows")
    res = _launch(engine, x, None, block, want, True, np.empty(0), None, None)
    res["sample"] = _named(res["sample"])
    return res


class Accumulator:
    """The running per-datum state of a chain's z-scores and chi^2 contributions on a device: feed it consecutive pieces of the
    chain with ``update`` (the result is the same bits for every cut), read it with ``result``."""

    def __init__(self, engine, block: str = "sn", thresholds: Sequence[float] = (2.0, 3.0), device=None):
        self.n = F._check_engine(engine, block, "influence.Accumulator")
        self.engine, self.block, self.thresholds = engine, block, F._thresholds(thresholds)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.z = F.DatumAcc(self.n, int(self.thresholds.size), self.device)
        self.contrib = F.DatumAcc(self.n, 0, self.device)

    def update(self, samples: torch.Tensor, weights: Optional[torch.Tensor] = None, want_sample: bool = False):
        """Continue over the rows of samples; returns the per-sample table [S, len(COLUMNS)] when want_sample, else None."""
        x = sample_rows(samples, self.engine.ndim, "influence.Accumulator.update")
        if x.device != self.device:
            raise ValueError("the accumulator lives on another device than the samples")
        w = row_weights(weights, x, "influence.Accumulator.update")
        return _launch(self.engine, x, w, self.block, (), want_sample, self.thresholds, self.z, self.contrib).get("sample")

    def result(self) -> dict:
        """Per datum, numpy arrays of the block's n data: z_mean, z_std (ddof 0), contrib_mean, contrib_std, exceed [n_thr, n]
        (the fraction of the weight with |z_i| beyond each threshold), loo_sigma = 1 / sqrt(K_ii) beside fit_report's sigma =
        sqrt(C_ii), redshift, thresholds, n_used, n_skipped, w_sum (a datum no row was used for gives NaN)."""
        z_mean, z_std = self.z.mean_std()
        c_mean, c_std = self.contrib.mean_std()
        w_sum = self.z.w_sum.cpu().numpy()
        with np.errstate(invalid="ignore", divide="ignore"):
            exceed = self.z.exceed.cpu().numpy() / w_sum[None, :]
        red = self.engine.sn_z if self.block == "sn" else self.engine.bao_z
        return dict(z_mean=z_mean, z_std=z_std, contrib_mean=c_mean, contrib_std=c_std, exceed=exceed,
                    loo_sigma=self.engine.precision(self.block).loo_sigma(), sigma=self.engine.resid_sigma(self.block),
                    redshift=None if red is None else red.copy(), thresholds=self.thresholds.copy(),
                    n_used=self.z.n_used.cpu().numpy(), n_skipped=self.z.n_skipped.cpu().numpy(), w_sum=w_sum)


def report(engine, chain: torch.Tensor, weights: Optional[torch.Tensor] = None, block: str = "sn",
           thresholds: Sequence[float] = (2.0, 3.0)) -> dict:
    """One pass over the rows of chain [S, ndim]: dict(sample [S, len(COLUMNS)] on the device, columns, datum = the dict of
    ``Accumulator.result``).  weights: one per row, finite and >= 0 (a row of weight 0 is skipped and counted)."""
    acc = Accumulator(engine, block, thresholds, device=chain.device if isinstance(chain, torch.Tensor) else None)
    sample = acc.update(chain, weights, want_sample=True)
    return dict(sample=sample, columns=COLUMNS, datum=acc.result())


def chain_report(engine, chain: torch.Tensor, **kw) -> dict:
    """``report`` with its keywords checked by name: what ``ShardedEnsemble.influence`` and ``DeviceNestedSampler.influence``
    return.  Keywords: weights, block, thresholds."""
    unknown = set(kw) - set(_REPORT_KEYS)
    if unknown:
        raise TypeError(f"influence got unexpected keyword(s) {sorted(unknown)}; valid: {list(_REPORT_KEYS)}")
    return report(engine, chain, **kw)


def _order(engine, block: str, n: int, order) -> np.ndarray:
    """The permutation the cumulative sum runs in: ascending redshift (stable) by default."""
    if order is None:
        red = engine.sn_z if block == "sn" else engine.bao_z
        return np.argsort(np.asarray(red, dtype=np.float64), kind="stable")
    order = np.asarray(order)
    if order.shape != (n,) or not np.array_equal(np.sort(order), np.arange(n)):
        raise ValueError(f"order must be a permutation of the block's {n} data")
    return order.astype(np.int64)


def attribution(engine, theta_a, theta_b, block: str = "sn", order=None) -> dict:
    """The exact split of a Delta chi^2 over the data: delta_i = contrib_i(theta_a) - contrib_i(theta_b).

    theta_a, theta_b: single rows [ndim] or paired chain rows [S, ndim] (row s of one against row s of the other).  Returns numpy
    arrays: delta [n] (paired rows: the mean over the pairs), delta_std [n] (ddof 0; zeros for one pair), order [n] (the
    permutation of the cumulative sum: ascending redshift, or the one given), redshift [n] in that order, cumulative [n] =
    cumsum(delta[order]), total = chi2(theta_a) - chi2(theta_b) of the block (paired rows: the mean; total_rows [S] has every
    pair's), and chi2_a, chi2_b [S].  sum_i delta_i = total up to rounding."""
    n = F._check_engine(engine, block, "influence.attribution")
    xa = _theta_rows(engine, theta_a, "influence.attribution")
    xb = _theta_rows(engine, theta_b, "influence.attribution")
    if xa.shape != xb.shape:
        raise ValueError("theta_a and theta_b must be one row each or the same number of paired rows")
    if xa.shape[0] < 1:
        raise ValueError("influence.attribution needs at least one pair of rows")
    perm = _order(engine, block, n, order)
    a = rows(engine, xa, block, want=("contrib",))
    b = rows(engine, xb, block, want=("contrib",))
    d = (a["contrib"] - b["contrib"]).cpu().numpy()
    chi2_a, chi2_b = a["sample"]["chi2"].cpu().numpy(), b["sample"]["chi2"].cpu().numpy()
    total_rows = chi2_a - chi2_b
    delta = d.mean(axis=0)
    red = engine.sn_z if block == "sn" else engine.bao_z
    return dict(delta=delta, delta_std=d.std(axis=0), order=perm, redshift=None if red is None else np.asarray(red)[perm],
                cumulative=np.cumsum(delta[perm]), total=float(total_rows.mean()), total_rows=total_rows, chi2_a=chi2_a,
                chi2_b=chi2_b)
