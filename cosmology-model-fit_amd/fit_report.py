"""
The fit report of a chain that lives on the device: residual statistics of every sample and of every datum.

Every ``main()`` of the reference ends with the same block: the model at the central parameters, the data residuals, then
R^2, RMSD, the skewness and kurtosis of the residuals, the degrees of freedom and chi^2 (sn/pantheon.py:150-183,
bao/desi_fs_lya.py:96-113), and the residuals against ``sqrt(diag(cov))`` with a normal fit (sn/plotting.py:46-71).  Here the
posterior-predictive form of that block, computed where the chain is (csrc/cosmofit_resid.hip, ``cf_resid_device``): the
residual rows of the likelihood's accessor path never leave the device.

* ``sample_stats(engine, samples, block)``: the statistics of every row, [S, ncol] with the columns ``COLUMNS``, and the
  ``chi2_blocks`` [S, 10] of ``engine.parts``.
* ``datum_stats(engine, samples, weights, block, thresholds, chunk)``: per datum over the rows, the posterior mean and scatter
  of its residual, its mean pull, and the fraction of the weight in which it lies beyond each threshold (in units of sigma).
* ``report(engine, samples, weights, ...)``: both from ONE pass (the likelihood is evaluated once per row).
* ``summary(engine, samples, weights, center)``: what the scripts print -- the statistics at the central row, dof, chi^2 --
  with the 15.9 / 50 / 84.1 percentiles of every per-sample statistic over the posterior.
* ``chain_report(engine, samples, **kw)``: ``report`` plus ``summary`` from one pass; what ``ShardedEnsemble.fit_report`` and
  ``DeviceNestedSampler.fit_report`` return.

block: "sn" (r = the residual vector, y = obs - mu_corr) or "bao" (r = val - bao_theory, y = val).  The inputs are float64
tensors on the engine's MI355X; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from . import _args, chain_stats, marginals

COLUMNS = L.RESID_COLUMNS
BLOCK_COLUMNS = L.CHI2_BLOCK_COLUMNS
SUMMARY_Q = (15.9, 50.0, 84.1)

# the reductions of ``summary`` (module attributes so that a test can put host stand-ins behind its arithmetic)
_percentile = chain_stats.percentile
_weighted_quantile = marginals._weighted_quantile


def _check_engine(engine, block: str, what: str) -> int:
    """The rules of cf_resid_device on the engine's facts, before any device work; returns the number of data of the block."""
    _args.single_device_engine(engine, what)
    if block not in L.RESID_BLOCKS:
        raise ValueError(f"block must be one of {sorted(L.RESID_BLOCKS)} (the cosmic-chronometer and growth-rate blocks export no "
                         f"theory vector)")
    n = int(engine.n_sn if block == "sn" else engine.n_bao)
    if n < 1:
        raise ValueError(f"{what}: this engine has no {block.upper()} block")
    return n


def _thresholds(thresholds) -> np.ndarray:
    t = np.atleast_1d(np.asarray(thresholds, dtype=np.float64)) if thresholds is not None and len(thresholds) else np.empty(0)
    if t.ndim != 1 or t.size > L.CF_RESID_MAX_THR:
        raise ValueError(f"at most {L.CF_RESID_MAX_THR} thresholds")
    if not (np.isfinite(t).all() and (t >= 0).all()):
        raise ValueError("thresholds must be finite and >= 0")
    return np.ascontiguousarray(t)


def dof(n_data: int, ndim: int) -> int:
    """``len(z_cmb) - len(best_fit)`` of the scripts (sn/pantheon.py:181, bao/desi_fs_lya.py:97)."""
    return int(n_data) - int(ndim)


def set_library_chunk(engine, rows: int = 0):
    """Rows per chunk of the library's own loop over the workspace (0: the default, ``_lib.CF_RESID_CHUNK``).  No result
    depends on it; tests lower it to cross chunk boundaries with few rows."""
    L.check(L.lib().cf_resid_set_chunk(engine._h, int(rows)))


class DatumAcc:
    """The arrays of one ``cf_resid_acc`` on a device, and the struct that points at them (``c``)."""

    def __init__(self, n: int, n_thr: int, device):
        f64 = dict(dtype=torch.float64, device=device)
        self.w_sum, self.mean, self.m2 = (torch.zeros(n, **f64) for _ in range(3))
        self.exceed = torch.zeros((n_thr, n), **f64)
        self.n_used, self.n_skipped = (torch.zeros(n, dtype=torch.int64, device=device) for _ in range(2))
        a = L.cf_resid_acc()
        a.struct_size, a.n, a.n_thr = C.sizeof(L.cf_resid_acc), n, n_thr
        a.w_sum, a.mean, a.m2 = self.w_sum.data_ptr(), self.mean.data_ptr(), self.m2.data_ptr()
        a.exceed = self.exceed.data_ptr() if n_thr else None
        a.n_used, a.n_skipped = self.n_used.data_ptr(), self.n_skipped.data_ptr()
        self.c = a

    def mean_std(self):
        """(mean, std with ddof 0) as numpy; a datum no row was used for gives NaN."""
        w_sum = self.w_sum.cpu().numpy()
        mean = np.where(w_sum > 0, self.mean.cpu().numpy(), np.nan)
        with np.errstate(invalid="ignore", divide="ignore"):
            return mean, np.sqrt(self.m2.cpu().numpy() / w_sum)


class Accumulator(DatumAcc):
    """The running per-datum state of ``cf_resid_acc`` on a device (a ``DatumAcc``: the arrays are its own ``w_sum``, ``mean``,
    ...): feed it consecutive pieces of a chain with ``update`` (the result is the same bits for every cut), read it with
    ``result``."""

    def __init__(self, engine, block: str = "sn", thresholds: Sequence[float] = (2.0, 3.0), device=None):
        self.n = _check_engine(engine, block, "Accumulator")
        self.engine, self.block, self.thresholds = engine, block, _thresholds(thresholds)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        super().__init__(self.n, int(self.thresholds.size), self.device)

    def update(self, samples: torch.Tensor, weights: Optional[torch.Tensor] = None):
        x = _args.sample_rows(samples, self.engine.ndim, "Accumulator.update")
        _launch(self.engine, x, _args.row_weights(weights, x, "Accumulator.update"), self.block, self, False)
        return self

    def result(self) -> dict:
        """mean, std (ddof 0), pull_mean = mean / sigma, exceed [n_thr, n] as fractions of the weight, sigma, z, thresholds,
        n_used, n_skipped, w_sum: numpy arrays of the block's n data (a datum no row was used for gives NaN)."""
        sigma = self.engine.resid_sigma(self.block)
        mean, std = self.mean_std()
        w_sum = self.w_sum.cpu().numpy()
        with np.errstate(invalid="ignore", divide="ignore"):
            exceed = self.exceed.cpu().numpy() / w_sum[None, :]
        z = self.engine.sn_z if self.block == "sn" else self.engine.bao_z
        return dict(mean=mean, std=std, pull_mean=mean / sigma, exceed=exceed, sigma=sigma, z=None if z is None else z.copy(),
                    thresholds=self.thresholds.copy(), n_used=self.n_used.cpu().numpy(), n_skipped=self.n_skipped.cpu().numpy(),
                    w_sum=w_sum)


def _launch(engine, x: torch.Tensor, w: Optional[torch.Tensor], block: str, acc: Optional[Accumulator], want_sample: bool):
    """One cf_resid_device call on torch's current stream (x and w checked by the caller): (sample [S, ncol], chi2_blocks
    [S, 10]) or (None, None)."""
    S, dev = x.shape[0], x.device
    if acc is not None and acc.device != dev:
        raise ValueError("the accumulator lives on another device than the samples")
    sample = torch.empty((S, L.CF_RS_NCOL), dtype=torch.float64, device=dev) if want_sample else None
    blocks = torch.empty((S, 10), dtype=torch.float64, device=dev) if want_sample else None
    if S == 0:
        return sample, blocks
    thr = acc.thresholds if acc is not None else np.empty(0)
    with torch.cuda.device(dev):
        L.check(L.lib().cf_resid_device(engine._h, x.data_ptr(), S, None if w is None else w.data_ptr(), L.RESID_BLOCKS[block],
                                        _args.ptr(thr) if thr.size else None, int(thr.size),
                                        None if sample is None else sample.data_ptr(), None if blocks is None else blocks.data_ptr(),
                                        None if acc is None else C.byref(acc.c), _args.stream_of(dev)))
    return sample, blocks


def sample_stats(engine, samples: torch.Tensor, block: str = "sn"):
    """(stats [S, len(COLUMNS)], chi2_blocks [S, 10]) on the samples' device, asynchronous on torch's current stream: for every
    row of samples [S, ndim] the residual statistics in the order of ``COLUMNS`` and the chi^2 shares in the order of
    ``BLOCK_COLUMNS``.  A row's values do not depend on S or on its position."""
    _check_engine(engine, block, "sample_stats")
    return _launch(engine, _args.sample_rows(samples, engine.ndim, "sample_stats"), None, block, None, True)


def datum_stats(engine, samples: torch.Tensor, weights: Optional[torch.Tensor] = None, block: str = "sn",
                thresholds: Sequence[float] = (2.0, 3.0), chunk: Optional[int] = None) -> dict:
    """Per datum over the rows of samples (``Accumulator.result``): mean, std, pull_mean, exceed, sigma, z, n_used, n_skipped.
    chunk: rows per call (None: one call; the library walks its workspace in chunks of its own); the accumulator is carried
    from call to call, so the result has the same bits for every chunk."""
    _check_engine(engine, block, "datum_stats")
    if chunk is not None and int(chunk) < 1:
        raise ValueError("chunk must be >= 1")
    x = _args.sample_rows(samples, engine.ndim, "datum_stats")
    w = _args.row_weights(weights, x, "datum_stats")
    acc = Accumulator(engine, block, thresholds, device=x.device)
    step = x.shape[0] if chunk is None else int(chunk)
    for s0 in range(0, x.shape[0], max(step, 1)):
        _launch(engine, x[s0:s0 + step], None if w is None else w[s0:s0 + step], block, acc, False)  # row slices stay contiguous
    return acc.result()


def report(engine, samples: torch.Tensor, weights: Optional[torch.Tensor] = None, block: str = "sn",
           thresholds: Sequence[float] = (2.0, 3.0)) -> dict:
    """Both kernels' outputs from one pass over the rows: dict(stats [S, ncol] and chi2_blocks [S, 10] on the device, columns,
    datum = the dict of ``datum_stats``)."""
    _check_engine(engine, block, "report")
    x = _args.sample_rows(samples, engine.ndim, "report")
    acc = Accumulator(engine, block, thresholds, device=x.device)
    stats, blocks = _launch(engine, x, _args.row_weights(weights, x, "report"), block, acc, True)
    return dict(stats=stats, chi2_blocks=blocks, columns=COLUMNS, datum=acc.result())


def center_of(samples: torch.Tensor, weights: Optional[torch.Tensor] = None, center: str = "median") -> np.ndarray:
    """The central row the scripts evaluate their report at, [ndim] numpy: "median" = ``np.percentile(samples, 50, axis=0)``
    (sn/pantheon.py:150; with weights ``corner.quantile(., 0.5, weights)`` per column, bao/desi_fs_lya.py:92-96), "mean" = the
    (weighted) mean (sn/pantheon_dipole_xyz.py:118)."""
    if center not in ("median", "mean"):
        raise ValueError('center must be "median" or "mean"')
    if center == "median":
        if weights is None:
            return np.asarray(_percentile(samples, 50.0).cpu().numpy(), dtype=np.float64)
        return np.asarray(_weighted_quantile(samples, weights, [0.5])[0], dtype=np.float64)
    if weights is None:
        return samples.mean(dim=0).cpu().numpy()
    return ((weights[:, None] * samples).sum(dim=0) / weights.sum()).cpu().numpy()


def summary(engine, samples: torch.Tensor, weights: Optional[torch.Tensor] = None, center: str = "median", block: str = "sn",
            n_data: Optional[int] = None, stats: Optional[torch.Tensor] = None) -> dict:
    """What the scripts print, with posterior widths: dict(center [ndim], at_center {column: value}, chi2 = chi^2 of the whole
    likelihood at the centre, n_data, dof = n_data - ndim, q = (15.9, 50, 84.1), posterior {column: [3]}) -- the percentiles of
    every per-sample statistic over the rows (``chain_stats.percentile``; with weights ``marginals._weighted_quantile``).
    n_data: the data the dof counts (default: those of the block).  stats: the [S, ncol] of ``sample_stats`` if already
    computed."""
    n = _check_engine(engine, block, "summary")
    x = _args.sample_rows(samples, engine.ndim, "summary")
    if x.shape[0] < 1:
        raise ValueError("summary needs at least one sample")
    w = _args.row_weights(weights, x, "summary")
    c = center_of(x, w, center)
    at, _ = sample_stats(engine, torch.from_numpy(np.ascontiguousarray(c[None, :])).to(x.device), block)
    at = at.cpu().numpy()[0]
    if stats is None:
        stats = sample_stats(engine, x, block)[0]
    cols = stats[:, :L.CF_RS_NCOL - 1]  # the index of the largest pull has no percentiles
    if w is None:
        post = _percentile(cols, list(SUMMARY_Q)).cpu().numpy()
    else:
        post = _weighted_quantile(cols, w, np.asarray(SUMMARY_Q) / 100.0)
    n_data = n if n_data is None else int(n_data)
    return dict(center=c, at_center=dict(zip(COLUMNS, at.tolist())), chi2=float(engine.chi_squared(c)), n_data=n_data,
                dof=dof(n_data, engine.ndim), q=np.asarray(SUMMARY_Q),
                posterior={name: post[:, j] for j, name in enumerate(COLUMNS[:-1])})


_REPORT_KEYS = ("weights", "block", "thresholds", "center", "n_data")


def chain_report(engine, samples: torch.Tensor, **kw) -> dict:
    """``report`` and ``summary`` of one chain from one pass over its rows: the dict of ``report`` plus ``summary``.  Keywords:
    weights, block, thresholds, center, n_data.  This is what ``ShardedEnsemble.fit_report`` and
    ``DeviceNestedSampler.fit_report`` return."""
    unknown = set(kw) - set(_REPORT_KEYS)
    if unknown:
        raise TypeError(f"fit_report got unexpected keyword(s) {sorted(unknown)}; valid: {list(_REPORT_KEYS)}")
    weights, block = kw.get("weights"), kw.get("block", "sn")
    out = report(engine, samples, weights=weights, block=block, thresholds=kw.get("thresholds", (2.0, 3.0)))
    out["summary"] = summary(engine, samples, weights=weights, center=kw.get("center", "median"), block=block,
                             n_data=kw.get("n_data"), stats=out["stats"])
    return out


def engine_of(log_prob_fn, engine=None, what: str = "fit_report"):
    """The engine behind a sampler's callable: the one given, or the one ``LikelihoodEngine.torch_log_prob`` attached."""
    engine = engine if engine is not None else getattr(log_prob_fn, "engine", None)
    if engine is None:
        raise ValueError(f"{what} needs the likelihood's engine: pass engine=, or sample with engine.torch_log_prob()")
    return engine
