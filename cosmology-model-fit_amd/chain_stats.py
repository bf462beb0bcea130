"""
Statistics of a chain held on the device: what the reference's scripts compute after ``sampler.run_mcmc``.

* ``integrated_time``: emcee 3's integrated autocorrelation time.  emcee normalises the autocorrelation of every
  (walker, dim) series (by FFT), averages it over the walkers, sums it into taus = 2 cumsum(f) - 1 and reads tau at its
  automatic window.  The window needs only a prefix of the lags, so the library sums the lags directly
  (csrc/cosmofit_chain.hip): the lag range grows (64, 128, 256, ... lags) until every dimension has its window, and each
  pass computes only the new lags.  Every sum runs in a fixed order, so tau is a deterministic function of the chain.
* ``gelman_rubin``: the arithmetic of the reference's ``gelman_rubin.py``, as torch reductions on the device.
* ``percentile``: a per-dimension sort on the device, then numpy's default ``linear`` method arithmetic (its virtual index
  and its ``_lerp``), so the result has ``np.percentile``'s bits.

The inputs are float64 tensors on an MI355X; there is no CPU fallback: CPU tensors raise.
"""
from __future__ import annotations

import warnings

import numpy as np
import torch

from . import _lib
from ._args import on_device, stream_of

_FIRST_LAGS = 64   # lags of the first pass; every further pass doubles the range ...
_MAX_PASS = 512    # ... by at most this many lags (the pass's lag sums are [lags, n_walkers * ndim] doubles)


class AutocorrError(Exception):
    """emcee's AutocorrError: the chain is too short for a reliable estimate; ``tau`` holds the estimate."""

    def __init__(self, tau, *args, **kwargs):
        self.tau = tau
        super().__init__(*args, **kwargs)


def _as_chain(x: torch.Tensor) -> torch.Tensor:
    """emcee's shapes: [n_t] -> [n_t, 1, 1], [n_t, n_w] -> [n_t, n_w, 1], [n_t, n_w, ndim] as is."""
    x = on_device(x, "integrated_time")
    if x.dim() == 1:
        x = x[:, None, None]
    elif x.dim() == 2:
        x = x[:, :, None]
    if x.dim() != 3 or min(x.shape) < 1:
        raise ValueError("invalid dimensions: the chain must be [n_t, n_walkers, ndim] (or [n_t, n_walkers], [n_t])")
    return x.contiguous()


def autocorr_window_search(x: torch.Tensor, c: float = 5.0):
    """(tau [ndim], window [ndim]) of emcee's ``integrated_time`` before its length check, both numpy.

    emcee's ``auto_window``: m = arange(n_t) < c taus; the window is argmin(m) if any(m), else n_t - 1.  So the window is
    the first lag that fails the test, and two corners follow emcee's code as it stands: a test that never fails gives
    argmin = 0 (tau = taus[0] = 1), and a dimension whose f is NaN (a walker that never moved) fails it everywhere, giving
    window n_t - 1 and tau NaN."""
    if not c > 0:
        raise ValueError("c must be > 0")
    x = _as_chain(x)
    n_t, n_w, ndim = x.shape
    n_s = n_w * ndim
    L = _lib
    lib = L.lib()
    with torch.cuda.device(x.device):
        stream = stream_of(x.device)
        mean = torch.empty(n_s, dtype=torch.float64, device=x.device)
        L.check(lib.cf_chain_mean(x.data_ptr(), n_t, n_s, mean.data_ptr(), stream))
        c0 = None
        f = np.empty((0, ndim))
        tau, window = np.full(ndim, np.nan), np.full(ndim, -1, dtype=np.int64)
        lag0 = 0
        while True:
            lag1 = min(n_t, lag0 + min(max(_FIRST_LAGS, lag0), _MAX_PASS))
            nlag = lag1 - lag0
            sums = torch.empty((nlag, n_s), dtype=torch.float64, device=x.device)
            L.check(lib.cf_chain_lagsum(x.data_ptr(), mean.data_ptr(), n_t, n_s, lag0, nlag, sums.data_ptr(), stream))
            if c0 is None:
                c0 = sums[0]  # lag 0: the normalisation of every series
            fd = torch.empty((nlag, ndim), dtype=torch.float64, device=x.device)
            L.check(lib.cf_chain_acf_mean(sums.data_ptr(), c0.data_ptr(), n_w, ndim, nlag, fd.data_ptr(), stream))
            f = np.concatenate([f, fd.cpu().numpy()])
            taus = 2.0 * np.cumsum(f, axis=0) - 1.0  # sequential prefix sums: the lags already seen keep their bits
            for d in np.flatnonzero(window < 0):
                m = np.arange(lag1) < c * taus[:, d]
                if not m[0]:  # NaN (c > 0 and taus[0] = 1 otherwise): any(m) is False over the whole chain
                    window[d], tau[d] = n_t - 1, np.nan
                elif not m.all():
                    window[d] = int(np.argmin(m))
                    tau[d] = taus[window[d], d]
            if (window >= 0).all() or lag1 == n_t:
                break
            lag0 = lag1
        for d in np.flatnonzero(window < 0):  # the test never failed: emcee's argmin of an all-True mask
            window[d], tau[d] = 0, taus[0, d]
    return tau, window


def integrated_time(x: torch.Tensor, c: float = 5, tol: float = 50, quiet: bool = False) -> np.ndarray:
    """emcee's ``integrated_time`` of a device chain [n_t, n_walkers, ndim]: tau per dimension (numpy, as emcee returns it).
    If tol * tau > n_t for any dimension, AutocorrError (with ``.tau``) is raised, or with ``quiet`` a warning is given
    and tau returned."""
    tau, _ = autocorr_window_search(x, c)
    n_t = _as_chain(x).shape[0]
    flag = tol * tau > n_t
    if np.any(flag):
        msg = ("The chain is shorter than {0} times the integrated autocorrelation time for {1} parameter(s). Use this "
               "estimate with caution and run a longer chain!\n").format(tol, np.sum(flag))
        msg += "N/{0} = {1:.0f};\ntau: {2}".format(tol, n_t / tol, tau)
        if not quiet:
            raise AutocorrError(tau, msg)
        warnings.warn(msg)
    return tau


def gelman_rubin(chains: torch.Tensor) -> torch.Tensor:
    """The reference's ``gelman_rubin(chains)`` on a device tensor (M, N, D): per-"chain" variances (ddof 1) along axis 1,
    W = their mean over axis 0, B = N var(means, ddof 1), sqrt(((N - 1) / N W + B / N) / W); [D] on the device."""
    chains = on_device(chains, "gelman_rubin")
    if chains.dim() != 3:
        raise ValueError("gelman_rubin takes a 3-d chain")
    M, N, D = chains.shape
    W = torch.var(chains, dim=1, correction=1).mean(dim=0)
    B = N * torch.var(chains.mean(dim=1), dim=0, correction=1)
    var_hat = ((N - 1) / N) * W + (1 / N) * B
    return torch.sqrt(var_hat / W)


def percentile(samples: torch.Tensor, q) -> torch.Tensor:
    """``np.percentile(samples, q, axis=0)`` (method 'linear') on a device tensor [n] or [n, ndim], same bits: the sort runs
    on the device; the virtual indices and weights are numpy's own scalar arithmetic; the interpolation is its ``_lerp``
    (a + (b - a) t, or b - (b - a)(1 - t) where t >= 0.5) as elementwise device operations.  Result [ndim] for a scalar q,
    [len(q), ndim] for a sequence (without the ndim axis for 1-d samples)."""
    a = on_device(samples, "percentile")
    if a.dim() not in (1, 2) or a.shape[0] < 1:
        raise ValueError("percentile takes non-empty samples [n] or [n, ndim]")
    qs = np.true_divide(np.asarray(q, dtype=np.float64), np.float64(100))
    if qs.ndim > 1:
        raise ValueError("q must be a scalar or a 1-d sequence")
    if np.isnan(qs).any() or not ((qs >= 0).all() and (qs <= 1).all()):
        raise ValueError("Percentiles must be in the range [0, 100]")
    n = a.shape[0]
    vi = np.atleast_1d((n - 1) * qs)                      # 'linear': get_virtual_index
    prev = np.floor(vi)
    nxt = prev + 1
    prev[vi >= n - 1], nxt[vi >= n - 1] = -1, -1           # _get_indexes: above the top -> the last element
    prev[vi < 0], nxt[vi < 0] = 0, 0
    prev, nxt = prev.astype(np.intp), nxt.astype(np.intp)
    gamma = np.asarray(vi - prev, dtype=vi.dtype)          # _get_gamma (from the adjusted previous index, as numpy)
    srt = torch.sort(a if a.dim() == 2 else a[:, None], dim=0).values  # NaN sorts last, as in numpy's partition
    dev = srt.device
    lo_v = srt[torch.as_tensor(prev % n, device=dev)]
    hi_v = srt[torch.as_tensor(nxt % n, device=dev)]
    t = torch.as_tensor(gamma, device=dev)[:, None]
    one_minus_t = torch.as_tensor(1 - gamma, device=dev)[:, None]
    diff = hi_v - lo_v                                     # _lerp
    res = torch.where(t >= 0.5, hi_v - diff * one_minus_t, lo_v + diff * t)
    res = torch.where(torch.isnan(srt[-1]), srt[-1], res)  # a slice holding a NaN gives NaN
    if a.dim() == 1:
        res = res[:, 0]
    return res[0] if qs.ndim == 0 else res
