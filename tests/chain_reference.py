"""Host (numpy) restatements that the chain-statistics tests compare the device against.

* ``integrated_time``: emcee 3's ``autocorr.integrated_time`` (FFT autocorrelation per walker, walker average in ascending
  order, taus = 2 cumsum(f) - 1, ``auto_window``), restated because emcee is not installed; it also returns the windows.
* ``gelman_rubin``: the arithmetic of the reference's ``gelman_rubin.py`` (checked against its recorded output in
  tests/golden/gelman_rubin.npz).
* the seeded inputs: AR(1) chains with a known autocorrelation time and the Gelman-Rubin fixture's input.
"""
import numpy as np


def _next_pow_two(n):
    i = 1
    while i < n:
        i = i << 1
    return i


def _acf_block(x):
    """Normalised autocorrelation of every column of x [n_t, k] (emcee's function_1d, one FFT per column)."""
    n_t = x.shape[0]
    n = _next_pow_two(n_t)
    f = np.fft.fft(x - np.mean(x, axis=0), n=2 * n, axis=0)
    acf = np.fft.ifft(f * np.conjugate(f), axis=0)[:n_t].real
    return acf / acf[0]


def auto_window(taus, c):
    m = np.arange(len(taus)) < c * taus
    if np.any(m):
        return int(np.argmin(m))
    return len(taus) - 1


def integrated_time(x, c=5, tol=50, chunk=256):
    """(tau [ndim], window [ndim], taus [n_t, ndim], too_short) of emcee's integrated_time on x [n_t, n_w, ndim]."""
    x = np.asarray(x, dtype=np.float64)
    n_t, n_w, n_d = x.shape
    tau, window = np.empty(n_d), np.empty(n_d, dtype=np.int64)
    all_taus = np.empty((n_t, n_d))
    for d in range(n_d):
        f = np.zeros(n_t)
        for k0 in range(0, n_w, chunk):
            acf = _acf_block(x[:, k0:k0 + chunk, d])
            with np.errstate(invalid="ignore"):
                for k in range(acf.shape[1]):
                    f += acf[:, k]
        f /= n_w
        taus = 2.0 * np.cumsum(f) - 1.0
        window[d] = auto_window(taus, c)
        tau[d] = taus[window[d]]
        all_taus[:, d] = taus
    return tau, window, all_taus, bool(np.any(tol * tau > n_t))


def window_margin(taus, window, c=5):
    """Smallest relative distance |i - c taus[i]| / (c |taus[i]|) over the lags up to each window: how far the fixture
    sits from a window boundary (a difference in the last bits of tau cannot move a window farther than this)."""
    out = np.inf
    for d in range(taus.shape[1]):
        i = np.arange(window[d] + 1)
        ct = c * taus[: window[d] + 1, d]
        out = min(out, float(np.min(np.abs(i - ct) / np.abs(ct))))
    return out


def ar1_chain(n_t, n_w, ndim, rho, seed):
    """x_t = rho x_{t-1} + sqrt(1 - rho^2) e_t per series, stationary start: tau = (1 + rho) / (1 - rho)."""
    rng = np.random.default_rng(seed)
    x = np.empty((n_t, n_w, ndim))
    x[0] = rng.standard_normal((n_w, ndim))
    s = np.sqrt(1.0 - rho * rho)
    for t in range(1, n_t):
        x[t] = rho * x[t - 1] + s * rng.standard_normal((n_w, ndim))
    return x


def gelman_rubin(chains):
    """The reference's gelman_rubin.py arithmetic on (M, N, D)."""
    M, N, D = chains.shape
    W = np.mean(np.var(chains, axis=1, ddof=1), axis=0)
    B = N * np.var(np.mean(chains, axis=1), axis=0, ddof=1)
    var_hat = ((N - 1) / N) * W + (1 / N) * B
    return np.sqrt(var_hat / W)


def gelman_rubin_input(seed, shape):
    """The fixture's input, regenerated from its seed: unit normals plus a per-row offset (axis 0 = the "chains"), so that
    R-hat is away from 1."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape)
    return x + 0.2 * rng.standard_normal((shape[0], 1, shape[2]))
