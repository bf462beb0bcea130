"""
Model-independent reconstruction of H(z) from the cosmic chronometers with an exact Gaussian process on the device.

The reference fits a constant mean and a scaled RBF kernel to the 38 CC points, with the full CC covariance as fixed noise
times one learned ``noise_scale`` (ohd/cc_gp.py:14-41, ohd/gp_lib.py:55-68), by 5000 serial Adam steps, and reads off
H0 = H(0) +- sigma, the band of H(z) and q(z) = -1 + (1 + z) H'(z) / H(z) (cc_gp.py:75-92).  Here the quantity that loop climbs,
the log marginal likelihood, is a batched ``theta [W, 4] -> [W]`` kernel (csrc/cosmofit_gp.hip), so that

* the type-II maximum is one ``optimize.best_fit`` call (``HubbleGP.fit``),
* the hyperparameter posterior comes from ``ensemble.ShardedEnsemble`` on ``HubbleGP.torch_log_prob()``, and the bands of
  H(z), H0 and q(z) marginalised over it from ``HubbleGP.marginal_predict`` (the reference has no counterpart),
* the evidence of the GP comes from ``nested.DeviceNestedSampler`` on the same callable.

theta = (m, s_f^2, l, s): constant mean, output scale, length scale, noise scale, in natural form and in the units of the
normalised data (``y = (H - mean H) / std H``, ``C = cov / std^2``, cc_gp.py:16-21); ``physical`` converts.  A box replaces
gpytorch's constraints; its default is m (-2, 2), s_f^2 (0.05, 20), l (max z, 3 max z) (the reference's ``Interval``,
cc_gp.py:28) and s (0.05, 4).

There is no tensor fallback: without an MI355X the object can be built and asked for its normalisation, every evaluation
raises.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import numpy as np

from . import _lib as L
from ._args import ptr, stream_of

NDIM = L.CF_GP_NDIM
NAMES = ("mean", "output_scale", "length_scale", "noise_scale")
QUANTITIES = ("mean", "var", "dmean", "dvar", "cov_fd")  # the five columns of cf_gp_predict_device


def default_bounds(z_max: float) -> np.ndarray:
    """The default box in normalised units for data whose largest redshift is z_max."""
    if not (np.isfinite(z_max) and z_max > 0):
        raise ValueError("the default box needs max z > 0 (length scale in (max z, 3 max z)); pass bounds=")
    return np.array([[-2.0, 2.0], [0.05, 20.0], [z_max, 3.0 * z_max], [0.05, 4.0]])



def _z_star(z_star) -> np.ndarray:
    z = np.atleast_1d(np.asarray(z_star, dtype=np.float64))
    if z.ndim != 1 or not 1 <= z.size <= L.CF_GP_MAX_NZ:
        raise ValueError(f"z_star must be a 1-d sequence of 1..{L.CF_GP_MAX_NZ} redshifts")
    return np.ascontiguousarray(z)


def _noise(noise) -> float:
    noise = float(noise)
    if not (math.isfinite(noise) and noise >= 0.0):
        raise ValueError("noise must be finite and >= 0")
    return noise


class HubbleGP:
    """Exact GP on (z, H, cov).  normalise=True standardises H as the script does (by 1 when std H == 0, i.e. n = 1)."""

    def __init__(self, z, H, cov, bounds=None, normalise: bool = True, device: int = 0):
        z = np.ascontiguousarray(np.asarray(z, dtype=np.float64).reshape(-1))
        H = np.ascontiguousarray(np.asarray(H, dtype=np.float64).reshape(-1))
        cov = np.asarray(cov, dtype=np.float64)
        n = z.size
        if H.size != n or cov.shape != (n, n):
            raise ValueError(f"shapes disagree: z [{n}], H [{H.size}], cov {cov.shape}")
        self.n, self.device = n, int(device)
        self.h_mean = float(np.mean(H)) if (normalise and n) else 0.0
        std = float(np.std(H)) if (normalise and n) else 1.0
        self.h_std = std if (np.isfinite(std) and std > 0.0) else 1.0
        self.z = z
        self.y = np.ascontiguousarray((H - self.h_mean) / self.h_std)
        self.cov = np.ascontiguousarray(cov / self.h_std**2)
        self.bounds = np.ascontiguousarray(default_bounds(float(np.max(z)) if n else math.nan) if bounds is None
                                           else np.asarray(bounds, dtype=np.float64))
        if self.bounds.shape != (NDIM, 2):
            raise ValueError(f"bounds must be [{NDIM}, 2]: (lo, hi) of {NAMES}")
        self.log_norm = n * math.log(self.h_std)  # log ML of H = log ML of y - n log std H (cc_gp.py:60)
        self._h = None
        self._no_device: Optional[L.CosmofitError] = None
        d = L.cf_gp_desc()
        d.struct_size, d.device, d.n = C.sizeof(L.cf_gp_desc), self.device, n
        d.z, d.y, d.cov, d.bounds = (a.ctypes.data for a in (self.z, self.y, self.cov, self.bounds))
        h = C.c_void_p()
        try:
            L.check(L.lib().cf_gp_create(C.byref(d), C.byref(h)))
            self._h = h
        except L.CosmofitError as e:
            if e.code != -2:  # argument errors are raised here; a missing GPU when something is evaluated
                raise
            self._no_device = e

    # ---- life cycle ----
    def close(self):
        if getattr(self, "_h", None) is not None:
            L.lib().cf_gp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _handle(self, what: str):
        if self._h is None:
            if self._no_device is not None:
                raise L.CosmofitError(-2, f"HubbleGP.{what} runs in the library's HIP kernels: {self._no_device} (there is no "
                                          "tensor fallback)")
            raise L.CosmofitError(-1, f"HubbleGP.{what}: this GP has been closed")
        return self._h

    def info(self) -> dict:
        i = L.cf_gp_info()
        L.check(L.lib().cf_gp_get_info(self._handle("info"), C.byref(i)))
        return dict(n=i.n, device=i.device, ld=i.ld, lds_bytes=i.lds_bytes, failed_factorizations=i.failed_factorizations)

    # ---- units ----
    def physical(self, theta) -> np.ndarray:
        """(mean, output scale, length scale, noise scale) in the data's units: km/s/Mpc, (km/s/Mpc)^2, redshift, 1."""
        th = np.asarray(theta, dtype=np.float64)
        if th.shape[-1] != NDIM:
            raise ValueError(f"theta must end in {NDIM} columns")
        out = th.copy()
        out[..., 0] = th[..., 0] * self.h_std + self.h_mean
        out[..., 1] = th[..., 1] * self.h_std**2
        return out

    def normalised(self, phys) -> np.ndarray:
        """The inverse of ``physical``."""
        ph = np.asarray(phys, dtype=np.float64)
        if ph.shape[-1] != NDIM:
            raise ValueError(f"theta must end in {NDIM} columns")
        out = ph.copy()
        out[..., 0] = (ph[..., 0] - self.h_mean) / self.h_std
        out[..., 1] = ph[..., 1] / self.h_std**2
        return out

    def _rows(self, theta) -> np.ndarray:
        th = np.ascontiguousarray(np.atleast_2d(np.asarray(theta, dtype=np.float64)))
        if th.ndim != 2 or th.shape[1] != NDIM:
            raise ValueError(f"theta must be [{NDIM}] or [W, {NDIM}]")
        return th

    # ---- host-buffer evaluations (cf_gp_mll / cf_gp_predict) ----
    def parts(self, theta) -> dict:
        """log_ml (normalised units), quad = r^T K^-1 r and logdet = log|K| of the rows of theta."""
        th = self._rows(theta)
        out, parts = np.empty(th.shape[0]), np.empty((th.shape[0], 2))
        L.check(L.lib().cf_gp_mll(self._handle("parts"), ptr(th), th.shape[0], ptr(out), ptr(parts)))
        return dict(log_ml=out, quad=parts[:, 0], logdet=parts[:, 1])

    def log_marginal_likelihood(self, theta):
        """log p(H | theta) in physical units (the normalised value - n log std H): float for theta [4], numpy [W] for
        [W, 4]; -inf outside the box."""
        th = self._rows(theta)
        out = np.empty(th.shape[0])
        L.check(L.lib().cf_gp_mll(self._handle("log_marginal_likelihood"), ptr(th), th.shape[0], ptr(out), None))
        out = out - self.log_norm
        return float(out[0]) if np.ndim(theta) == 1 else out

    def predict_normalised(self, theta, z_star, noise: float = 0.0) -> np.ndarray:
        """[S, nz, 5] = (mean, var, dmean, dvar, cov_fd) of the normalised process: the kernel's own output."""
        th, zs = self._rows(theta), _z_star(z_star)
        out = np.empty((th.shape[0], zs.size, 5))
        L.check(L.lib().cf_gp_predict(self._handle("predict"), ptr(th), th.shape[0], ptr(zs), zs.size, _noise(noise), ptr(out)))
        return out

    def _to_physical(self, zs, mean, var, dmean, dvar, cov, xp=np) -> dict:
        s = self.h_std
        H = mean * s + self.h_mean
        dH = dmean * s
        return dict(z=zs, mean=H, std=xp.sqrt(xp.maximum(var, 0.0)) * s, dmean=dH, dstd=xp.sqrt(xp.maximum(dvar, 0.0)) * s,
                    cov_fd=cov * s**2, q=-1.0 + (1.0 + zs) * (dH / H))  # cc_gp.py:92

    def predict(self, theta, z_star, noise: float = 0.0) -> dict:
        """H(z*) of one hyperparameter row or of S rows: dict of z [nz] and mean, std, dmean, dstd, cov_fd, q ([nz] for
        theta [4], [S, nz] for [S, 4]) in km/s/Mpc; q from the means (cc_gp.py:92).  noise: the reference's ``test_noise``, a
        variance in normalised units that enters as s * noise (gp_lib.py:62-63)."""
        out = self.predict_normalised(theta, z_star, noise)
        if np.ndim(theta) == 1:
            out = out[0]
        return self._to_physical(_z_star(z_star), *(out[..., k] for k in range(5)))

    # ---- device evaluations ----
    def _check_device_rows(self, x, name: str):
        import torch

        if not isinstance(x, torch.Tensor) or not x.is_cuda or x.device.index != self.device or x.dtype != torch.float64 or \
                not x.is_contiguous() or x.dim() != 2 or x.shape[1] != NDIM:
            raise ValueError(f"{name} must be a contiguous float64 tensor [W, {NDIM}] on the GP's GPU (cuda:{self.device})")

    def torch_log_prob(self):
        """Callable ``f(theta: cuda float64 tensor [W, 4]) -> tensor [W]``: log ML (physical units) inside the box, -inf
        outside, asynchronous on torch's current stream.  Plugs into ``ensemble.ShardedEnsemble``, ``optimize.best_fit`` /
        ``profile`` and ``nested.DeviceNestedSampler`` (with a ``Prior`` over the same box)."""
        import torch

        self._handle("torch_log_prob")  # no GPU, or closed: say so now, not at the first step of a sampler
        lib = L.lib()

        def f(theta):
            # through self on every call: the callable keeps the GP (and its device buffers) alive for as long as a sampler
            # holds it, and a GP closed meanwhile raises here instead of launching on a freed handle
            h = self._handle("torch_log_prob")
            self._check_device_rows(theta, "theta")
            out = torch.empty(theta.shape[0], dtype=torch.float64, device=theta.device)
            if theta.shape[0]:
                L.check(lib.cf_gp_mll_device(h, theta.data_ptr(), theta.shape[0], out.data_ptr(), None,
                                             stream_of(theta.device)))
                out -= self.log_norm
            return out

        return f

    def fit(self, n_starts: int = 32, seed: int = 0, **options):
        """The type-II maximum in the box (the end point of the reference's 5000 Adam steps): ``optimize.best_fit`` on
        ``torch_log_prob``; returns its ``FitResult`` (x in normalised units, log_prob in physical units)."""
        import torch

        from . import optimize

        f = self.torch_log_prob()
        with torch.cuda.device(self.device):
            return optimize.best_fit(f, self.bounds, n_starts=n_starts, seed=seed, **options)

    def _predict_rows(self, x, zd, noise: float):
        """[m, nz, 5] on the device of x (cf_gp_predict_device on torch's current stream)."""
        import torch

        h = self._handle("marginal_predict")
        self._check_device_rows(x, "samples")
        out = torch.empty((x.shape[0], zd.shape[0], 5), dtype=torch.float64, device=x.device)
        with torch.cuda.device(x.device):
            L.check(L.lib().cf_gp_predict_device(h, x.data_ptr(), x.shape[0], zd.data_ptr(), zd.shape[0], noise, out.data_ptr(),
                                                 stream_of(x.device)))
        return out

    def marginal_predict(self, samples, z_star, weights=None, noise: float = 0.0, max_bytes: int = 2**28) -> dict:
        """The predictive moments marginalised over hyperparameter samples [S, 4] (a flat device chain, or the nested
        posterior with its weights): the mixture of the S Gaussians,

            mean = E[mean_s],  var = E[var_s + mean_s^2] - mean^2,  cov_fd = E[cov_s + mean_s dmean_s] - mean dmean,

        and the same for the derivative.  Returns what ``predict`` returns (numpy, km/s/Mpc, q from the mixture means) plus
        H0 = (mean, std) at the first z* == 0 (None without one).  The rows are evaluated in chunks whose output stays under
        max_bytes."""
        import torch

        zs, noise = _z_star(z_star), _noise(noise)
        if not isinstance(samples, torch.Tensor) or samples.dtype != torch.float64 or samples.dim() != 2 or \
                samples.shape[1] != NDIM or samples.shape[0] < 1:
            raise ValueError(f"marginal_predict takes a float64 tensor of samples [S, {NDIM}] with S >= 1")
        if max_bytes < 1:
            raise ValueError("max_bytes must be >= 1")
        x = samples.contiguous()
        S, nz = x.shape[0], zs.size
        if weights is None:
            w = torch.full((S,), 1.0 / S, dtype=torch.float64, device=x.device)
        else:
            w = torch.as_tensor(weights, dtype=torch.float64).to(x.device).reshape(-1)
            if w.shape[0] != S or not bool(torch.isfinite(w).all()) or bool((w < 0).any()) or not float(w.sum()) > 0:
                raise ValueError("weights must be [S], finite, >= 0, with a positive sum")
            w = w / w.sum()
        zd = torch.from_numpy(zs).to(x.device)
        chunk = marginal_chunk(S, nz, int(max_bytes))
        acc = torch.zeros((5, nz), dtype=torch.float64, device=x.device)
        for s0 in range(0, S, chunk):
            p = self._predict_rows(x[s0:s0 + chunk], zd, noise)  # [m, nz, 5]
            ww = w[s0:s0 + chunk, None]
            mean, var, dmean, dvar, cov = (p[:, :, k] for k in range(5))
            acc[0] += (ww * mean).sum(0)
            acc[1] += (ww * (var + mean * mean)).sum(0)
            acc[2] += (ww * dmean).sum(0)
            acc[3] += (ww * (dvar + dmean * dmean)).sum(0)
            acc[4] += (ww * (cov + mean * dmean)).sum(0)
            del p
        a = acc.cpu().numpy()
        out = self._to_physical(zs, a[0], a[1] - a[0] ** 2, a[2], a[3] - a[2] ** 2, a[4] - a[0] * a[2])
        at0 = np.nonzero(zs == 0.0)[0]
        out["H0"] = (float(out["mean"][at0[0]]), float(out["std"][at0[0]])) if at0.size else None
        return out


def marginal_chunk(S: int, nz: int, max_bytes: int) -> int:
    """Rows per chunk of ``marginal_predict``: the most whose [rows, nz, 5] output stays under max_bytes, at least 1."""
    if max_bytes < 1:
        raise ValueError("max_bytes must be >= 1")
    return int(max(1, min(S, max_bytes // (5 * 8 * max(nz, 1)))))
