"""
Shape tables and seeded inputs of the Gaussian-process tests (tests/test_gp_cpu.py, tests/test_gpu_gp_kernels.py,
tests/test_gpu_gp.py).  The long-double references are computed once per data size and shared (``reference``).

Data: n = 38 is the real cosmic-chronometer set (tests/golden/ohd_cc.npz, normalised as ohd/cc_gp.py:16-21); the other sizes
are synthetic: z sorted uniform on (0.05, 2), H_t = 70 sqrt(0.3 (1 + z)^3 + 0.7), sigma = H_t U(0.05, 0.2),
H = H_t + sigma N(0, 1), C = diag(sigma^2) + f f^T with f = 0.03 H_t, the default box with max z = 2.
"""
import functools

import numpy as np

import gp_reference as R
from conftest import golden

N_SET = (1, 2, 17, 38, 63, 64)   # 38: the real data; 63 / 64: the last lane and a full wave
ROWS_SET = (1, 63, 64, 65, 257, 4097)
NZ_SET = (1, 63, 64, 65, 130)
N_BASE = 65                      # distinct hyperparameter rows per size; larger batches repeat them at other positions
NZ_FULL = max(NZ_SET)
TEST_NOISE = 1e-4                # ohd/cc_gp.py:76


def default_bounds(z_max):
    return np.array([[-2.0, 2.0], [0.05, 20.0], [z_max, 3.0 * z_max], [0.05, 4.0]])


@functools.lru_cache(maxsize=None)
def data(n):
    """(z, y, C, bounds, h_mean, h_std): normalised data and the default box."""
    if n == 38:
        g = golden("ohd_cc")
        z, H, cov = (np.asarray(g[k], dtype=np.float64) for k in ("cc_z", "cc_h", "cc_cov"))
        z_max = float(z.max())
    else:
        rng = np.random.default_rng(7100 + n)
        z = np.sort(rng.uniform(0.05, 2.0, n))
        Ht = 70.0 * np.sqrt(0.3 * (1 + z) ** 3 + 0.7)
        sigma = Ht * rng.uniform(0.05, 0.2, n)
        H = Ht + sigma * rng.standard_normal(n)
        f = 0.03 * Ht
        cov = np.diag(sigma**2) + np.outer(f, f)
        z_max = 2.0
    mean, std = float(np.mean(H)), float(np.std(H))
    std = std if std > 0 else 1.0
    return z, (H - mean) / std, cov / std**2, default_bounds(z_max), mean, std


def raw_data(n):
    """(z, H, cov) in km/s/Mpc: what ``HubbleGP`` takes."""
    z, y, C, _, mean, std = data(n)
    return z, y * std + mean, C * std**2


@functools.lru_cache(maxsize=None)
def base_thetas(n):
    """N_BASE rows uniform strictly inside the box of size n."""
    b = data(n)[3]
    u = np.random.default_rng(4200 + n).uniform(0.02, 0.98, (N_BASE, 4))
    return np.ascontiguousarray(b[:, 0] + u * (b[:, 1] - b[:, 0]))


def row_index(rows):
    """Which base row sits at each position of a batch of `rows`: the first N_BASE in order, then a stride that puts every
    base row at many positions."""
    k = np.arange(rows)
    return np.where(k < N_BASE, k, (7 * k + 3) % N_BASE) if rows > N_BASE else k


def thetas(n, rows):
    return np.ascontiguousarray(base_thetas(n)[row_index(rows)])


@functools.lru_cache(maxsize=None)
def z_star_full(n):
    """NZ_FULL test redshifts; every prefix of NZ_SET's lengths is a test set.  The first is 0 (H0); then a training redshift
    exactly, a point below the data, one above, the last training redshift, further training redshifts, and a grid from
    -0.2 to max z + 0.5."""
    z = data(n)[0]
    special = [0.0, float(z[0]), -0.1, float(z.max()) + 0.3, float(z[-1])] + [float(v) for v in z[1:: max(1, len(z) // 8)][:8]]
    grid = np.linspace(-0.2, float(z.max()) + 0.5, NZ_FULL - len(special))
    return np.ascontiguousarray(np.concatenate([special, grid]))


def z_star(n, nz):
    return np.ascontiguousarray(z_star_full(n)[:nz])


@functools.lru_cache(maxsize=None)
def reference(n):
    """Long double, once per size: mll [N_BASE, 3] = (log ML, quad, logdet) and pred [N_BASE, NZ_FULL, 5] at TEST_NOISE."""
    z, y, C = data(n)[:3]
    th = base_thetas(n)
    mll = np.array([R.mll_parts(z, y, C, t) for t in th], dtype=R.LD)
    pred = np.array([R.predict(z, y, C, t, z_star_full(n), TEST_NOISE) for t in th], dtype=R.LD)
    return mll, pred


def bad_rows(n):
    """Rows that must not be evaluated: one coordinate outside the box on either side, NaN, +inf, -inf."""
    b = data(n)[3]
    good = base_thetas(n)[0]
    rows = []
    for k in range(4):
        for v in (b[k, 0] - 0.01, b[k, 1] + 0.01, b[k, 0], b[k, 1], np.nan, np.inf, -np.inf):
            t = good.copy()
            t[k] = v
            rows.append(t)
    return np.array(rows)
