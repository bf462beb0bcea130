"""Shapes, covariances and host-side helpers the attribution tests share (tests/test_infl_cpu.py,
tests/test_gpu_infl_kernels.py, tests/test_gpu_infl.py)."""
import ctypes as C

import numpy as np

import infl_reference as IR
import resid_shapes as RS
from conftest import synthetic_cov

# cf_prec_apply_device: n around the k step of 4, the 16-wide tile, the 64-wide block; S around a row tile and a row block
N_APPLY = (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 257)
S_APPLY = (1, 2, 15, 16, 17, 255, 256, 257)
S_MAX = 257
N_HARD = 257                   # hard_cov here, synthetic_cov below
N_SN = RS.N_SN                 # the SN engines of cf_infl_device
N_PANTHEON, S_PANTHEON = RS.N_PANTHEON, 33
CHUNKS = RS.CHUNKS
THRESHOLDS = (0.5, 1.0, 2.0)


def covariance(pkg, n, seed=0):
    """The covariance of the kernel tests: ``synthetic.hard_cov`` at n = 257, the fixtures' ``synthetic_cov`` below."""
    rng = np.random.default_rng(700 + n)
    sigma = rng.uniform(0.1, 0.3, n)
    if n >= N_HARD:
        z = np.sort(np.exp(rng.uniform(np.log(0.01), np.log(2.26), n)))
        return pkg.synthetic.hard_cov(z, sigma, seed=seed)
    return synthetic_cov(sigma, seed=seed, rank=min(40, n))


def residual_rows(L, S, seed=1):
    """S rows drawn from the covariance L L^T (so that chi^2 ~ n), a few of them scaled up and one all zero."""
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((S, L.shape[0])) @ np.tril(L).T
    rows[::7] *= 3.0
    if S > 2:
        rows[2] = 0.0
    return np.ascontiguousarray(rows)


def host_precision(L_mod, lib, chol):
    """(K [n, n], diag K [n]) of cf_selftest_prec_host: the host half of cf_prec_create, no device."""
    chol = np.ascontiguousarray(chol, dtype=np.float64)
    n = chol.shape[0]
    K, kd = np.empty((n, n)), np.empty(n)
    L_mod.check(lib.cf_selftest_prec_host(chol.ctypes.data, n, n, K.ctypes.data, kd.ctypes.data))
    return K, kd


def host_out(L_mod, S, n, want=("g", "contrib", "z", "loo", "sample")):
    """A cf_infl_out over host arrays: (struct, dict of the arrays)."""
    arrs = {k: np.full((S, L_mod.CF_INFL_NCOL if k == "sample" else n), np.nan) for k in want}
    o = L_mod.cf_infl_out()
    o.struct_size = C.sizeof(L_mod.cf_infl_out)
    for k, v in arrs.items():
        setattr(o, k, v.ctypes.data)
    return o, arrs


def restate(case_rows, g_ref, kdiag):
    """dict of the restatement's row arrays and sample table for residual rows and their g."""
    contrib, z, loo, drop = IR.row_arrays(case_rows, g_ref, kdiag)
    return dict(g=g_ref, contrib=contrib, z=z, loo=loo, drop=drop, sample=IR.sample_table(case_rows, g_ref, kdiag))
