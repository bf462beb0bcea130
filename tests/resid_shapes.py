"""Shapes, engines and host-side helpers the fit-report tests share (tests/test_resid_cpu.py, tests/test_gpu_resid_kernels.py,
tests/test_gpu_resid.py)."""
import ctypes as C

import numpy as np

from conftest import golden, synthetic_cov

# SN sizes around the pitch of the residual rows (n_ld = n rounded up to 64) and its padding; one Pantheon+-sized engine
N_SN = (1, 2, 63, 64, 65, 257)
N_PANTHEON = 1590
ROWS = (1, 2, 255, 256, 257)
S_MAX = 257
CHUNKS = (32, 96, S_MAX)       # rows per chunk of the library's loop (test-only: cf_resid_set_chunk)
THRESHOLDS = (0.5, 1.0, 2.0)
REL, ABS = 1e-10, 1e-10        # the project's parity bar; absolute for the columns that cross zero
FIXTURE_CASES = ("sn_pantheon", "sn_pantheon_and_sh0es", "sn_union3_1", "bao_desi_fs_lya")
# fixture column -> column of the report (norm.fit's pair is mean and std)
FIXTURE_COLUMNS = dict(ss_res="ss_res", ss_tot="ss_tot", r2="r2", rmsd="rmsd", skew="skew", kurtosis="kurtosis",
                       fit_mean="mean", fit_std="std")


def sn_likelihood(pkg, n, seed=5):
    syn = pkg.synthetic.pantheon_like(n_sn=n, seed=seed, rank=min(40, n))
    return pkg.sn_pantheon.PantheonLikelihood(syn["z_cmb"], syn["z_hel"], syn["obs"], chol=syn["chol"]), syn


def sn_thetas(pkg, S=S_MAX, seed=9):
    """Rows of sn/pantheon.py's box, narrowed to where the residuals are of the size of the errors."""
    box = np.array([(-19.6, -19.1), (60.0, 80.0), (0.15, 0.5), (-2.0, 2.0)])
    return pkg.synthetic.walkers(box, S, seed=seed)


def bao_likelihood(pkg):
    g = golden("bao_desi_fs_lya")
    return pkg.scripts.build("bao/desi_fs_lya.py", bao=(g["bao_z"], g["bao_val"], g["bao_qty"], g["bao_inv_cov"])), g


def bao_thetas(pkg, S=S_MAX, seed=10):
    return pkg.synthetic.walkers(np.array([(0.5, 0.8), (0.1, 0.8), (-1.0, 0.0)]), S, seed=seed)


def fixture_likelihood(pkg, case):
    """(mirror, block) of one of the four scripts of tests/golden/residuals.npz, from the script's own data fixture."""
    if case == "sn_pantheon":
        g = golden("sn_pantheon")
        return pkg.sn_pantheon.PantheonLikelihood(g["z_cmb"], g["z_hel"], g["obs"], synthetic_cov(g["sigma"])), "sn"
    if case == "sn_pantheon_and_sh0es":
        g = golden("sn_pantheon_and_sh0es")
        return pkg.sn_pantheon.PantheonLikelihood(g["z_cmb"], g["z_hel"], g["obs"], synthetic_cov(g["sigma"]), step=g["corr_sign"],
                                                  fixed_mu=np.where(g["ceph"] != -9, g["ceph"], np.nan), bounds=g["bounds"],
                                                  h0_prior=None), "sn"
    if case == "sn_union3_1":
        g = golden("sn_union3_1")
        return pkg.likelihoods.SnUnion3(g["z_cmb"], g["z_hel"], g["obs"], g["cov"], H0=float(g["H0"])), "sn"
    return bao_likelihood(pkg)[0], "bao"


def parts_rows(engine, theta, block, data):
    """(residual rows [S, n], y rows [S, n]) from ``engine.parts`` -- the accessor path the report reduces.  data: the block's
    observed values (obs for "sn", val for "bao")."""
    p = engine.parts(theta)
    data = np.asarray(data, dtype=np.float64)
    if block == "sn":
        return p["delta"], data[None, :] - p["mu_corr"]
    return data[None, :] - p["bao_theory"], np.broadcast_to(data, p["bao_theory"].shape)


def fixture_data(case):
    """The observed values of the block the fixture's statistics are of."""
    return golden(case)["bao_val" if case == "bao_desi_fs_lya" else "obs"]


def host_acc(L, n, n_thr):
    """A zeroed cf_resid_acc over host arrays: (struct, dict of the arrays)."""
    arrs = dict(w_sum=np.zeros(n), mean=np.zeros(n), m2=np.zeros(n), exceed=np.zeros((max(n_thr, 1), n)),
                n_used=np.zeros(n, dtype=np.int64), n_skipped=np.zeros(n, dtype=np.int64))
    a = L.cf_resid_acc()
    a.struct_size, a.n, a.n_thr = C.sizeof(L.cf_resid_acc), n, n_thr
    for k, v in arrs.items():
        setattr(a, k, v.ctypes.data)
    return a, arrs
