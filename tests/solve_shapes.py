"""Shapes of the inverse-GEMM solve sweep (tests/test_solve_shapes_cpu.py, tests/test_gpu_solve_shapes.py,
tests/solve_forms_worker.py): factor sizes, batch sizes, CF_TUNE strings, the seeded SN data and the base walker rows.

The solve kernels (tri_gemm_chi2_kernel<NP,2>, tri_gemm_small_kernel<PF,FRAG,TPW>) take their launch-time form from the batch
size W, the factor's row blocks and a dozen CF_TUNE keys (csrc/cosmofit_api.hip: launch_tri_gemm*, launch_eval); cf_solve_form
reports it.  Everything here is plain numpy: importing this module needs neither the library nor a GPU."""
import importlib

import numpy as np

from oracle import oracle_np as onp

PKG_NAME = "cosmology-model-fit_amd"

# (N, n_rb, nt_last, why): row blocks of 64 rows, 16-row tiles of the last row block that hold rows of the factor
SIZES = (
    (1, 1, 1, "sn_parts larger than n_sn"),
    (17, 1, 2, "one row block, two tiles"),
    (64, 1, 4, "no padding at all"),
    (65, 2, 1, "one split level and one whole level"),
    (81, 2, 2, "two tiles in the last of several row blocks (17 has them in its only one)"),
    (177, 3, 4, "three row blocks, a full last one (177 -> 192 rows)"),
    (420, 7, 3, "exactly six split levels, equal to n_rb - 1"),
    (449, 8, 1, "six split levels and two whole; row blocks on both sides of 3"),
    (4097, 65, 1, "via_lds false (64 n_rb > 4096 shares); one row past 64 blocks"),
)
N_SMALL = tuple(n for n, *_ in SIZES if n <= 449)
N_LARGE = 4097
N_FIXED_MU = (177, 449)  # a second likelihood with fixed_mu on every seventh SN: the generic per-walker kernel, row-ordered residuals

# in-process batch sizes.  880: W mod 32 = 16, the last panel's second half is empty; 897: its first half holds one walker; 8193 and
# 12000 leave the last panel group partly empty (3 groups of 88 panels for 257, 3 of 128 for 375)
W_DEFAULT = (1, 16, 17, 64, 65, 96, 97, 160, 161, 512, 513, 864, 865, 880, 897, 1792, 1793, 4096, 8192, 8193, 12000)
W_LARGE = (1, 16, 97, 160, 161, 513, 897)  # for N = 4097
W_WORKER = (1, 16, 17, 97, 160, 161, 256, 257, 513, 880, 897, 1793, 2100)


def w_list(n):
    return W_LARGE if n == N_LARGE else W_DEFAULT


# one fresh process per string (CF_TUNE is read once per process)
TUNES = (
    "gemm_np=1,small_max=0",                              # 16-walker panels at every size, the throughput kernel on 1 walker
    "gemm_np=2,small_max=0,gemm_split=0",                 # 32-walker panels at every size, no half units
    "gemm_np=2,small_max=0,gemm_split=12,gemm_order=0",   # half units at every size, clipped to n_rb - 1, descending order
    "gemm_order=1,gemm_group=8",                          # snake order at every size, groups of 8 panels
    "small_max=256,small_tpw=1,small_frag=0,sn_parts=1",
    "small_max=256,small_tpw=2,sn_parts=4",
    "gemm_trim=0,gemm_diag_skip=0,small_lds_cap=0,sn_parts=2",
)

NAMES = ("offset", "H0", "Om", "v")
BOUNDS = np.array([(-19.6, -19.0), (60.0, 80.0), (0.15, 0.5), (-3.0, 3.0)])
Z_HI, N_GRID, Z_TURN = 1.5, 513, 0.15
Z_MAX = Z_HI + 0.1
ROW_OUTSIDE, ROW_FACE = 1, 2  # base rows: H0 = 95 (outside the box), v one ulp inside the box face


def sn_data(rng, n, z_hi):
    """Seeded SN block: sorted redshifts, a diagonal-plus-low-rank covariance and its Cholesky factor."""
    z = np.sort(rng.uniform(0.01, z_hi, n))
    zh = z * (1 + 1e-3 * rng.standard_normal(n))
    sig = rng.uniform(0.1, 0.3, n)
    A = 0.02 * rng.standard_normal((n, min(n, 12)))
    cov = np.diag(sig**2) + A @ A.T
    obs = 25 + 5 * np.log10((1 + zh) * 4283.0 * z * (1 + 0.4 * z)) - 19.3 + 0.15 * rng.standard_normal(n)
    return z, zh, obs, np.linalg.cholesky(cov)


_cache = {}


def data(n, fixed_mu=False):
    """dict(z_cmb, z_hel, obs, chol[, fixed_mu]) of factor size n, seeded by n (computed once per process)."""
    key = (n, bool(fixed_mu))
    if key not in _cache:
        z, zh, obs, chol = sn_data(np.random.default_rng(n), n, Z_HI)
        d = dict(z_cmb=z, z_hel=zh, obs=obs, chol=chol)
        if fixed_mu:  # calibrator-like rows: mu fixed near the datum's own distance modulus
            fm = np.full(n, np.nan)
            fm[::7] = obs[::7] + 19.3 + 0.05 * np.random.default_rng(10_000 + n).standard_normal(fm[::7].size)
            d["fixed_mu"] = fm
        _cache[key] = d
    return _cache[key]


def oracle_likelihood(n, fixed_mu=False):
    d = data(n, fixed_mu)
    return onp.Likelihood(ndim=4, z_max=Z_MAX, n_grid=N_GRID, bounds=BOUNDS, z_turn=Z_TURN,
                          **{name: onp.Slot(i) for i, name in enumerate(NAMES)}, **d)


def engine(pkg, n, fixed_mu=False):
    """SN-only flat LambdaCDM (offset, H0, Om, v; +-1 velocity step), inverse-GEMM solve."""
    d = data(n, fixed_mu)
    return pkg.LikelihoodEngine(ndim=4, z_max=Z_MAX, n_grid=N_GRID, bounds=BOUNDS,
                                params={name: pkg.Param(i) for i, name in enumerate(NAMES)},
                                sn=dict(z_turn=Z_TURN, step=None, **d), solve_mode=pkg.engine.solve_mode_of("inverse"))


def n_base(n):
    return 31 if n == N_LARGE else 251


def base_rows(n):
    """B distinct walker rows; row ROW_OUTSIDE lies outside the box, row ROW_FACE has v one ulp inside the box face."""
    synthetic = importlib.import_module(PKG_NAME + ".synthetic")
    base = synthetic.walkers(BOUNDS, n_base(n), seed=n)
    base[ROW_OUTSIDE, 1] = 95.0
    base[ROW_FACE, 3] = np.nextafter(BOUNDS[3, 1], 0.0)
    return base


def batch_rows(W, B):
    """Base row of walker i of a batch of W: (7 i) mod B.  7 is coprime to 251 and 31, so every base row recurs at many panel,
    half-unit and lane positions, and every output row of every batch has a reference value."""
    return (7 * np.arange(W)) % B


FORM_FIELDS = ("kernel", "panel_width", "tpw", "n_rb", "nt_last", "split_levels", "n_groups", "panels_per_group", "snake", "workgroups")


def default_form(n, W, *, small_max=160, np_forced=0, split=None, order=None, group=None, tpw=None, trim=True):
    """The solve form as DESIGN.md section 3.2 / 5 states the rules, written out independently of the library: what cf_solve_form
    must report without CF_TUNE (keywords: the CF_TUNE keys of the same meaning)."""
    n_pad = -(-n // 16) * 16
    n_rb = -(-(n_pad // 16) // 4)
    nt_last = min(4, max(1, (n_pad - 64 * (n_rb - 1)) // 16)) if trim else 4
    if W <= min(small_max, 256):
        t = tpw or (1 if W <= 96 else 2)
        panels = -(-W // 16)
        units = -(-(4 // t) * n_rb // 8) * 8
        return dict(zip(FORM_FIELDS, (0, 16, t, n_rb, nt_last, 0, 1, panels, 0, panels * units)))
    pw = {0: 32 if W > 512 else 16, 1: 16, 2: 32}[np_forced]
    panels = -(-W // pw)
    max_group = group if group is not None else (128 if panels > 256 else 0)
    ppg = panels
    if max_group > 0 and panels > max_group:
        g0 = -(-panels // max_group)
        ppg = -(-(-(-panels // g0)) // 8) * 8
    n_groups = -(-panels // ppg)
    levels = split if split is not None else (6 if 28 <= panels <= 56 else 0)
    levels = min(n_rb - 1, levels) if pw == 32 else 0
    wgs = n_groups * ppg * (n_rb + levels)
    snake = order if order is not None else int(wgs <= 1280)
    return dict(zip(FORM_FIELDS, (1, pw, 0, n_rb, nt_last, levels, n_groups, ppg, snake, wgs)))


# the keywords of default_form that each string of TUNES sets
TUNE_KW = (
    dict(np_forced=1, small_max=0),
    dict(np_forced=2, small_max=0, split=0),
    dict(np_forced=2, small_max=0, split=12, order=0),
    dict(order=1, group=8),
    dict(small_max=256, tpw=1),
    dict(small_max=256, tpw=2),
    dict(trim=False),
)


def check_forced(k, n, W, form):
    """Assert that the values string TUNES[k] forces hold in `form` (dict over FORM_FIELDS[, frag_order]) of (n, W)."""
    n_rb = form["n_rb"]
    ctx = f"CF_TUNE={TUNES[k]} N={n} W={W}: {form}"
    if k == 0:
        assert (form["kernel"], form["panel_width"], form["split_levels"]) == (1, 16, 0), ctx
    elif k == 1:
        assert (form["kernel"], form["panel_width"], form["split_levels"]) == (1, 32, 0), ctx
    elif k == 2:
        assert (form["kernel"], form["panel_width"], form["snake"]) == (1, 32, 0) and form["split_levels"] == min(n_rb - 1, 12), ctx
    elif k == 3:
        assert form["kernel"] == (0 if W <= 160 else 1), ctx
        if form["kernel"] == 1:
            panels = -(-W // form["panel_width"])
            assert form["snake"] == 1 and form["n_groups"] == -(-panels // 8) and (panels <= 8 or form["panels_per_group"] == 8), ctx
    elif k in (4, 5):
        assert form["kernel"] == (0 if W <= 256 else 1), ctx
        if W <= 256:
            assert form["tpw"] == (1 if k == 4 else 2), ctx
            assert form.get("frag_order", -1) in (-1, 0 if k == 4 else 1), ctx
    elif k == 6:
        assert form["nt_last"] == 4, ctx
    want = default_form(n, W, **TUNE_KW[k])
    assert {f: form[f] for f in FORM_FIELDS} == want, f"{ctx}\nexpected {want}"


def form_dict(row):
    """A worker's saved form row (int32 [11]) as a dict over FORM_FIELDS + frag_order."""
    return dict(zip(FORM_FIELDS + ("frag_order",), (int(v) for v in row)))


def run_workers(tunes, out_dir, mode="eval", timeout=600):
    """tests/solve_forms_worker.py once per CF_TUNE string, the processes side by side -> {string: dict of its arrays}."""
    import os
    import subprocess
    import sys

    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "solve_forms_worker.py")
    procs = []
    for k, tune in enumerate(tunes):
        out = os.path.join(str(out_dir), f"solve_{mode}_{k}.npz")
        p = subprocess.Popen([sys.executable, worker, out, mode], env=dict(os.environ, CF_TUNE=tune), stdout=subprocess.PIPE,
                             stderr=subprocess.STDOUT, text=True)
        procs.append((tune, out, p))
    results = {}
    try:
        for tune, out, p in procs:
            log, _ = p.communicate(timeout=timeout)
            assert p.returncode == 0, f"worker under CF_TUNE={tune!r} failed ({p.returncode}):\n{log}"
            results[tune] = dict(np.load(out))
    finally:
        for _, _, p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    return results


def position(i, panel_width):
    """(panel, half, lane column) of walker i in a batch solved in panels of `panel_width` walkers."""
    return i // panel_width, (i % panel_width) // 16, i % 16
