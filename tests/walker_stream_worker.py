"""Every case of tests/test_gpu_walker_stream.py under whatever CF_TUNE the process was started with:
    python tests/walker_stream_worker.py <0|1|auto> <out.npz>
0 / 1: CF_TUNE walker_stream=0 / 1 is set; each likelihood must report that form (cf_walker_form) for the batch it is given.
auto: the automatic switch; only the batch-invariance case runs.  The arrays go to <out.npz> as float64, compared as bits by
the test."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
amd = importlib.import_module("cosmology-model-fit_amd")
eng_mod = importlib.import_module("cosmology-model-fit_amd.engine")
Param, LikelihoodEngine, C_KM_S = eng_mod.Param, eng_mod.LikelihoodEngine, eng_mod.C_KM_S
sn = amd.sn_pantheon

MODE, OUT = sys.argv[1], sys.argv[2]
HALO, SEG, GUARD_NODES = 64, 512, 64 // 2 - 4  # csrc/cosmofit_device.h
results = {}


def permuted(syn, seed):
    """The SNe in a seeded random order (the covariance permuted with them): z_cmb is not sorted."""
    p = np.random.default_rng(seed).permutation(syn["z_cmb"].size)
    cov = syn["cov"][np.ix_(p, p)]
    return dict(z_cmb=syn["z_cmb"][p], z_hel=syn["z_hel"][p], obs=syn["obs"][p], chol=np.linalg.cholesky(cov))


def engine_of(data, n_grid=4000, step=None, lin_coef=None, z_max=None):
    z_max = float(np.max(data["z_cmb"]) + 0.1) if z_max is None else z_max
    params = dict(offset=Param(0), H0=Param(1), Om=Param(2))
    params["lin" if lin_coef is not None else "v"] = Param(3)
    return LikelihoodEngine(ndim=4, z_max=z_max, n_grid=n_grid, params=params,
                            sn=dict(z_cmb=data["z_cmb"], z_hel=data["z_hel"], obs=data["obs"], chol=data["chol"], z_turn=sn.Z_TURN,
                                    step=step, lin_coef=lin_coef),
                            bounds=sn.bounds, gauss=[sn.H0_PRIOR], solve_mode=eng_mod.solve_mode_of("inverse")), z_max


def thetas(W, data, z_max, n_grid, max_step=1.0, seed=5):
    """Rows inside the box, at both ends of v, just inside / just outside / far outside the streaming kernel's guard, one that puts
    z_cosmo of the lowest SN below 0, one with NaN v."""
    th = amd.synthetic.walkers(sn.bounds, W, seed=seed)
    inv_step = (n_grid - 1) / z_max
    K = (1.0 + float(np.max(data["z_cmb"]))) * inv_step
    a_star = GUARD_NODES / (K + GUARD_NODES)          # shift bound K a / (1 - a) = GUARD_NODES
    v_star = a_star * C_KM_S / max_step / 100.0       # in the sampler's units of 100 km/s
    z_low = float(np.min(data["z_cmb"]))
    v_neg = (1.0 + 2.0 * z_low) * z_low * C_KM_S / 100.0 / max_step + 1.0  # (1 + z_low) / (1 + v / c) - 1 < 0
    special = [-2.999999, 2.999999, v_star * (1 - 1e-9), v_star * (1 + 1e-9), -v_star * (1 - 1e-9), -v_star * (1 + 1e-9),
               3.0 * v_star, -3.0 * v_star, 100.0, v_neg, -v_neg, np.nan]
    for k, v in enumerate(special):
        th[3 + 7 * k, 3] = v
    return th


def run(name, eng, theta, kinds=("chi2", "logp")):
    W = theta.shape[0]
    if MODE in ("0", "1"):
        form = eng.walker_form(W)
        assert form == int(MODE), f"{name}: cf_walker_form({W}) = {form} under CF_TUNE={os.environ.get('CF_TUNE')}"
    for kind in kinds:
        f = {"chi2": eng.chi_squared, "logp": eng.log_probability, "logl": eng.log_likelihood}[kind]
        a, b = f(theta), f(theta)
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), f"{name}: repeated evaluations differ"
        results[f"{name}:{kind}"] = a


def boundary_data(n_grid, z_max, seed):
    """SNe within a node of a segment boundary and of the packing boundary on either side, one below node 1, the rest between
    nodes 2600 and 3000: inside segment 5 only on the grids of 4000 and 4096 nodes (segments with no SN at all); on the grid of
    520 nodes those lie above z_max and take the extrapolation above the grid, in the last segment."""
    step = z_max / (n_grid - 1)
    nodes = [0.3, 510.5, 511.5, 512.5, 513.5, SEG - HALO // 2 - 1.5, SEG - HALO // 2 - 0.5, SEG - HALO // 2 + 0.5,
             SEG - HALO // 2 + 1.5, 511.999, 512.001, SEG - HALO // 2 - 0.001, SEG - HALO // 2 + 0.001]
    rng = np.random.default_rng(seed)
    far = 5 * SEG + 40 + 400 * rng.random(70 - len(nodes))
    z = np.concatenate([nodes, far]) * step
    syn = amd.synthetic.pantheon_like(n_sn=z.size, seed=seed)
    p = rng.permutation(z.size)
    return dict(z_cmb=z[p], z_hel=z[p] * (1 + 1e-4), obs=syn["obs"], chol=syn["chol"])


if MODE == "auto":
    data = permuted(amd.synthetic.pantheon_like(n_sn=1701, seed=0), 1)
    eng, z_max = engine_of(data)
    rows = thetas(176, data, z_max, 4000)[[3 + 7 * k for k in range(12)] + list(range(100, 120))]  # the special rows + 20 ordinary
    assert eng.walker_form(176) == 0 and eng.walker_form(4096) == 1, (eng.walker_form(176), eng.walker_form(4096))
    for W in (176, 4096):
        th = amd.synthetic.walkers(sn.bounds, W, seed=9)
        th[40:72] = rows
        results[f"invariance_{W}:chi2"] = eng.chi_squared(th)[40:72]
        results[f"invariance_{W}:logp"] = eng.log_probability(th)[40:72]
    # a batch that ends in a partly filled round of the chip and a partly filled workgroup of the streaming form; one just above
    # a full round keeps the workgroup form (the automatic rule of csrc/cosmofit_api.hip: walker_stream_chosen)
    W = 5201
    assert eng.walker_form(W) == 1 and eng.walker_form(4132) == 0, (eng.walker_form(W), eng.walker_form(4132))
    th = amd.synthetic.walkers(sn.bounds, W, seed=9)
    th[40:72] = rows
    th[W - 32:] = rows
    for kind, f in (("chi2", eng.chi_squared), ("logp", eng.log_probability)):
        out = f(th)
        results[f"invariance_split_head:{kind}"] = out[40:72]
        results[f"invariance_split_tail:{kind}"] = out[W - 32:]
    eng.close()
else:
    W = 176
    for n_sn in (70, 200):
        data = permuted(amd.synthetic.pantheon_like(n_sn=n_sn, seed=n_sn), n_sn)
        for n_grid in ((4000,) if n_sn == 70 else (4000, 1000, 4096, 520)):
            eng, z_max = engine_of(data, n_grid=n_grid)
            run(f"pm1_n{n_sn}_g{n_grid}", eng, thetas(W, data, z_max, n_grid))
            eng.close()
    for n_grid in (4000, 4096, 520):
        z_max = 2.36
        data = boundary_data(n_grid, z_max, 11)
        eng, _ = engine_of(data, n_grid=n_grid, z_max=z_max)
        run(f"boundary_g{n_grid}", eng, thetas(W, data, z_max, n_grid))
        eng.close()
    data = permuted(amd.synthetic.pantheon_like(n_sn=200, seed=21), 21)
    weights = np.random.default_rng(21).uniform(-0.95, 0.95, 200)
    eng, z_max = engine_of(data, step=weights)
    run("weights_n200", eng, thetas(W, data, z_max, 4000, max_step=float(np.max(np.abs(weights)))))
    eng.close()
    eng, z_max = engine_of(data, lin_coef=np.random.default_rng(22).standard_normal(200))
    run("lin_n200", eng, thetas(W, data, z_max, 4000))
    eng.close()
    data = permuted(amd.synthetic.pantheon_like(n_sn=1701, seed=0), 1)
    eng, z_max = engine_of(data)
    run("pm1_n1701_g4000", eng, thetas(192, data, z_max, 4000))
    eng.close()
    # the joint likelihood bench.py builds for --workload desi_cmb_des5y --fde cpl: BAO table nodes (n_aux > 0), CPL table build
    g = np.load(os.path.join(ROOT, "tests", "golden", "bao_desi_cmb_des5y.npz"))
    A = 0.01 * np.random.default_rng(0).standard_normal((g["sigma"].size, 40))
    chol = np.linalg.cholesky(np.diag(g["sigma"] ** 2) + A @ A.T)
    lk = amd.likelihoods.DesiCmbDes5y(g["z_cmb"], g["z_hel"], g["obs"], None, g["bao_z"], g["bao_val"], g["bao_qty"], g["bao_inv_cov"],
                                      chol=chol, fde="cpl")
    box = np.array([(-0.5, 0.5), (60.0, 75.0), (0.010, 0.030), (0.01, 0.25), (-4.5, 4.5), (-3.0, 1.0), (-3.0, 2.0)])
    run("joint_cpl", lk.engine, amd.synthetic.walkers(box, W, seed=3), kinds=("logl",))
    lk.engine.close()

np.savez(OUT, **results)
