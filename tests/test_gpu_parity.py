"""
GPU (-m gpu): the HIP path, called through the C-ABI, against the CPU oracle and the golden
vectors generated from the reference.  Tolerances: chi^2 / log-probability <= 1e-10 relative
(BASELINE.json north_star); intermediates looser only where a cancellation amplifies rounding.
"""
import os

import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

RTOL = 1e-10  # the parity bar of BASELINE.json


@pytest.fixture(scope="module")
def gpu(pkg):
    if pkg.lib().cf_device_count() < 1:
        pytest.fail("GPU tests need an MI355X; no HIP device visible (there is no fallback path)")
    return pkg


def _spd_chol(n, seed, garbage=True):
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((n, n))
    L = np.linalg.cholesky(M @ M.T + n * np.eye(n))
    if garbage:  # cho_factor semantics: the strict upper triangle holds junk that must be ignored
        L = L + np.triu(rng.standard_normal((n, n)), 1) * 5.0
    return L


# ---- a11: solve_triangular -----------------------------------------------------------------
@pytest.mark.parametrize("n,nrhs", [(1, 1), (15, 3), (16, 16), (17, 17), (129, 5), (256, 33), (257, 2), (531, 40),
                                    (1701, 48)])
def test_solve_triangular_vs_oracle(gpu, n, nrhs):
    from oracle import oracle_c as oc

    L = _spd_chol(n, seed=n + nrhs)
    b = np.random.default_rng(7).standard_normal((nrhs, n))
    got = gpu.solve_triangular.solve_triangular(L, b)
    ref = np.array([oc.solve_triangular(L, bb) for bb in b])
    np.testing.assert_allclose(got, ref, rtol=1e-12)
    if nrhs == 1:
        assert isinstance(gpu.solve_triangular.solve_triangular(L, b[0]), float)


def test_solve_triangular_golden_and_properties(gpu):
    g = golden("interpolator")
    got = gpu.solve_triangular.solve_triangular(g["t_L"], g["t_b"])
    np.testing.assert_allclose(got, g["t_out"], rtol=1e-12)
    # quadratic form properties: chi2(a b) = a^2 chi2(b); chi2 >= 0; == b^T C^-1 b
    got3 = gpu.solve_triangular.solve_triangular(g["t_L"], -3.0 * g["t_b"])
    np.testing.assert_allclose(got3, 9.0 * got, rtol=1e-13)
    assert np.all(got >= 0)
    Lc = np.tril(g["t_L"])
    np.testing.assert_allclose(got, [b @ np.linalg.solve(Lc @ Lc.T, b) for b in g["t_b"]], rtol=1e-10)


def test_solve_triangular_rejects_bad_factor(gpu):
    L = np.eye(40)
    L[11, 11] = -1.0
    with pytest.raises(gpu.CosmofitError, match="CF_ERR_NOT_POSDEF"):
        gpu.solve_triangular.solve_triangular(L, np.ones(40))


# ---- a6 / a7: interpolators ------------------------------------------------------------------
def test_interpolators_golden(gpu):
    g = golden("interpolator")
    ip = gpu.interpolator
    np.testing.assert_allclose(ip.interp_hermite(g["h_xq"], g["h_x"], g["h_y"], g["h_yp"]), g["h_out"], rtol=1e-14)
    np.testing.assert_allclose(ip.interp_pchip(g["p_xq"], g["p_x"], g["p_y"]), g["p_out"], rtol=1e-13, atol=1e-14)
    np.testing.assert_allclose(ip.interp_pchip(g["m_xq"], g["m_x"], g["m_y"]), g["m_out"], rtol=1e-14)
    # PCHIP end-point branches (sign change, overshoot clamp, flat): evaluate next to the ends
    for name in ("p3", "p4"):
        x, y = g[name + "_x"], g[name + "_y"]
        xq = np.concatenate([np.linspace(x[0], x[-1], 41), [x[0] - 1, x[-1] + 1]])
        from oracle import oracle_np as onp
        np.testing.assert_allclose(ip.interp_pchip(xq, x, y), onp.interp_pchip(xq, x, y), rtol=1e-14, atol=1e-15)


def test_interp_hermite_reproduces_nodes_and_slopes(gpu):
    rng = np.random.default_rng(3)
    x = np.sort(rng.uniform(0, 5, 200))
    y, yp = np.sin(x), np.cos(x)
    ih = gpu.interpolator.interp_hermite
    np.testing.assert_allclose(ih(x[1:-1], x, y, yp), y[1:-1], rtol=1e-13, atol=1e-14)
    eps = 1e-6
    num = (ih(x[1:-1] + eps, x, y, yp) - ih(x[1:-1] - eps, x, y, yp)) / (2 * eps)
    np.testing.assert_allclose(num, yp[1:-1], rtol=0, atol=1e-6)
    # linear extrapolation outside the grid with the end slopes
    np.testing.assert_allclose(ih(np.array([-1.0, 7.0]), x, y, yp), [y[0] + yp[0] * (-1 - x[0]), y[-1] + yp[-1] * (7 - x[-1])], rtol=1e-14)


# ---- a1-a10 + a11 + a17: the SN likelihood against the reference's golden vectors -----------
@pytest.fixture(scope="module", params=["inverse", "blocked"])
def pantheon_lk(gpu, pantheon_golden, request):
    g = pantheon_golden
    lk = gpu.sn_pantheon.PantheonLikelihood(g["z_cmb"], g["z_hel"], g["obs"], chol=g["chol"], bounds=g["bounds"], solve=request.param)
    assert lk.engine.info()["solve_mode"] == gpu._lib.SOLVE_MODES[request.param]
    assert abs(lk.z_max - float(g["z_max"])) == 0.0
    yield lk
    lk.engine.close()


def test_sn_pantheon_golden_chi2_logp(pantheon_lk, pantheon_golden):
    g, lk = pantheon_golden, pantheon_lk
    finite = np.isfinite(g["logp"])
    chi2 = lk.chi_squared(g["thetas"])
    logp = lk.log_probs_vectorized(g["thetas"])
    logl = lk.log_likelihood(g["thetas"])
    np.testing.assert_allclose(chi2[finite], g["chi2"][finite], rtol=RTOL)
    np.testing.assert_allclose(logp[finite], g["logp"][finite], rtol=RTOL)
    np.testing.assert_allclose(logl[finite], g["logl"][finite], rtol=RTOL)
    assert np.all(logp[~finite] == -np.inf), "outside the strict box (edges included) the reference returns -inf"
    assert not np.any(np.isnan(logp)) and not np.any(np.isnan(logl)), "emcee aborts on NaN"
    # single-theta call signature: log_probability(theta[ndim]) -> float
    k = int(np.flatnonzero(finite)[0])
    one = lk.log_probability(g["thetas"][k])
    assert isinstance(one, float) and one == pytest.approx(g["logp"][k], rel=RTOL)


def test_sn_pantheon_golden_intermediates(pantheon_lk, pantheon_golden):
    g, lk = pantheon_golden, pantheon_lk
    parts = lk.engine.parts(g["thetas"][:3])
    for k in range(3):
        np.testing.assert_allclose(parts["dm"][k], g[f"dm_{k}"], rtol=1e-13)
        np.testing.assert_allclose(parts["mu_corr"][k], g[f"mucorr_{k}"], rtol=0, atol=1e-13)
        np.testing.assert_allclose(parts["delta"][k], g[f"delta_{k}"], rtol=0, atol=1e-12)
        np.testing.assert_allclose(lk.mu_theory(g["thetas"][k]), g[f"muth_{k}"], rtol=1e-14)


# ---- BASELINE config 2 (N=1701, W=4096) at full size ------------------------------------------
@pytest.fixture(scope="module", params=["auto", "blocked"])
def config2(gpu, request):
    """Both solve kernels at full size; "auto" is what every mirror uses by default and picks the inverse-GEMM solve here."""
    from oracle import oracle_c, oracle_np as onp

    syn = gpu.synthetic.pantheon_like(n_sn=1701, seed=0)
    lk = gpu.sn_pantheon.PantheonLikelihood(syn["z_cmb"], syn["z_hel"], syn["obs"], chol=syn["chol"], solve=request.param)
    want_mode = gpu.CF_SOLVE_BLOCKED_TRSM if request.param == "blocked" else gpu.CF_SOLVE_INVERSE_GEMM
    assert lk.engine.info()["solve_mode"] == want_mode
    ref = oracle_c.COracle(onp.Likelihood(
        ndim=4, z_max=lk.z_max, offset=onp.Slot(0), H0=onp.Slot(1), Om=onp.Slot(2), v=onp.Slot(3),
        z_cmb=syn["z_cmb"], z_hel=syn["z_hel"], obs=syn["obs"], chol=syn["chol"],
        bounds=gpu.sn_pantheon.bounds, gauss=[gpu.sn_pantheon.H0_PRIOR]))
    theta = gpu.synthetic.walkers(gpu.sn_pantheon.bounds, 4096, seed=0)
    yield lk, ref, theta
    lk.engine.close()


def test_config2_full_batch_vs_oracle(config2):
    lk, ref, theta = config2
    got = lk.chi_squared(theta)
    want = ref.chi2(theta)  # 4096 x 1.1 ms on all host threads
    rel = np.abs(got - want) / np.abs(want)
    assert rel.max() < RTOL, f"max rel diff {rel.max():.3e} at walker {rel.argmax()}"
    np.testing.assert_allclose(lk.log_probs_vectorized(theta), ref.logp(theta), rtol=RTOL)
    assert lk.engine.info()["nonfinite_count"] == 0


def test_config2_batch_invariance(config2):
    """Walkers are independent: order, batch size and panel position must not change ANY bit."""
    lk, _, theta = config2
    full = lk.chi_squared(theta)
    perm = np.random.default_rng(5).permutation(len(theta))
    np.testing.assert_array_equal(lk.chi_squared(theta[perm]), full[perm])
    halves = np.concatenate([lk.chi_squared(theta[:2048]), lk.chi_squared(theta[2048:])])
    np.testing.assert_array_equal(halves, full)
    # ragged panels; the small-batch path (<= 160 walkers: residuals in fragment order, 4 / 2 workgroups per walker up to 64 / 160,
    # one / two tiles per solve workgroup up to 96 / 160) and the throughput kernel
    # 512 / 513: 16- / 32-walker panels.  865 .. 1792 walkers (28 .. 56 panels): the six lowest row blocks of a panel as two 16-walker
    # units each -- with the last panel's second half empty (W mod 32 in 1 .. 16: 897, 1040, 1777), partly filled (1000, 1500) and
    # full (896, 1792); 1793: whole units again.  The 4096-walker batch multiplies nothing it may skip either (padded tiles of the
    # last row block, zero tiles of the diagonal blocks), like every batch here.
    for W in (1, 2, 15, 16, 17, 31, 33, 48, 63, 64, 65, 96, 97, 100, 127, 128, 129, 160, 161, 256, 257, 512, 513, 864, 865, 896, 897, 1000,
              1040, 1500, 1777, 1792, 1793, 3000):
        np.testing.assert_array_equal(lk.chi_squared(theta[:W]), full[:W], err_msg=f"W={W}")
    assert lk.chi_squared(theta[:0]).shape == (0,)


def test_config2_random_small_batches_soak(config2):
    """Thousands of synchronous calls of random batch sizes at random offsets (mostly the small-batch path: fragment-ordered
    residuals, one / two tiles per solve workgroup, several workgroups per walker, completion words), every result the same BITS as
    in the 4096-walker batch: an intermittent hand-off or completion race would show here (tools/soak_small_batches.py runs 10^5s)."""
    lk, _, theta = config2
    full = np.array(lk.log_probs_vectorized(theta), copy=True)
    rng = np.random.default_rng(11)
    sizes = np.concatenate([rng.integers(1, 200, 2700), rng.integers(200, 3000, 300)])
    rng.shuffle(sizes)
    prev = (0, 0)
    for W in sizes:
        o = int(rng.integers(0, len(theta) - W + 1))
        got = lk.log_probs_vectorized(theta[o:o + W])
        if not np.array_equal(got, full[o:o + W]):  # whose results are the wrong ones? another walker's = stale theta / table / results
            j = int(np.flatnonzero(got != full[o:o + W])[0])
            owners = np.flatnonzero(full == got[j]).tolist()
            again = np.array_equal(lk.log_probs_vectorized(theta[o:o + W]), full[o:o + W])
            pytest.fail(f"W={W} offset={o}: {int((got != full[o:o + W]).sum())} of {W} wrong, first at row {j}: {got[j]!r} instead of "
                        f"{full[o + j]!r}; that value is walker {owners}'s; previous call W={prev[0]} offset={prev[1]}; the same call again is "
                        f"{'right' if again else 'wrong again'}")
        prev = (int(W), o)


@pytest.mark.parametrize("W", [16, 1000, 4096])
def test_device_evaluation_is_captured_into_a_graph_and_replayed(gpu, W):
    """evaluations that stay on one stream are purely asynchronous and may be captured into a hipGraph.  Capture one
    cf_eval_device of each kernel family (small-batch, throughput) on a torch stream, overwrite theta in place, replay: the replayed
    result must be the bits of a direct call on the new theta."""
    torch = pytest.importorskip("torch")
    syn = gpu.synthetic.pantheon_like(n_sn=1701, seed=0)
    lk = gpu.sn_pantheon.PantheonLikelihood(syn["z_cmb"], syn["z_hel"], syn["obs"], chol=syn["chol"])
    try:
        f = lk.engine.torch_log_prob()
        dev = torch.device("cuda:0")
        th_a = torch.from_numpy(gpu.synthetic.walkers(gpu.sn_pantheon.bounds, W, seed=1)).to(dev)
        th_b = torch.from_numpy(gpu.synthetic.walkers(gpu.sn_pantheon.bounds, W, seed=2)).to(dev)
        x = th_a.clone()
        s = torch.cuda.Stream(dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            want_a = f(x).clone()  # the first call on this stream: workspace, stream switch -- neither may happen under capture
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=s):
                out = f(x)
            graph.replay()
            s.synchronize()
            assert torch.equal(out, want_a)
            x.copy_(th_b)
            graph.replay()
            graph.replay()  # back to back: the arrival counters re-arm themselves
            s.synchronize()
            got_b = out.clone()
            want_b = f(th_b)
            s.synchronize()
        assert torch.equal(got_b, want_b) and not torch.equal(want_a, want_b)
    finally:
        lk.engine.close()


@pytest.mark.parametrize("W", [8192, 65536])
def test_configs3_shape_per_rank_and_whole_ensemble(config2, W):
    """BASELINE configs[3]: 65536 walkers over 8 GPUs = 8192 per rank.  Both shapes on ONE GPU (the per-rank batch, and the
    whole ensemble as a strong-scaling N = 1 run would see it): the oracle on a 512-walker subset, bit-equality with the
    same walkers evaluated in 4096-walker batches (batch invariance), the device-resident entry point bit-equal to the
    host one, and the size-independent property chi2(theta) >= 0 with no non-finite result."""
    import torch

    lk, ref, theta4096 = config2
    gpu_pkg = __import__("conftest").load_pkg()
    theta = gpu_pkg.synthetic.walkers(gpu_pkg.sn_pantheon.bounds, W, seed=0)
    assert np.array_equal(theta[:0], theta4096[:0]) and theta.shape == (W, 4)
    got = lk.log_probs_vectorized(theta)
    assert got.shape == (W,) and np.all(np.isfinite(got))
    pick = np.sort(np.random.default_rng(W).choice(W, 512, replace=False))
    pick[0], pick[-1] = 0, W - 1
    want = ref.logp(theta[pick])
    rel = np.abs(got[pick] - want) / np.abs(want)
    assert rel.max() < RTOL, f"max rel diff {rel.max():.3e}"
    for a in (0, W // 2, W - 4096):  # the same walkers in a 4096 batch: not one bit may differ
        np.testing.assert_array_equal(lk.log_probs_vectorized(theta[a:a + 4096]), got[a:a + 4096])
    th = torch.from_numpy(theta).cuda()
    out = torch.empty(W, dtype=torch.float64, device="cuda")
    lk.engine.eval_device(th.data_ptr(), W, out.data_ptr(), gpu_pkg.CF_OUT_LOGP, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), got)
    chi2 = lk.chi_squared(theta)
    assert np.all(chi2 >= 0) and lk.engine.info()["nonfinite_count"] == 0


def test_config2_offset_parameter_property(config2):
    """chi^2 is an exact quadratic in the magnitude offset M: chi2(M) = a + b M + c M^2 with c = 1^T C^-1 1."""
    lk, _, theta = config2
    base = theta[:8].copy()
    Ms = np.array([-19.9, -19.6, -19.3, -19.1])
    vals = []
    for M in Ms:
        t = base.copy()
        t[:, 0] = M
        vals.append(lk.chi_squared(t))
    vals = np.array(vals)  # [4, 8]
    for k in range(8):
        coef = np.polyfit(Ms, vals[:, k], 2)
        fit = np.polyval(coef, Ms)
        np.testing.assert_allclose(fit, vals[:, k], rtol=1e-9)
        assert coef[0] > 0


def test_device_resident_eval_matches_host_eval(gpu, config2):
    torch = pytest.importorskip("torch")
    lk, _, theta = config2
    th = torch.from_numpy(theta[:1000]).to("cuda:0")
    out = torch.empty(1000, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    lk.engine.eval_device(th.data_ptr(), 1000, out.data_ptr(), gpu.CF_OUT_LOGP, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), lk.log_probs_vectorized(theta[:1000]))


def test_nonfinite_is_minus_inf_and_counted(gpu):
    syn = gpu.synthetic.pantheon_like(n_sn=64, seed=1)
    lk = gpu.sn_pantheon.PantheonLikelihood(syn["z_cmb"], syn["z_hel"], syn["obs"], chol=syn["chol"],
                                            bounds=np.array([(-20, -19), (50, 90), (-5.0, 0.7), (-3, 3)]))
    th = np.array([[-19.3, 70.0, 0.3, 0.0], [-19.3, 70.0, -4.0, 0.0]])  # Om = -4: sqrt of a negative number
    lp = lk.log_probs_vectorized(th)
    assert np.isfinite(lp[0]) and lp[1] == -np.inf
    assert lk.engine.info()["nonfinite_count"] == 1
    lk.engine.close()


# ---- 8e / 8f-1: device-resident ensemble driving the HIP path through cf_eval_device -----------------------
def test_device_ensemble_stretch_move_matches_oracle_driven_chain(gpu):
    torch = pytest.importorskip("torch")
    from oracle import oracle_c, oracle_np as onp

    syn = gpu.synthetic.pantheon_like(n_sn=200, seed=5)
    lk = gpu.sn_pantheon.PantheonLikelihood(syn["z_cmb"], syn["z_hel"], syn["obs"], chol=syn["chol"])
    co = oracle_c.COracle(onp.Likelihood(
        ndim=4, z_max=lk.z_max, offset=onp.Slot(0), H0=onp.Slot(1), Om=onp.Slot(2), v=onp.Slot(3),
        z_cmb=syn["z_cmb"], z_hel=syn["z_hel"], obs=syn["obs"], chol=syn["chol"],
        bounds=gpu.sn_pantheon.bounds, gauss=[gpu.sn_pantheon.H0_PRIOR]))
    start = gpu.synthetic.THETA_TRUE + 1e-2 * np.random.default_rng(1).standard_normal((96, 4))
    ens_gpu = gpu.ensemble.ShardedEnsemble(lk.engine.torch_log_prob(), torch.from_numpy(start).to("cuda:0"), seed=3)
    from oracle import moves_torch
    ens_cpu = gpu.ensemble.ShardedEnsemble(lambda t: torch.from_numpy(co.logp(t.numpy())), torch.from_numpy(start), seed=3,
                                           moves_impl=moves_torch.TensorMoves(gpu.ensemble.stream_key))
    ens_gpu.run(12)
    ens_cpu.run(12)
    torch.cuda.synchronize()
    np.testing.assert_allclose(ens_gpu.x.cpu().numpy(), ens_cpu.x.numpy(), rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(ens_gpu.logp.cpu().numpy(), ens_cpu.logp.numpy(), rtol=1e-9)
    assert ens_gpu.n_accepted == ens_cpu.n_accepted and 0 < ens_gpu.n_accepted < ens_gpu.n_proposed
    lk.engine.close()


@pytest.mark.parametrize("ndim,n_total", [(4, 512), (6, 130), (1, 64)])
@pytest.mark.parametrize("randomize", [False, True])
def test_native_ensemble_moves_match_the_tensor_statement(gpu, ndim, n_total, randomize):
    """cf_ens_active_set / cf_ens_kde_prepare / cf_ens_propose / cf_ens_accept against oracle/moves_torch.py's tensor statement of
    the same moves (same counter-based random numbers): active sets, proposals, Hastings factors, KDE fit, accept decisions --
    for two and three splits, with the fixed classes and the per-step re-drawn splits, and for SHARDS that do not start at
    walker 0 (shard_start != 0, boundaries that cut pairs and triples): the local index of a walker is its global index less the
    shard start, which is what a rank r > 0 of the sharded ensemble hands to the kernels."""
    torch = pytest.importorskip("torch")
    from oracle import moves_torch

    E = gpu.ensemble
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(ndim)
    pos = torch.from_numpy(rng.standard_normal((n_total, ndim)) * np.linspace(0.5, 2.0, ndim) + 3.0).to(dev)
    f = lambda t: -0.5 * ((t - 3.0) ** 2).sum(dim=1)
    ens = E.ShardedEnsemble(f, pos, seed=11, moves=E.REFERENCE_MOVES, randomize_split=randomize)
    assert isinstance(ens.impl, E.NativeMoves)
    tm = moves_torch.TensorMoves(E.stream_key)
    lib, L, stream = gpu.lib(), gpu._lib, torch.cuda.current_stream(dev).cuda_stream
    all_ids = torch.arange(n_total, dtype=torch.int64, device=dev)
    kde_params = torch.empty(2 * ndim * ndim + 1, dtype=torch.float64, device=dev)
    kde_wc = torch.empty((n_total, ndim), dtype=torch.float64, device=dev)
    lp_all = f(pos)
    shards = [(0, n_total), (n_total // 3 + 1, 2 * n_total // 3), (n_total - 7, n_total), (5, 6)]
    for step in (0, 5):
        ens.step_count = step
        split_key = E.stream_key(ens.seed, step, 0, E._SPLIT_STREAM) if randomize else 0
        for S in (2, 3):
            sp = moves_torch.split_of(split_key, S, all_ids)
            if randomize:
                assert not torch.equal(sp, all_ids % S)
            for split in range(S):
                comp = pos[sp != split]
                assert lib.cf_ens_comp_count(split_key, S, split, n_total) == comp.shape[0]
                key0 = E.stream_key(ens.seed, step, split)
                for start, stop in shards:
                    ids = all_ids[start:stop][sp[start:stop] == split].contiguous()
                    idx = ids - start
                    n = int(ids.numel())
                    assert lib.cf_ens_active_count(split_key, S, split, start, stop) == n == E.active_count(split_key, S, split, start, stop)
                    # the library's own active set, sentinel-filled buffers one entry longer than the count
                    k_ids = torch.full((n + 1,), -7, dtype=torch.int64, device=dev)
                    k_idx = torch.full((n + 1,), -7, dtype=torch.int64, device=dev)
                    L.check(lib.cf_ens_active_set(split_key, S, split, start, stop, k_ids.data_ptr(), k_idx.data_ptr(), stream))
                    torch.cuda.synchronize()
                    assert torch.equal(k_ids[:n], ids) and torch.equal(k_idx[:n], idx) and int(k_ids[n]) == -7 and int(k_idx[n]) == -7
                    if n == 0:
                        continue
                    x_shard, lp_shard = pos[start:stop].clone(), lp_all[start:stop].clone()
                    for kind, name in enumerate(("stretch", "de", "kde")):
                        want_y, want_lf = getattr(tm, "propose_" + name)(ens, pos[ids], ids, comp, split)
                        if kind == 2:
                            L.check(lib.cf_ens_kde_prepare(pos.data_ptr(), n_total, ndim, S, split, split_key, kde_params.data_ptr(),
                                                           kde_wc.data_ptr(), stream))
                        y, lf = torch.empty((n, ndim), dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev)
                        L.check(lib.cf_ens_propose(kind, pos.data_ptr(), n_total, ndim, S, split, split_key, k_ids.data_ptr(), n, key0,
                                                   ens.a, ens.de_sigma, kde_params.data_ptr(), kde_wc.data_ptr(), y.data_ptr(),
                                                   lf.data_ptr(), stream))
                        torch.cuda.synchronize()
                        np.testing.assert_allclose(y.cpu().numpy(), want_y.cpu().numpy(), rtol=1e-11, atol=1e-12, err_msg=name)
                        np.testing.assert_allclose(lf.cpu().numpy(), want_lf.cpu().numpy(), rtol=1e-9, atol=1e-9, err_msg=name)
                        # accept on the SHARD's arrays (local indices): same decisions as log(u) < log_factor + lp_new - lp_old
                        x_loc, lp_loc = x_shard.clone(), lp_shard.clone()
                        lp_new = f(y)
                        u = tm.uniform01(ens.seed, step, split, ids, 2)
                        want_acc = torch.log(u) < (lf + lp_new - lp_shard[idx])
                        count = torch.zeros(1, dtype=torch.int64, device=dev)
                        L.check(lib.cf_ens_accept(k_ids.data_ptr(), k_idx.data_ptr(), n, ndim, key0, y.data_ptr(), lp_new.data_ptr(),
                                                  lf.data_ptr(), x_loc.data_ptr(), lp_loc.data_ptr(), count.data_ptr(), stream))
                        torch.cuda.synchronize()
                        assert int(count.item()) == int(want_acc.sum())
                        exp_x, exp_lp = x_shard.clone(), lp_shard.clone()
                        exp_x[idx[want_acc]] = y[want_acc]
                        exp_lp[idx[want_acc]] = lp_new[want_acc]
                        assert torch.equal(x_loc, exp_x) and torch.equal(lp_loc, exp_lp)
    # whole steps of the driver: the kernels' chain == the tensor statement's chain on the same target
    e_native = E.ShardedEnsemble(f, pos.clone(), seed=4, moves=E.REFERENCE_MOVES, randomize_split=randomize)
    e_tensor = E.ShardedEnsemble(f, pos.clone(), seed=4, moves=E.REFERENCE_MOVES, randomize_split=randomize, moves_impl=tm)
    e_native.run(8)
    e_tensor.run(8)
    torch.cuda.synchronize()
    np.testing.assert_allclose(e_native.x.cpu().numpy(), e_tensor.x.cpu().numpy(), rtol=1e-9, atol=1e-11)
    assert e_native.n_accepted == e_tensor.n_accepted and e_native.n_proposed == e_tensor.n_proposed


def test_in_kernel_log10_is_within_one_ulp(gpu):
    import ctypes as C
    rng = np.random.default_rng(0)
    x = np.concatenate([np.exp(rng.uniform(np.log(1e-3), np.log(1e6), 400000)),  # the range distances live in
                        np.exp(rng.uniform(-700, 700, 100000)), [1.0, 10.0, 1e5, 0.5, 2.0, np.sqrt(0.5), np.sqrt(2.0)],
                        [0.0, -1.0, np.inf, np.nan, 5e-324]])
    out = np.empty_like(x)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    gpu._lib.check(gpu.lib().cf_selftest_log10(p(x), x.size, p(out)))
    with np.errstate(all="ignore"):
        ref = np.log10(x)
    fin = np.isfinite(ref)
    ulp = np.abs(out[fin] - ref[fin]) / np.spacing(np.abs(ref[fin]) + 5e-324)
    assert ulp.max() <= 1.0, f"max error {ulp.max()} ulp"
    assert out[x == 1.0][0] == 0.0 and out[x == 10.0][0] == 1.0
    assert out[-5] == -np.inf and np.isnan(out[-4]) and out[-3] == np.inf and np.isnan(out[-2])


def test_table_build_exp_is_within_two_ulp(gpu):
    """exp_tab: the table-driven exp of the wCDM / CPL dark-energy density in walker_kernel's table build; its argument is
    3 (1 + w0 + wa) ln(1 + z) - 3 wa z / (1 + z), |x| < 40 for any prior box of the reference's scripts."""
    import ctypes as C
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.uniform(-40, 40, 400000), rng.uniform(-1e-3, 1e-3, 50000), rng.uniform(-700, 700, 50000),
                        [0.0, np.log(2) / 64, -np.log(2) / 128, 1.0, -1.0, 25.0]])
    out = np.empty_like(x)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    gpu._lib.check(gpu.lib().cf_selftest_exp_tab(p(x), x.size, p(out)))
    ref = np.exp(x.astype(np.longdouble))
    ulp = np.abs(out - ref) / np.spacing(np.exp(x))
    assert float(ulp.max()) <= 2.0, f"max error {float(ulp.max())} ulp"
    assert out[x == 0.0][0] == 1.0


def test_positive_operand_sqrt_and_quotient_are_the_library_bits(gpu):
    """sqrt_pos / div_pos (H(z) at the Gauss-Legendre nodes of the compressed-CMB distances, small_blocks_kernel): the library
    routines' instruction sequences without the exponent scaling and class selects that positive, finite, normal operands never take.
    The claim is THE SAME BITS as sqrt() and a / b on the device -- and, both being correctly rounded there, as numpy's."""
    import ctypes as C
    rng = np.random.default_rng(5)
    a = np.concatenate([np.exp(rng.uniform(np.log(1e-6), np.log(1e30), 400000)), rng.uniform(0.5, 4.0, 100000),
                        np.exp(rng.uniform(-230, 230, 100000)), [1.0, 2.0, 4.0, 0.25, 3.0, 1e-200, 1e200]])
    b = np.concatenate([np.exp(rng.uniform(np.log(1e-6), np.log(1e12), 400000)), rng.uniform(0.5, 4.0, 100000),
                        np.exp(rng.uniform(-230, 230, 100000)), [3.0, 3.0, 7.0, 0.1, 1.0, 1e-100, 1e-100]])
    out = np.empty((a.size, 4))
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    gpu._lib.check(gpu.lib().cf_selftest_pos_ops(p(a), p(b), a.size, p(out)))
    assert np.array_equal(out[:, 0], out[:, 1]), "sqrt_pos differs from the device library's sqrt"
    assert np.array_equal(out[:, 2], out[:, 3]), "div_pos differs from the device library's quotient"
    assert np.array_equal(out[:, 1], np.sqrt(a)) and np.array_equal(out[:, 3], a / b)


def test_quotient_of_a_negative_or_zero_numerator_is_the_library_bits(gpu):
    """div_pos with the numerators the CPL exponent at the Gauss-Legendre nodes hands it (H_at_gl_node: -3 wa z over 1 + z): negative
    for wa > 0, -0.0 for wa = 0 -- and +0.0 -- over positive denominators.  Only the two quotient columns are compared (the square
    root of such operands is not claimed): the same bits as a / b, the sign of a zero included."""
    import ctypes as C
    rng = np.random.default_rng(6)
    b = np.concatenate([1.0 + np.exp(rng.uniform(np.log(1e-6), np.log(1e8), 200000)), rng.uniform(0.5, 4.0, 50000),
                        np.exp(rng.uniform(-230, 230, 50000)), [1.0, 3.0, 7.0, 0.1, 1e-100, 1e100, 1100.0, 2.5]])
    a = -np.concatenate([3 * rng.uniform(0.0, 2.0, 200000) * (b[:200000] - 1.0), rng.uniform(0.5, 4.0, 50000),
                         np.exp(rng.uniform(-230, 230, 50000)), [1.0, 1.0, 3.0, 1e-200, 1e-100, 1e200, 3297.0, 4.5]])
    zeros = np.concatenate([np.full(1000, -0.0), np.full(1000, 0.0)])
    a = np.concatenate([a, zeros])
    b = np.concatenate([b, np.tile(b[:1000], 2)])
    assert np.all(b > 0) and np.all(a <= 0) and np.signbit(a).sum() == a.size - 1000
    out = np.empty((a.size, 4))
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    gpu._lib.check(gpu.lib().cf_selftest_pos_ops(p(a), p(b), a.size, p(out)))
    bits = lambda x: np.ascontiguousarray(x).view(np.uint64)
    bad = np.flatnonzero(bits(out[:, 2]) != bits(out[:, 3]))
    assert bad.size == 0, f"div_pos differs from the device library's quotient at {bad.size} operands; first: {a[bad[0]]!r} / {b[bad[0]]!r} -> {out[bad[0], 2]!r} vs {out[bad[0], 3]!r}"
    assert np.array_equal(bits(out[:, 3]), bits(a / b))


def test_production_loop_log10_absolute_error(gpu):
    """log10_tab (table-driven, production SN loop): what a distance modulus needs is ABSOLUTE accuracy of 5 log10(d)
    at the 1e-15 level on mu ~ 25..45; bound it at 3e-16 max(1, |log10 x|) over the whole double range."""
    import ctypes as C
    from decimal import Decimal, getcontext
    rng = np.random.default_rng(1)
    x = np.concatenate([np.exp(rng.uniform(np.log(1e-3), np.log(1e6), 400000)), np.exp(rng.uniform(-700, 700, 100000)),
                        1.0 + rng.uniform(-1e-3, 1e-3, 2000), [1.0, 10.0, 1e5, 0.5, 2.0, 0.999999, 1.000001],
                        [0.0, -1.0, np.inf, np.nan, 5e-324]])
    out = np.empty_like(x)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    gpu._lib.check(gpu.lib().cf_selftest_log10_tab(p(x), x.size, p(out)))
    with np.errstate(all="ignore"):
        ref = np.log10(x)
    fin = np.isfinite(ref)
    err = np.abs(out[fin] - ref[fin]) / np.maximum(1.0, np.abs(ref[fin]))
    assert err.max() <= 3e-16, f"max scaled error {err.max():.3e}"
    # numpy's own log10 is good to ~1 ulp; pin a handful of points against 40-digit arithmetic
    getcontext().prec = 40
    for k in rng.integers(0, 400000, 50):
        exact = float(Decimal(float(x[k])).log10())
        assert abs(out[k] - exact) <= 3e-16 * max(1.0, abs(exact))
    assert out[-5] == -np.inf and np.isnan(out[-4]) and out[-3] == np.inf and np.isnan(out[-2])


def test_ill_conditioned_factor_is_refused_not_silently_wrong(gpu, config2):
    lk, _, _ = config2
    assert lk.engine.info()["pack_probe_rel"] < 1e-13  # well-conditioned synthetic Pantheon+ factor
    n = 300
    rng = np.random.default_rng(0)
    bad = np.tril(rng.standard_normal((n, n)), -1) * 3.0 + np.diag(np.full(n, 1e-3))
    with pytest.raises(gpu.CosmofitError, match="CF_ERR_ILL_CONDITIONED"):
        gpu.solve_triangular.solve_triangular(bad, rng.standard_normal(n))
    z = np.sort(rng.uniform(0.01, 1.0, n))
    with pytest.raises(gpu.CosmofitError, match="CF_ERR_ILL_CONDITIONED"):
        gpu.sn_pantheon.PantheonLikelihood(z, z, 40 + 0 * z, chol=bad)


def test_batched_laplace_evidence_gpu_vs_oracle(gpu):
    """the job of log_evidence.py with every stencil as one GPU batch; same ln Z as with the CPU oracle."""
    from oracle import oracle_c, oracle_np as onp

    syn = gpu.synthetic.pantheon_like(n_sn=300, seed=4)
    lk = gpu.sn_pantheon.PantheonLikelihood(syn["z_cmb"], syn["z_hel"], syn["obs"], chol=syn["chol"])
    co = oracle_c.COracle(onp.Likelihood(
        ndim=4, z_max=lk.z_max, offset=onp.Slot(0), H0=onp.Slot(1), Om=onp.Slot(2), v=onp.Slot(3),
        z_cmb=syn["z_cmb"], z_hel=syn["z_hel"], obs=syn["obs"], chol=syn["chol"],
        bounds=gpu.sn_pantheon.bounds, gauss=[gpu.sn_pantheon.H0_PRIOR]))
    samples = gpu.synthetic.THETA_TRUE + np.array([0.02, 1.0, 0.03, 0.3]) * np.random.default_rng(2).standard_normal((64, 4))
    lp = lk.log_probs_vectorized(samples)
    z_gpu, d_gpu = gpu.laplace.log_evidence(samples, lp, lk.log_probs_vectorized, lk.bounds, return_details=True)
    z_cpu, d_cpu = gpu.laplace.log_evidence(samples, lp, co.logp, lk.bounds, return_details=True)
    assert np.isfinite(z_gpu) and z_gpu == pytest.approx(z_cpu, abs=1e-5)
    np.testing.assert_allclose(d_gpu["theta_map"], d_cpu["theta_map"], rtol=1e-5, atol=1e-6)
    assert d_gpu["log_post_map"] >= lp.max() - 1e-9
    lk.engine.close()


def test_auto_mode_falls_back_to_the_blocked_solve(gpu, config2):
    """CF_SOLVE_AUTO with a failing inverse probe (forced through cf_desc.probe_limit) must run the blocked solve."""
    _, ref, theta = config2
    syn = gpu.synthetic.pantheon_like(n_sn=1701, seed=0)
    lk = gpu.sn_pantheon.PantheonLikelihood(syn["z_cmb"], syn["z_hel"], syn["obs"], chol=syn["chol"], probe_limit=1e-300)
    assert lk.engine.info()["solve_mode"] == gpu.CF_SOLVE_BLOCKED_TRSM
    np.testing.assert_allclose(lk.log_probs_vectorized(theta[:200]), ref.logp(theta[:200]), rtol=RTOL)
    with pytest.raises(gpu.CosmofitError, match="CF_ERR_ILL_CONDITIONED"):
        gpu.sn_pantheon.PantheonLikelihood(syn["z_cmb"], syn["z_hel"], syn["obs"], chol=syn["chol"], solve="inverse", probe_limit=1e-300)
    lk.engine.close()


@pytest.mark.parametrize("solve", ["auto", "blocked"])
def test_replicas_do_not_change_a_walkers_result(gpu, solve):
    """one handle over several devices splits the rows of theta over its replicas (one host thread + one
    stream each).  On a one-GPU box the ordinals repeat -- two / three replicas on the same device exercise the same
    split, threads and streams; where more GPUs are visible, "all" spreads over them.  Results are bit-identical to the
    single-device handle."""
    syn = gpu.synthetic.pantheon_like(n_sn=531, seed=4)
    mk = lambda **kw: gpu.sn_pantheon.PantheonLikelihood(syn["z_cmb"], syn["z_hel"], syn["obs"], chol=syn["chol"], solve=solve, **kw)
    theta = gpu.synthetic.walkers(gpu.sn_pantheon.bounds, 3000, seed=5)
    theta[17, 2] = 0.9  # one walker outside the box
    one = mk()
    want = one.log_probs_vectorized(theta)
    for devs in ([0, 0], [0, 0, 0], "all"):
        lk = mk(devices=devs)
        info = lk.engine.info()
        assert info["n_devices"] == (gpu.lib().cf_device_count() if devs == "all" else len(devs))
        for W in (3000, 1, 31, 33, 64, 1000):
            assert np.array_equal(lk.log_probs_vectorized(theta[:W]), want[:W]), (devs, W)
        assert np.array_equal(lk.chi_squared(theta), one.chi_squared(theta))
        if info["n_devices"] > 1:
            import torch
            t = torch.zeros((64, 4), dtype=torch.float64, device="cuda")
            with pytest.raises(gpu.CosmofitError, match="several devices"):
                lk.engine.eval_device(t.data_ptr(), 64, t.data_ptr(), gpu.CF_OUT_LOGP, 0)
        lk.engine.close()
    one.engine.close()


def test_evaluations_on_different_streams_are_ordered(gpu):
    """cf_eval (the handle's own stream) right after an asynchronous cf_eval_device on the caller's stream
    shares the one workspace; the library orders them with an event."""
    import torch

    syn = gpu.synthetic.pantheon_like(n_sn=700, seed=6)
    lk = gpu.sn_pantheon.PantheonLikelihood(syn["z_cmb"], syn["z_hel"], syn["obs"], chol=syn["chol"])
    th_a = gpu.synthetic.walkers(gpu.sn_pantheon.bounds, 2048, seed=7)
    th_b = gpu.synthetic.walkers(gpu.sn_pantheon.bounds, 2048, seed=8)
    want_a, want_b = lk.log_probs_vectorized(th_a), lk.log_probs_vectorized(th_b)
    ta = torch.from_numpy(th_a).cuda()
    side = torch.cuda.Stream()
    for _ in range(10):
        out_a = torch.empty(2048, dtype=torch.float64, device="cuda")
        with torch.cuda.stream(side):
            for _ in range(3):
                lk.engine.eval_device(ta.data_ptr(), 2048, out_a.data_ptr(), gpu.CF_OUT_LOGP, side.cuda_stream)
        got_b = lk.log_probs_vectorized(th_b)  # host path, on the handle's stream, while `side` is still busy
        side.synchronize()
        assert np.array_equal(got_b, want_b)
        assert np.array_equal(out_a.cpu().numpy(), want_a)
    lk.engine.close()


# ---- inverse-GEMM solve: triangular GEMM against the explicit inverse (cf_solve_mode CF_SOLVE_INVERSE_GEMM) ---------
def test_latency_mode_parity_and_speed(gpu, config2):
    import time
    lk_blocked, ref, theta = config2
    if lk_blocked.engine.info()["solve_mode"] != gpu.CF_SOLVE_BLOCKED_TRSM:
        pytest.skip("runs once, beside the blocked-solve instance of the fixture")
    syn = gpu.synthetic.pantheon_like(n_sn=1701, seed=0)
    lk = gpu.sn_pantheon.PantheonLikelihood(syn["z_cmb"], syn["z_hel"], syn["obs"], chol=syn["chol"], latency_mode=True)
    assert lk.engine.info()["pack_probe_rel"] < 1e-12 and lk.engine.info()["solve_mode"] == gpu.CF_SOLVE_INVERSE_GEMM
    # the two kernels agree far inside the parity bar
    np.testing.assert_allclose(lk.chi_squared(theta), lk_blocked.chi_squared(theta), rtol=1e-12)
    full = lk.chi_squared(theta)
    want = ref.chi2(theta)
    rel = np.abs(full - want) / np.abs(want)
    assert rel.max() < RTOL, f"max rel diff {rel.max():.3e}"
    np.testing.assert_allclose(lk.log_probs_vectorized(theta[:300]), ref.logp(theta[:300]), rtol=RTOL)
    for W in (1, 2, 15, 16, 17, 100, 512, 2048):  # batch-size invariance inside the mode: bit-identical
        np.testing.assert_array_equal(lk.chi_squared(theta[:W]), full[:W])
    one = lk.log_probability(theta[7])
    assert isinstance(one, float) and one == pytest.approx(ref.logp(theta[7:8])[0], rel=RTOL)
    # a NaN walker must not leak into its neighbours (the ragged last row block reads K columns past n_pad)
    bad = theta[:40].copy()
    bad[13, 2] = -4.0
    got = lk.chi_squared(bad)
    assert not np.isfinite(got[13])
    np.testing.assert_array_equal(np.delete(got, 13), np.delete(full[:40], 13))

    def wall(fn, arg, reps=20):
        fn(arg)
        t0 = time.perf_counter()
        for _ in range(reps):
            fn(arg)
        return (time.perf_counter() - t0) / reps * 1e6

    lines = []
    for W in (1, 75, 512, 2048, 4096):
        lines.append(f"W={W}: blocked {wall(lk_blocked.log_probs_vectorized, theta[:W]):.0f} us, inverse GEMM {wall(lk.log_probs_vectorized, theta[:W]):.0f} us")
    print("\n".join(lines))
    assert wall(lk.log_probs_vectorized, theta[:1]) < wall(lk_blocked.log_probs_vectorized, theta[:1])
    lk.engine.close()


def test_posterior_means_match_the_oracle_driven_chain_to_sampling_noise(gpu):
    """north_star: 'chi^2 matches to <= 1e-10 (posterior means to sampling noise)'.  A short chain with the reference's
    move mixture (sn/pantheon.py:114-117) on the GPU engine vs the same chain driven by the CPU oracle."""
    torch = pytest.importorskip("torch")
    from oracle import oracle_c, oracle_np as onp

    syn = gpu.synthetic.pantheon_like(n_sn=160, seed=11)
    lk = gpu.sn_pantheon.PantheonLikelihood(syn["z_cmb"], syn["z_hel"], syn["obs"], chol=syn["chol"], latency_mode=True)
    co = oracle_c.COracle(onp.Likelihood(
        ndim=4, z_max=lk.z_max, offset=onp.Slot(0), H0=onp.Slot(1), Om=onp.Slot(2), v=onp.Slot(3),
        z_cmb=syn["z_cmb"], z_hel=syn["z_hel"], obs=syn["obs"], chol=syn["chol"],
        bounds=gpu.sn_pantheon.bounds, gauss=[gpu.sn_pantheon.H0_PRIOR]))
    start = gpu.synthetic.THETA_TRUE + np.array([0.02, 1.0, 0.03, 0.3]) * np.random.default_rng(4).standard_normal((128, 4))
    moves = gpu.ensemble.REFERENCE_MOVES
    e_gpu = gpu.ensemble.ShardedEnsemble(lk.engine.torch_log_prob(), torch.from_numpy(start).to("cuda:0"), seed=5, moves=moves)
    from oracle import moves_torch
    e_cpu = gpu.ensemble.ShardedEnsemble(lambda t: torch.from_numpy(co.logp(t.numpy())), torch.from_numpy(start), seed=5, moves=moves,
                                         moves_impl=moves_torch.TensorMoves(gpu.ensemble.stream_key))
    burn, keep = 60, 120
    chain_g, chain_c = [], []
    for step in range(burn + keep):
        e_gpu.step()
        e_cpu.step()
        if step >= burn:
            chain_g.append(e_gpu.x.cpu().numpy().copy())
            chain_c.append(e_cpu.x.numpy().copy())
    g, c = np.concatenate(chain_g), np.concatenate(chain_c)
    sd = c.std(axis=0)
    # identical seeds + chi^2 agreement at 1e-14: accept/reject decisions essentially never differ
    assert np.all(np.abs(g.mean(axis=0) - c.mean(axis=0)) < 0.05 * sd), (g.mean(axis=0), c.mean(axis=0), sd)
    assert np.all(np.abs(g.std(axis=0) / sd - 1) < 0.05)
    # and the posterior sits on the truth the data were generated from
    assert np.all(np.abs(g.mean(axis=0) - gpu.synthetic.THETA_TRUE) < 4 * sd)
    assert 0.1 < e_gpu.acceptance_fraction() < 0.9
    lk.engine.close()


def test_host_calls_in_place_and_through_copies_agree_bit_for_bit(gpu, tmp_path):
    """cf_eval lets the kernels read theta from / write the results to the pinned staging block in place for batches up to
    CF_ZEROCOPY_MAX walkers (default 16384) and goes through two copy commands above it; the knob is read once per process,
    so the two forms run in two child processes on the same inputs."""
    import subprocess
    import sys

    script = tmp_path / "zc.py"
    script.write_text(
        "import importlib, sys, numpy as np\n"
        f"sys.path.insert(0, {os.path.dirname(os.path.dirname(os.path.abspath(__file__)))!r})\n"
        "amd = importlib.import_module('cosmology-model-fit_amd')\n"
        "syn = amd.synthetic.pantheon_like(n_sn=300, seed=2)\n"
        "lk = amd.sn_pantheon.PantheonLikelihood(syn['z_cmb'], syn['z_hel'], syn['obs'], chol=syn['chol'])\n"
        "th = amd.synthetic.walkers(amd.sn_pantheon.bounds, 1000, seed=4)\n"
        "th[5, 1] = 200.0  # out of the box: -inf\n"
        "out = np.concatenate([lk.log_probs_vectorized(th[:W]) for W in (1, 33, 1000)] + [lk.chi_squared(th[:77])])\n"
        "np.save(sys.argv[1], out)\n")
    outs = []
    for tag, zc in (("copy", "0"), ("inplace", "100000")):
        env = dict(os.environ, CF_ZEROCOPY_MAX=zc)
        r = subprocess.run([sys.executable, str(script), str(tmp_path / (tag + ".npy"))], capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(np.load(tmp_path / (tag + ".npy")))
    assert np.array_equal(outs[0], outs[1], equal_nan=True) and np.isneginf(outs[0][1 + 5])
