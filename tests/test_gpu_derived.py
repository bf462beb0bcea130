"""GPU (-m gpu): ``derived`` as a user calls it -- ``columns`` / ``augment`` on a device chain, the ensemble's ``get_blobs``, the
nested sampler's derived marginals, the mirrors' ``derived`` and the posterior-predictive ``bands``.  The kernels themselves are
judged in tests/test_gpu_derived_kernels.py; here the plumbing must hand their bits through unchanged and the reductions must be
numpy's / corner's, exactly."""
import numpy as np
import pytest
import torch

import derived_shapes as DS
from conftest import golden

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def D(pkg):
    if pkg.lib().cf_device_count() < 1:
        pytest.fail("GPU tests need an MI355X; no HIP device visible (there is no fallback path)")
    return pkg.derived


@pytest.fixture(scope="module")
def desi_cmb(pkg, D):
    eng = pkg.LikelihoodEngine(**DS.engine_kwargs(pkg, "desi_cmb_thawing"))
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def union3(pkg, D):
    g = golden("bao_desi_cmb_union3_fs8")
    lk = pkg.likelihoods.DesiCmbUnion3Fs8(g["z_cmb"], g["z_hel"], g["obs"], g["cov_sn"], g["bao_z"], g["bao_val"], g["bao_qty"],
                                          g["bao_inv_cov"], g["fs8_z"], g["fs8_val"], g["fs8_cov"], g["fs8_fid"])
    yield lk
    lk.engine.close()


def _corner_quantile(x, q, w):
    """corner.quantile(x, q, weights=w), written out (corner/core.py: quantile)."""
    idx = np.argsort(x, kind="stable")
    sw = w[idx]
    cdf = np.cumsum(sw)[:-1]
    cdf /= cdf[-1]
    return np.interp(q, np.append(0, cdf), x[idx])


@pytest.mark.parametrize("case", DS.CASES)
def test_columns_reproduce_the_fixture(pkg, D, case):
    eng = pkg.LikelihoodEngine(**DS.engine_kwargs(pkg, case))
    try:
        spec = D.Spec(eng, DS.COLUMNS[case], **DS.consts(pkg, case))
        x = torch.from_numpy(DS.thetas(case)).to(DEV)
        got = D.columns(spec, x)
        assert got.is_cuda and got.shape == (x.shape[0], spec.n_q)
        got, want = got.cpu().numpy(), DS.expected(case)
        for j, name in enumerate(spec.names):
            if name in DS.ZERO_CROSSING or name == "wa":
                assert np.max(np.abs(got[:, j] - want[:, j])) <= 1e-12, (case, name)
            else:
                assert np.max(np.abs(got[:, j] / want[:, j] - 1)) <= 1e-10, (case, name)
        assert D.columns(spec, x[:0]).shape == (0, spec.n_q)
    finally:
        eng.close()


def test_at_z_names_are_columns_of_the_curves_and_augment_feeds_marginals(pkg, D, desi_cmb):
    x = torch.from_numpy(DS.thetas("desi_cmb_thawing")).to(DEV)
    names = ["Om", "DV_rd@0.51", "H@0.51", "rd", "DM@2.33", "DV_rd@1.3", "mu@0.1", "lA"]
    spec = D.Spec(desi_cmb, names, **DS.consts(pkg, "desi_cmb_thawing"))
    cols = D.columns(spec, x)
    dv = D.curves(spec, x, [1.3, 0.51], "DV_rd")
    assert torch.equal(cols[:, 1], dv[:, 1]) and torch.equal(cols[:, 5], dv[:, 0])
    assert torch.equal(cols[:, 2], D.curves(desi_cmb, x, [0.51], "H")[:, 0])
    assert torch.equal(cols[:, 4], D.curves(desi_cmb, x, [2.33], "DM")[:, 0])
    assert torch.equal(cols[:, 6], D.curves(desi_cmb, x, [0.1], "mu")[:, 0])
    assert torch.equal(cols[:, [0, 3, 7]], D.columns(D.Spec(desi_cmb, ["Om", "rd", "lA"]), x))
    aug = D.augment(spec, x)
    assert aug.shape == (300, 4 + 8) and torch.equal(aug[:, :4], x) and torch.equal(aug[:, 4:], cols)
    cd = pkg.marginals.corner_data(aug, bins=20)
    assert cd["h1"].shape == (12, 20) and cd["quantiles"].shape == (3, 12)
    np.testing.assert_array_equal(cd["quantiles"], np.percentile(aug.cpu().numpy(), list(100.0 * np.array([0.159, 0.5, 0.841])), axis=0))
    np.testing.assert_array_equal(pkg.chain_stats.percentile(aug, [15.9, 50, 84.1]).cpu().numpy(),
                                  np.percentile(aug.cpu().numpy(), [15.9, 50, 84.1], axis=0))
    # a strided view of a longer chain is the same as its contiguous copy
    assert torch.equal(D.columns(spec, x[::3]), cols[::3])
    big = D.curves(desi_cmb, x[:3], np.linspace(0, 2.4, 5000), "DM")  # more redshifts than one launch takes
    assert torch.equal(big[:, 4096:], D.curves(desi_cmb, x[:3], np.linspace(0, 2.4, 5000)[4096:], "DM"))


def test_get_blobs_equals_columns_of_get_chain(pkg, D, union3):
    E = pkg.ensemble
    spec = D.Spec(union3.engine, ["omh2", "Om", "S8", "rd", "q0", "j0", "theta_star100", "z_star"], comp=pkg.cmb_data.PLANCK_ACT)
    rng = np.random.default_rng(2)
    start = np.array([0.0, 67.5, 0.0224, 0.119, 0.0, 0.8]) + np.array([0.02, 0.5, 1e-4, 1e-3, 0.3, 0.02]) * rng.standard_normal((32, 6))
    ens = E.ShardedEnsemble(union3.engine.torch_log_prob(kind=pkg.CF_OUT_LOGL), torch.from_numpy(start).to(DEV), seed=3, blobs=spec)
    with pytest.raises(AttributeError, match="run_mcmc"):
        ens.get_blobs()
    ens.run_mcmc(20)
    blobs = ens.get_blobs(discard=3, thin=2)
    chain = ens.get_chain(discard=3, thin=2)
    assert chain.shape == (8, 32, 6) and blobs.shape == (8, 32, 8) and blobs.is_cuda
    assert torch.equal(blobs, D.columns(spec, chain.reshape(-1, 6)).reshape(8, 32, 8))
    flat = ens.get_blobs(discard=3, thin=2, flat=True)
    assert torch.equal(flat, D.columns(spec, ens.get_chain(discard=3, thin=2, flat=True))) and flat.shape == (256, 8)
    assert torch.equal(ens.get_blobs()[3 + 2 - 1:: 2], blobs) and ens.get_blobs().shape == (20, 32, 8)
    assert bool(torch.isfinite(blobs).all())
    plain = E.ShardedEnsemble(union3.engine.torch_log_prob(kind=pkg.CF_OUT_LOGL), torch.from_numpy(start).to(DEV), seed=3)
    plain.run_mcmc(20)  # the blobs change nothing of the chain
    assert torch.equal(plain.get_chain(), ens.get_chain())
    with pytest.raises(AttributeError, match="blobs="):
        plain.get_blobs()


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("quantity", ["DV_rd", "H", "mu"])
def test_bands_are_numpy_percentiles_of_the_curves(pkg, D, desi_cmb, weighted, quantity):
    rng = np.random.default_rng(7)
    base = DS.thetas("desi_cmb_thawing")
    x = torch.from_numpy(base[rng.integers(0, 300, 5000)] * (1 + 1e-3 * rng.standard_normal((5000, 4)))).to(DEV)
    w = torch.from_numpy(rng.uniform(0, 1, 5000) ** 3).to(DEV) if weighted else None
    z = np.linspace(0.01, 2.33, 200)
    q = (0.159, 0.5, 0.841)
    got = D.bands(desi_cmb, x, z, quantity, q=q, weights=w)
    curve = D.curves(desi_cmb, x, z, quantity).cpu().numpy()
    assert got["bands"].shape == (3, 200) and np.array_equal(got["z"], z) and np.array_equal(got["q"], np.array(q))
    if weighted:
        wh = w.cpu().numpy()
        want = np.stack([_corner_quantile(curve[:, j], np.array(q), wh) for j in range(200)], axis=1)
        mean = (wh[:, None] * curve).sum(0) / wh.sum()
    else:
        want = np.stack([np.percentile(curve[:, j], list(100.0 * np.array(q))) for j in range(200)], axis=1)
        mean = curve.mean(0)
    assert np.array_equal(got["bands"], want), float(np.max(np.abs(got["bands"] / want - 1)))
    np.testing.assert_allclose(got["mean"], mean, rtol=1e-12)
    assert (got["bands"][0] <= got["bands"][1]).all() and (got["bands"][1] <= got["bands"][2]).all() and (got["std"] > 0).all()
    small = D.bands(desi_cmb, x, z, quantity, q=q, weights=w, max_bytes=D._BAND_BUFFERS * 8 * 5000 * 7)  # 7 redshifts per chunk
    for key in ("bands", "mean", "std"):
        assert np.array_equal(small[key], got[key]), key


def test_nested_marginals_take_derived_columns(pkg, D, desi_cmb):
    nested = pkg.nested
    mu = torch.tensor([67.5, 0.0222, 0.119, -0.8], dtype=torch.float64, device=DEV)
    sd = torch.tensor([1.0, 2e-4, 2e-3, 0.05], dtype=torch.float64, device=DEV)
    p = nested.Prior()
    for name, lo_hi in zip(("H0", "wb", "wc", "w0"), ((60.0, 75.0), (0.021, 0.0235), (0.10, 0.14), (-1.0, -0.5))):
        p.add_parameter(name, dist=lo_hi)
    s = nested.DeviceNestedSampler(p, lambda th: -0.5 * (((th - mu) / sd) ** 2).sum(1), n_live=300, seed=5)
    assert s.run() is True
    spec = D.Spec(desi_cmb, ["Om", "rd", "z_star"])
    cols, w = s.posterior_derived(spec)
    pts, log_w, _ = s.posterior()
    assert cols.shape == (len(pts), 3) and torch.equal(cols, D.columns(spec, torch.from_numpy(pts).to(DEV)))
    np.testing.assert_array_equal(w.cpu().numpy(), np.exp(log_w))
    got = s.marginals(derived=spec, bins=20)
    want = pkg.marginals.corner_data(torch.cat([torch.from_numpy(pts).to(DEV), cols], dim=1), weights=w, bins=20)
    assert got["h1"].shape == (7, 20) and set(got) == set(want)
    for key in got:
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    plain = s.marginals(bins=20)
    np.testing.assert_array_equal(plain["h1"], got["h1"][:4])


def test_mirrors_derive_on_the_host_path(pkg, D):
    th = DS.thetas("cmb_cmb")[:10]
    lk = pkg.likelihoods.CmbOnly()
    try:
        names = ["theta_star100", "rs_star", "DM_star", "z_star", "omh2", "Om", "z_drag", "r_drag", "z_eq"]
        got = lk.derived(th, names)
        assert got.shape == (10, 9) and lk.derived(th[0], names).shape == (9,)
        blobs = lk.blobs(th)
        got[:, 2] /= 1000
        np.testing.assert_allclose(got[:, :4], blobs, rtol=1e-12)
        np.testing.assert_allclose(got[:, 4:], DS.expected("cmb_cmb")[:10, :5], rtol=1e-10)
        with pytest.raises(ValueError, match="^S8 needs"):
            lk.derived(th, ["S8"])
    finally:
        lk.engine.close()
