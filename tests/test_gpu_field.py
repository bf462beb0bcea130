"""GPU (-m gpu): ``quintessence`` as a user calls it -- ``reconstruct`` and ``bands`` on a synthetic thawing chain, on the tensor an
ensemble hands out, and the example.  The bands must be ``np.percentile`` / corner's weighted quantile of ``reconstruct``'s own
columns to the bit (what ``derived.bands`` promises of its curves), whatever max_bytes; rows without a field are dropped and
counted."""
import os
import runpy
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, golden

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
QS = np.array([0.159, 0.5, 0.841])


@pytest.fixture(scope="module")
def Q(pkg):
    if pkg.lib().cf_device_count() < 1:
        pytest.fail("GPU tests need an MI355X; no HIP device visible (there is no fallback path)")
    return pkg.quintessence


@pytest.fixture(scope="module")
def chain():
    """3000 rows around field.py's triple, three of them without a field: a NaN, a negative Om, H0 = 0."""
    rng = np.random.default_rng(21)
    x = np.array([66.53, 0.312, -0.763]) + np.array([0.6, 0.008, 0.06]) * rng.standard_normal((3000, 3))
    x[:, 2] = np.maximum(x[:, 2], -0.999)
    x[17, 1], x[1500, 1], x[2999, 0] = np.nan, -5.0, 0.0
    return torch.from_numpy(x).to(DEV)


@pytest.fixture(scope="module")
def model(Q):
    return Q.Model(columns={"H0": 0, "Om": 1, "w0": 2}, n_a=257)


def _corner_quantile(x, q, w):
    """corner.quantile(x, q, weights=w), written out (corner/core.py: quantile)."""
    idx = np.argsort(x, kind="stable")
    sw = w[idx]
    cdf = np.cumsum(sw)[:-1]
    cdf /= cdf[-1]
    return np.interp(q, np.append(0, cdf), x[idx])


def test_reconstruct_on_a_chain(Q, model, chain):
    a = np.array([0.25, 0.5, 1.0, 2.0])
    res = Q.reconstruct(model, chain, a=a, phi=50, t=[1.0, 5.0, 13.0])
    assert all(v.is_cuda for v in res.values())
    assert res["status"].dtype == torch.int32 and res["phi_a"].dtype == torch.float64
    assert res["phi_a"].shape == (3000, 4) and res["a_phi"].shape == (3000, 50) and res["phi_grid"].shape == (3000, 50)
    assert res["a_t"].shape == (3000, 3) and res["t_grid"].shape == (3,) and res["t_today"].shape == (3000,)
    st = res["status"].cpu().numpy()
    assert st[[17, 1500, 2999]].tolist() == [2, 2, 2] and st.sum() == 6
    ok = st == 0
    t0, phi0 = res["t_today"].cpu().numpy(), res["phi_today"].cpu().numpy()
    assert np.isnan(t0[~ok]).all() and (np.abs(t0[ok] - 13.7) < 1.0).all() and (phi0[ok] > 0).all()
    assert torch.equal(res["phi_a"][:, 2][torch.from_numpy(ok).to(DEV)], res["phi_today"][torch.from_numpy(ok).to(DEV)])  # a = 1 is today
    w_a = res["w_a"].cpu().numpy()[ok]
    assert (np.diff(w_a, axis=1) > 0).all() and (w_a > -1).all()  # thawing: w leaves -1
    np.testing.assert_allclose((res["K_a"] + res["V_a"]).cpu().numpy()[ok, 2], 4 / 2.0**2, rtol=1e-13)  # rho_de(1) = 4 / D^2, D = 2
    a_t = res["a_t"].cpu().numpy()[ok]
    assert (np.diff(a_t, axis=1) > 0).all() and (np.abs(a_t[:, 2] - 1) < 0.1).all()
    # a strided view and an empty chain
    np.testing.assert_array_equal(Q.reconstruct(model, chain[::3], a=a)["V_a"].cpu().numpy(), res["V_a"][::3].cpu().numpy())  # NaN rows too
    empty = Q.reconstruct(model, chain[:0], a=a, phi=5)
    assert empty["V_a"].shape == (0, 4) and empty["status"].shape == (0,) and empty["phi_grid"].shape == (0, 5)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("quantity,x", [("V_phi", np.linspace(0.0, 0.008, 9)), ("a_t", np.linspace(0.5, 20.0, 7)),
                                        ("phi_a", np.array([0.1, 1.0, 3.0])), ("t_today", None), ("phi_today", None)])
def test_bands_are_numpy_quantiles_of_reconstruct_s_columns(Q, model, chain, quantity, x, weighted):
    w = None
    if weighted:
        w = torch.from_numpy(np.random.default_rng(5).uniform(0.0, 1.0, 3000)).to(DEV)
    band = Q.bands(model, chain, quantity, x, q=QS, weights=w)
    assert (band["n_used"], band["n_phantom"], band["n_invalid"]) == (2997, 0, 3)
    kind = Q.QUANTITIES[quantity]
    res = Q.reconstruct(model, chain, **({kind: x} if kind else {}))
    ok = (res["status"] == 0).cpu().numpy()
    cols = res[quantity].cpu().numpy()[ok]
    cols = cols[:, None] if cols.ndim == 1 else cols
    assert band["bands"].shape == (3, cols.shape[1]) and np.isfinite(band["bands"]).all()
    if w is None:
        np.testing.assert_array_equal(band["bands"], np.percentile(cols, list(100.0 * QS), axis=0))
        np.testing.assert_allclose(band["mean"], cols.mean(axis=0), rtol=1e-13)
        np.testing.assert_allclose(band["std"], cols.std(axis=0), rtol=1e-9)
    else:
        wn = w.cpu().numpy()[ok]
        want = np.stack([_corner_quantile(cols[:, j], QS, wn) for j in range(cols.shape[1])], axis=1)
        np.testing.assert_array_equal(band["bands"], want)
        np.testing.assert_allclose(band["mean"], (wn[:, None] * cols).sum(axis=0) / wn.sum(), rtol=1e-13)
    if x is not None:  # the chunking changes nothing: one column per chunk, and a few
        for max_bytes in (1, 4 * 8 * 2997 * 2):
            again = Q.bands(model, chain, quantity, x, q=QS, weights=w, max_bytes=max_bytes)
            for k in ("bands", "mean", "std"):
                np.testing.assert_array_equal(again[k], band[k])


def test_bands_count_phantom_rows_and_refuse_a_chain_without_a_field(Q, chain):
    m = Q.Model(fde="wcdm", columns={"H0": 0, "Om": 1, "w0": 2}, n_a=64)
    x = chain[:200].clone()
    x[5:9, 2] = -1.1
    band = Q.bands(m, x, "t_a", [0.5, 1.0])
    assert (band["n_used"], band["n_phantom"], band["n_invalid"]) == (195, 4, 1)
    keep = torch.ones(200, dtype=torch.bool, device=DEV)
    keep[5:9], keep[17] = False, False
    np.testing.assert_array_equal(band["bands"], Q.bands(m, x[keep], "t_a", [0.5, 1.0])["bands"])
    with pytest.raises(ValueError, match="no row"):
        Q.bands(m, x[5:9], "t_a", [1.0])


def test_samples_straight_from_an_ensemble(pkg, Q):
    g = golden("bao_desi")
    lk = pkg.likelihoods.DesiBao(g["bao_z"], g["bao_val"], g["bao_qty"], g["bao_inv_cov"])  # theta = (h, Om, w0), thawing
    try:
        start = np.array([0.68, 0.31, -0.85]) + np.array([0.01, 0.01, 0.05]) * np.random.default_rng(1).standard_normal((32, 3))
        ens = pkg.ensemble.ShardedEnsemble(lk.engine.torch_log_prob(), torch.from_numpy(start).to(DEV), seed=7)
        ens.run_mcmc(12)
        flat = ens.get_chain(discard=2, flat=True)
        assert flat.is_cuda and flat.shape == (320, 3)
        m = Q.Model.from_recipe("bao/desi_fs_lya.py", n_a=257)  # the same theta: h with a scale of 100
        res = Q.reconstruct(m, flat, t=[13.0])
        ok = (res["status"] == 0).cpu().numpy()
        np.testing.assert_array_equal(res["hubble_time"].cpu().numpy()[ok], (9.77813 / (100.0 * flat[:, 0].cpu().numpy() / 100))[ok])
        band = Q.bands(m, flat, "t_today")
        assert band["n_used"] == int(ok.sum()) > 300
        np.testing.assert_array_equal(band["bands"][:, 0], np.percentile(res["t_today"].cpu().numpy()[ok], list(100.0 * QS)))
    finally:
        lk.engine.close()


def test_the_example_runs_to_its_npz(Q, tmp_path, monkeypatch, capsys):
    out = tmp_path / "band.npz"
    monkeypatch.setattr(sys, "argv", ["quintessence_band.py", "--samples", "400", "--out", str(out)])
    runpy.run_path(os.path.join(ROOT, "examples", "quintessence_band.py"), run_name="__main__")
    z = np.load(out)
    assert z["V_bands"].shape == (3, 2000) and z["a_bands"].shape == (3, 1000) and z["age_bands"].shape == (3,)
    assert int(z["n_used"]) == 400 and 13.0 < z["age_bands"][1] < 14.5
    assert (z["V_bands"][0] <= z["V_bands"][2]).all() and (np.diff(z["a_bands"][1]) > 0).all()
    assert "age of the universe" in capsys.readouterr().out
