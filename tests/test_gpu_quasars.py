"""GPU (-m gpu): the quasar Hubble-diagram likelihoods (quasars.py, csrc/cosmofit_quasar.hip) on an MI355X.

* Every fixture of tests/golden/generate_quasars.py -- the five scripts and qsr_union3 on the unbinned catalogue -- through
  quasars.build at rtol 1e-10: CF_OUT_CHI2 / LOGL / LOGP and the per-block accessor (chi^2 per block, mu, BAO theory).
* The same rows give the same bits in batches of 1, 3, 20, 257, 4096 and 65536, through host buffers and cf_eval_device,
  and on a second handle.
* Posterior: the device ensemble (stretch move, as emcee runs these scripts) on the real-data scripts qsr_union3 and qsr_desi
  against the "Flat wzCDM" block of their docstrings.
"""
import numpy as np
import pytest
import torch

import quasar_reference as ref
from conftest import golden, synthetic_cov

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def qpkg(pkg):
    if pkg.lib().cf_device_count() < 1:
        pytest.fail("GPU tests need an MI355X; no HIP device visible (there is no fallback path)")
    return pkg


def _build(pkg, name):
    g = dict(golden(name))
    qsr, sn, bao = ref.fixture_data(g, synthetic_cov)
    return g, pkg.quasars.build(ref.SCRIPTS[name], qsr=qsr, sn=sn, bao=bao)


def _check(got, want, rtol=1e-10):
    got, want = np.asarray(got, float), np.asarray(want, float)
    fin = np.isfinite(want)
    np.testing.assert_allclose(got[fin], want[fin], rtol=rtol, atol=0)


@pytest.mark.parametrize("name", ref.CASES)
def test_case_matches_the_reference(qpkg, name):
    g, lk = _build(qpkg, name)
    th = g["thetas"]
    logp = lk.log_probability(th)
    out = ~np.isfinite(g["logp"])
    assert np.all(logp[out] == -np.inf), "outside the box log P is -inf, exactly"
    _check(logp, g["logp"])
    _check(lk.log_likelihood(th), g["logl"])
    _check(lk.chi_squared(th), g["chi2_parts"].sum(axis=1))
    _check(lk.chi2_parts(th), g["chi2_parts"])
    rows = g["theory_rows"]
    t = lk.theory(th[rows])
    _check(t["mu_qsr"], g["mu_qsr"])
    if "mu_sn" in g:
        _check(t["mu_sn"], g["mu_sn"])
    if "bao_theory" in g:
        _check(t["bao_theory"], g["bao_theory"])
    lk.close()


@pytest.mark.parametrize("name", ["qsr_pantheon", "qsr_desi", "qsr_des5y_desi"])
def test_bits_do_not_depend_on_the_batch(qpkg, name):
    g, lk = _build(qpkg, name)
    _, lk2 = _build(qpkg, name)
    rng = np.random.default_rng(7)
    b = g["bounds"]
    big = rng.uniform(b[:, 0], b[:, 1], size=(65536, len(b)))
    big[:len(g["thetas"])] = g["thetas"]
    for kind in (qpkg.CF_OUT_CHI2, qpkg.CF_OUT_LOGL, qpkg.CF_OUT_LOGP):
        full = lk.engine._eval(big, kind)
        for W in (1, 3, 20, 257, 4096):
            np.testing.assert_array_equal(lk.engine._eval(big[:W], kind), full[:W])
        np.testing.assert_array_equal(lk2.engine._eval(big[:4096], kind), full[:4096])
        f = lk.engine.torch_log_prob(kind)
        for W in (1, 3, 20, 257, 4096, 65536):
            d = f(torch.from_numpy(big[:W]).to(DEV))
            torch.cuda.synchronize()
            np.testing.assert_array_equal(d.cpu().numpy(), full[:W])
    lk.close()
    lk2.close()


# "Flat wzCDM" block of the docstrings: (median, +, -) per parameter
WZCDM = {
    "qsr_union3": [(-0.101, 0.091, 0.093), (0.391, 0.076, 0.059), (-0.064, 0.089, 0.089), (0.350, 0.046, 0.047),
                   (-0.893, 0.178, 0.209)],
    "qsr_desi": [(-0.125, 0.102, 0.104), (0.405, 0.077, 0.059), (139.974, 3.648, 3.422), (0.312, 0.013, 0.013),
                 (-0.787, 0.145, 0.153)],
}


@pytest.mark.parametrize("name", ["qsr_union3", "qsr_desi"])
def test_device_ensemble_reproduces_the_published_posterior(qpkg, name):
    from importlib import import_module

    ens_mod = import_module(qpkg.__name__ + ".ensemble")
    g, lk = _build(qpkg, name)
    b = g["bounds"]
    start = np.random.default_rng(3).uniform(b[:, 0], b[:, 1], size=(512, len(b)))  # as the scripts start (uniform in the box)
    ens = ens_mod.ShardedEnsemble(lk.engine.torch_log_prob(), torch.from_numpy(start).to(DEV), seed=2024,
                                  moves=ens_mod.STRETCH_ONLY)
    ens.run_mcmc(3000)
    q = ens.percentile([16, 50, 84], discard=1000).cpu().numpy()
    for k, (med, up, lo) in enumerate(WZCDM[name]):
        sigma = 0.5 * (up + lo)
        assert abs(q[1, k] - med) < 0.1 * sigma, (name, k, q[:, k], med, sigma)
        width = q[2, k] - q[0, k]
        assert abs(width / (up + lo) - 1) < 0.10, (name, k, width, up + lo)
    lk.close()
