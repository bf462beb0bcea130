"""GPU: cf_create's descriptor refusals between two working engines, and cf_qsr_eval_parts' own refusals.

The refusals return before anything is allocated; an engine created behind them must compute what the one before them did."""
import ctypes as C

import numpy as np
import pytest

import create_refusals
import quasar_shapes as qs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(pkg):
    if pkg.lib().cf_device_count() < 1:
        pytest.fail("GPU tests need an MI355X; no HIP device visible (there is no fallback path)")
    return pkg


def _tiny_sn_engine(gpu, syn):
    return gpu.LikelihoodEngine(ndim=2, z_max=syn["z_max"], n_grid=64, params=dict(offset=gpu.Param(fixed=-19.3), H0=gpu.Param(0), Om=gpu.Param(1)),
                                sn=dict(z_cmb=syn["z_cmb"], z_hel=syn["z_hel"], obs=syn["obs"], chol=syn["chol"]),
                                bounds=[[60.0, 80.0], [0.1, 0.6]])


def test_refusals_leave_the_next_engine_its_bits(gpu):
    syn = gpu.synthetic.pantheon_like(n_sn=16, seed=3)
    theta = gpu.synthetic.walkers([[60.0, 80.0], [0.1, 0.6]], 33, seed=7)
    first = _tiny_sn_engine(gpu, syn)
    try:
        want = first.chi_squared(theta).copy()
    finally:
        first.close()
    assert want.shape == (33,) and np.all(np.isfinite(want)) and np.all(want > 0)
    create_refusals.check(gpu)
    second = _tiny_sn_engine(gpu, syn)
    try:
        got = second.chi_squared(theta)
    finally:
        second.close()
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


def _parts_error(gpu, eng, W, mu_sn=None):
    theta = np.zeros((max(W, 1), eng.ndim))
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    with pytest.raises(gpu.CosmofitError) as err:
        gpu._lib.check(gpu.lib().cf_qsr_eval_parts(eng._h, p(theta), W, None, p(mu_sn), None, None))
    assert err.value.code == -1
    return str(err.value)


def test_qsr_eval_parts_refusals(gpu):
    syn = gpu.synthetic.pantheon_like(n_sn=16, seed=3)
    plain = _tiny_sn_engine(gpu, syn)
    try:
        assert _parts_error(gpu, plain, 1) == "CF_ERR_INVALID: cf_qsr_eval_parts: not a quasar handle (cf_create_quasar)"
    finally:
        plain.close()
    case = qs.build_case(0)  # the smallest of the sweep: 16 nodes, one quasar, no SN and no BAO block
    assert case["n_grid"] == min(qs.N_GRID) and case["n_qsr"] == min(qs.N_QSR) and case["sn"] is None and case["bao"] is None
    eng = gpu.LikelihoodEngine(**qs.engine_kwargs(case, gpu.Param, gpu.engine.solve_mode_of("auto")))
    try:
        assert _parts_error(gpu, eng, 1, mu_sn=np.empty((1, 1))) == "CF_ERR_INVALID: cf_qsr_eval_parts: this likelihood has no SN block"
        assert _parts_error(gpu, eng, 0) == "CF_ERR_INVALID: cf_qsr_eval_parts: W out of range"
        parts = eng.quasar_parts(case["theta"])  # and the handle still evaluates
        assert np.all(np.isfinite(parts["chi2_blocks"])) and np.all(parts["chi2_blocks"][:, 0] == 0)
    finally:
        eng.close()
