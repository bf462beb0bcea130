"""GPU (-m gpu): qsr_walker_kernel (csrc/cosmofit_quasar.hip) at the shapes its C entry point accepts, against the long-double
run of the numpy restatement (tests/quasar_reference.py), cast to float64 at the end.

The cases come from tests/quasar_shapes.py: grids of 16 .. 8192 nodes around the 256-thread chunking of the table build, 1 ..
65536 quasars, 0 .. 700 SNe on a grid of their own or on the quasars', 0 .. 64 BAO data with distinct, equal and paired
redshifts, H0 free or fixed, one slot fixed or scaled, qsr_z_top at, below and above max z, redshifts on nodes, both solves.
tests/test_quasar_shapes_cpu.py proves on the same seeds that the reference is finite on every compared row, that float64
and long double agree to 1e-12 there (so that 1e-10 is no coin toss), and that every list is reached.

The bars: rtol 1e-10 (the project's parity bar) on chi^2 per block, chi^2, mu and the BAO predictions wherever the reference
is finite; log L and log P within 1e-10 x (|chi2_total| + |sum ln(sigma^2 + s^2)|), both from the reference -- log L is half
the sum of those two and the second can be negative, so a plain relative bar would be ill-conditioned on some draws.
CF_TEST_RANDOM_SHAPES=<n> runs more (or fewer) seeds.
"""
import os

import numpy as np
import pytest
import torch

import quasar_shapes as qs

pytestmark = pytest.mark.gpu
RTOL = 1e-10
DEV = torch.device("cuda:0")
LD = np.longdouble


@pytest.fixture(scope="module")
def gpu(pkg):
    if pkg.lib().cf_device_count() < 1:
        pytest.fail("GPU tests need an MI355X; no HIP device visible (there is no fallback path)")
    return pkg


def _close(got, want, what, case):
    """rtol on the finite entries of the reference; prints and returns the largest relative error."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    fin = np.isfinite(want)
    err, size = np.abs(got[fin] - want[fin]), np.abs(want[fin])
    assert np.all(np.isfinite(got[fin])), f"{what}: not finite where the reference is; {qs.describe(case)}"
    assert np.all(err[size == 0] == 0), f"{what}: an absent block's value is 0; {qs.describe(case)}"
    worst = float(np.max(err[size > 0] / size[size > 0])) if np.any(size > 0) else 0.0
    print(f"  {what}: max rel {worst:.2e} over {int(fin.sum())} entries")
    np.testing.assert_allclose(got[fin], want[fin], rtol=RTOL, atol=0, err_msg=f"{what}; {qs.describe(case)}")
    return worst


def _close_logl(got, want, scale, what, case):
    got = np.asarray(got, dtype=np.float64)
    fin = np.isfinite(want)
    assert np.all(np.isfinite(got[fin])), f"{what}: not finite where the reference is; {qs.describe(case)}"
    err = np.abs(got[fin] - want[fin]) / scale[fin]
    worst = float(np.max(err)) if fin.any() else 0.0
    print(f"  {what}: max scaled error {worst:.2e} over {int(fin.sum())} rows")
    assert np.all(err <= RTOL), f"{what}: {worst:.3e}; {qs.describe(case)}"
    return worst


def _run_case(gpu, c):
    assert np.finfo(LD).eps < 1e-18, "the judge must be an extended type, not float64 judging float64"
    print(qs.describe(c))
    want = qs.reference(c, LD)
    eng = gpu.LikelihoodEngine(**qs.engine_kwargs(c, gpu.Param, gpu.engine.solve_mode_of(c["solve"])))
    theta, W = c["theta"], c["W"]
    worst = 0.0
    try:
        parts = eng.quasar_parts(theta)
        worst = max(worst, _close(parts["chi2_blocks"], want["chi2_parts"], "chi2_parts", c))
        for k, block in enumerate(("sn", "quasars", "bao")):
            _close(parts["chi2_blocks"][:, k], want["chi2_parts"][:, k], "chi2 " + block, c)
        worst = max(worst, _close(parts["mu_qsr"], want["mu_qsr"], "mu_qsr", c))
        assert (parts["mu_sn"] is None) == (want["mu_sn"] is None) and (parts["bao_theory"] is None) == (want["bao_theory"] is None)
        if want["mu_sn"] is not None:
            worst = max(worst, _close(parts["mu_sn"], want["mu_sn"], "mu_sn", c))
        if want["bao_theory"] is not None:
            worst = max(worst, _close(parts["bao_theory"], want["bao_theory"], "bao_theory", c))
        chi2, logl, logp = eng.chi_squared(theta), eng.log_likelihood(theta), eng.log_probability(theta)
        worst = max(worst, _close(chi2, want["chi2"], "chi_squared", c))
        scale = qs.logl_scale(want)
        worst = max(worst, _close_logl(logl, want["logl"], scale, "log_likelihood", c))
        worst = max(worst, _close_logl(logp, want["logp"], scale, "log_probability", c))
        out = want["logp"] == -np.inf
        assert np.array_equal(logp == -np.inf, out), f"outside the box log P is -inf, exactly, and nowhere else; {qs.describe(c)}"
        assert not np.any(np.isnan(logp))
        if c["row_out"] is not None:
            assert out[c["row_out"]] and np.isfinite(logl[c["row_out"]])
        # the same rows inside a large batch, then after a batch of NaN rows in a batch that ends inside a 16-walker panel
        host = {gpu.CF_OUT_CHI2: chi2, gpu.CF_OUT_LOGL: logl, gpu.CF_OUT_LOGP: logp}
        big = np.concatenate([theta, qs.filler(c, 2200 - W, c["seed"])])
        for kind, first in host.items():
            np.testing.assert_array_equal(eng._eval(big, kind)[:W], first, err_msg=f"kind {kind} in a 2200-row batch; {qs.describe(c)}")
        eng.chi_squared(qs.nan_rows(c, 2200, c["seed"]))  # leaves NaN residual rows behind in the workspace
        ragged = np.resize(theta, (37, theta.shape[1]))
        n = min(W, 37)
        for kind, first in host.items():
            np.testing.assert_array_equal(eng._eval(ragged, kind)[:n], first[:n],
                                          err_msg=f"kind {kind} in a 37-row batch after NaN rows; {qs.describe(c)}")
        # device buffers on torch's stream: the host path's bits
        dth = torch.from_numpy(theta).to(DEV)
        for kind, first in host.items():
            d = eng.torch_log_prob(kind)(dth)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(d.cpu().numpy(), first, err_msg=f"kind {kind} through torch_log_prob; {qs.describe(c)}")
    finally:
        eng.close()
    print(f"  worst of the case: {worst:.2e}")


# the two largest tables first and alone: 64 KiB of dynamic LDS with one grid, 128 KiB with an SN grid of its own
@pytest.mark.parametrize("name", sorted(qs.FIXED_CASES))
def test_largest_grid(gpu, name):
    c = qs.fixed_case(name)
    assert c["n_grid"] == 8192 and (c["sn_z_top"] > 0) == (name == "two_grids_8192")
    _run_case(gpu, c)


# CF_TEST_RANDOM_SHAPES=<n>: soak with more seeds (the default 24 walk every list once)
@pytest.mark.parametrize("seed", range(int(os.environ.get("CF_TEST_RANDOM_SHAPES", "24"))))
def test_quasar_shape(gpu, seed):
    _run_case(gpu, qs.build_case(seed))
