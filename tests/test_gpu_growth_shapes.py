"""GPU (-m gpu): growth_kernel (csrc/cosmofit_kernels.hip) and its host tables over the shapes and models the C-ABI accepts -- the
cases of tests/growth_shapes.py -- against the long-double restatement tests/growth_reference.py AT THE SAME effective step count
and a-grid, so the bar is the kernel's arithmetic, not RK4's truncation:

  theory   ``parts["fs8_theory"]`` and ``fs8_theory_at``: 1e-12 relative (float64 on the same scheme: <= 1.1e-14,
           tests/test_growth_shapes_cpu.py; the room is for the device's exp in the wCDM / CPL coefficient and the tree association
           of the 2 x 2 products);
  chi^2    ``parts["chi2_fs8"]``: 1e-10, the bar of every block that reads the distance table; chi_squared = the sum of the
           blocks; log L carries n ln f_err and logl_const; the row outside the box is -inf;
  rounding a request of 257 / 513 / 1025 steps matches the 512 / 1024 / 2048 scheme and misses the one below by more than 1e-10;
  bits     a walker's results inside a 2200-row batch, and a redshift's fs8_theory_at at every request length and position,
           are the same bits;
  H(z)     cf_eval_hz over all eight models and n = 1 .. 1000 against derived_reference.H_of_z: 1e-13.

Every test prints the largest deviation it saw (``-s`` shows them; profiles/NOTES_growth_shape_sweeps.md tabulates them)."""
import numpy as np
import pytest

import derived_reference as R
import growth_reference as G
import growth_shapes as GS
from oracle import oracle_np as onp

pytestmark = pytest.mark.gpu
LD = np.longdouble
THEORY_BAR, CHI2_BAR, HZ_BAR, SUM_BAR = 1e-12, 1e-10, 1e-13, 1e-14


@pytest.fixture(scope="module")
def gpu(pkg):
    if pkg.lib().cf_device_count() < 1:
        pytest.fail("GPU tests need an MI355X; no HIP device visible (there is no fallback path)")
    return pkg


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.int64), np.ascontiguousarray(b, dtype=np.float64).view(np.int64))


def _rel(got, want):
    return float(np.max(np.abs(np.asarray(got).astype(LD) / want - 1)))


def _oracle(b):
    """oracle_np.Likelihood of the blocks that are NOT the growth block (no logl_const: the test adds the growth block's terms)"""
    kw = dict(b["oracle"])
    slots = kw.pop("slots")
    return onp.Likelihood(**kw, **{n: onp.Slot(i) for n, i in slots.items()})


@pytest.mark.parametrize("name", [c.name for c in GS.CASES])
def test_growth_case(gpu, name):
    b = GS.build(gpu, GS.BY_NAME[name])
    c, th, m, f = b["case"], b["theta"], b["model"], b["engine"]["fs8"]
    W, n = th.shape[0], c.n_fs8
    both = np.concatenate([f["z"], b["z_at"]])   # one integration serves the data and the fs8_theory_at requests
    ref = G.theory(m, th, both, a_init=c.a_init, S=c.S, n_agrid=c.a_grid)
    ref_data, ref_at = ref[:, :n], ref[0, n:]
    with gpu.LikelihoodEngine(**b["engine"]) as eng:
        parts = eng.parts(th)
        # ---- theory, at the effective S the header's rule states for the request ----
        dev = _rel(parts["fs8_theory"], ref_data)
        full = eng.fs8_theory_at(th[0], b["z_at"])
        dev_at = _rel(full, ref_at)
        print(f"GROWTH {name} model {c.ez_model} fde {c.fde} C {c.C}: theory {dev:.2e} fs8_theory_at {dev_at:.2e}", end=" ")
        assert dev <= THEORY_BAR and dev_at <= THEORY_BAR, (name, dev, dev_at)
        if c in GS.ROUNDING:
            below = G.theory(m, th, f["z"], a_init=c.a_init, S=c.S // 2, n_agrid=c.a_grid)
            assert _rel(parts["fs8_theory"], below) > 1e-10, name
        # ---- a redshift's bits depend neither on the request's length nor on its place in it ----
        for k in GS.AT_N:
            got = eng.fs8_theory_at(th[0], b["z_at"][:k])
            assert got.shape == (k,) and _same_bits(got, full[:k]), (name, k)
        assert _same_bits(eng.fs8_theory_at(th[0], b["z_at"][::-1]), full[::-1]), name
        assert _same_bits(eng.fs8_theory_at(th[0], f["z"]), parts["fs8_theory"][0]), name
        if c.index == 5:
            alone = np.array([eng.fs8_theory_at(th[0], b["z_at"][k:k + 1])[0] for k in range(130)])
            assert _same_bits(alone, full), name
        for bad in (np.array([0.3, -1e-9]), np.array([np.nextafter(GS.z_edge(c.a_init), np.inf), 0.1]), np.array([np.nan])):
            with pytest.raises(gpu.CosmofitError, match="CF_ERR_INVALID.*a_init <= a <= 1"):
                eng.fs8_theory_at(th[0], bad)
        # ---- chi^2 of the block, the total, log L, the prior ----
        chi2, logl, logp = eng.chi_squared(th), eng.log_likelihood(th), eng.log_probability(th)
        box = b["engine"]["bounds"]
        inside = np.all((box[:, 0] < th) & (th < box[:, 1]), axis=1)
        assert inside[0] and np.all(logp[~inside] == -np.inf) and (W < 3 or not inside[1])
        others = parts["chi2_blocks"].sum(axis=1) + parts["chi2_cc"]
        blocks_sum = others + parts["chi2_fs8"]
        if c.z0_exact:   # q = H D_M / fid = 0 at z = 0: not a number on either side (tests/growth_shapes.py)
            assert not np.isfinite(parts["chi2_fs8"]).any() and not np.isfinite(chi2).any() and np.all(logp == -np.inf)
            print("chi2 not finite (z = 0 datum)")
        else:
            q = G.ap_factor(m, th, f["z"], f["fid"])
            want = G.chi2(m, th, f, S=c.S, q=q)
            dev_c = _rel(parts["chi2_fs8"], want)
            print(f"chi2 {dev_c:.2e}")
            assert dev_c <= CHI2_BAR, (name, dev_c)
            assert _rel(chi2, blocks_sum.astype(LD)) <= SUM_BAR
            olk = _oracle(b)
            with np.errstate(all="ignore"):
                other = np.array([onp.chi_squared(olk, t) for t in th])
                other_ll = np.array([onp.log_likelihood(olk, t) for t in th])
                prior = np.array([onp.log_prior(olk, t) for t in th])
            if c.block == "alone":
                assert np.all(other == 0) and _same_bits(chi2, parts["chi2_fs8"])
            else:
                np.testing.assert_allclose(others, other, rtol=CHI2_BAR)
            terms = G.logl_terms(m, th, n, c.logl_const)
            want_ll = other_ll.astype(LD) - want / 2 + terms
            size = np.abs(other_ll) + np.abs(want / 2) + np.abs(terms)   # the terms' magnitudes: log L may be a difference
            assert np.all(np.abs(logl - want_ll) <= CHI2_BAR * size), name
            assert np.all(np.abs(logp[inside] - (want_ll + prior)[inside]) <= CHI2_BAR * (size + np.abs(prior))[inside]), name
            if c.ferr_free:   # n ln f_err is in log L: left out, some row would miss the bar above a hundred times over
                assert np.max(np.abs(terms - LD(c.logl_const)) / size) > 100 * CHI2_BAR
        # ---- the same rows inside a batch large enough for the throughput kernels: the same bits ----
        big = np.concatenate([th, gpu.synthetic.walkers(box, 2200 - W, seed=c.index)])
        assert _same_bits(eng.chi_squared(big)[:W], chi2), name
        assert _same_bits(eng.parts(big)["fs8_theory"][:W], parts["fs8_theory"]), name


@pytest.mark.parametrize("index", range(8))
def test_hz_kernel_over_models_and_lengths(gpu, index):
    """cf_eval_hz: all eight (ez_model, fde), n around the 256-thread block and z = 0, against derived_reference.H_of_z"""
    b = GS.build(gpu, GS.CASES[index])
    m, th = b["model"], b["theta"][0]
    assert (m.ez_model, m.fde) == GS.PAIRS[index]
    _, cos = R._cosmo(m, th[None])
    worst = 0.0
    with gpu.LikelihoodEngine(**b["engine"]) as eng:
        ref_z = GS.hz_redshifts(1000, b["engine"]["z_max"])
        full = eng.H_z(th, ref_z)
        for n in GS.HZ_N:
            z = GS.hz_redshifts(n, b["engine"]["z_max"])
            assert 0.0 in z
            got = eng.H_z(th, z)
            worst = max(worst, _rel(got, R.H_of_z(m, R._col(cos), z.astype(LD))[0]))
            assert _same_bits(eng.H_z(th, ref_z[:n]), full[:n])   # one thread per redshift: its place does not matter
    print(f"HZ model {m.ez_model} fde {m.fde}: {worst:.2e}")
    assert worst <= HZ_BAR
