"""CPU: the conditions that keep the GPU shape sweeps honest, proved without a GPU on the same seeds and the same builders.

Quasar kernel (tests/quasar_shapes.py, judged on the GPU by tests/test_gpu_quasar_shapes.py):
* the long-double run of the restatement is finite on every row but the out-of-box row and the Om < 0 row, and on those two
  the quasar chi^2 is still finite: no row is left out of the comparison;
* its float64 run agrees with its long-double run to 1e-12 on every compared quantity (log L on the scale of the GPU bar):
  no case is so ill-conditioned that the GPU's 1e-10 would be a coin toss;
* every value of every list of the sweep is reached over the default 24 seeds.

Chain sums (tests/chain_shapes.py, judged on the GPU by tests/test_gpu_chain_kernels.py):
* a float64 restatement of the kernel's segment order stays below 0.2 of the derived bound at every n_t of the sweep;
* the bound is at most 3e-6 of a median product, so one dropped or mis-indexed product misses it by five orders.
"""
import numpy as np
import pytest

import chain_shapes as cs
import quasar_shapes as qs

LD = np.longdouble
QUANTITIES = ("chi2_parts", "chi2", "mu_qsr", "mu_sn", "bao_theory")


def test_long_double_is_an_extended_type():
    assert np.finfo(LD).eps < 1e-18


def _cases():
    return [qs.build_case(s) for s in range(qs.N_DEFAULT)] + [qs.fixed_case(n) for n in sorted(qs.FIXED_CASES)]


@pytest.fixture(scope="module")
def cases():
    return _cases()


@pytest.mark.parametrize("k", range(qs.N_DEFAULT + len(qs.FIXED_CASES)))
def test_reference_is_finite_and_well_conditioned(cases, k):
    assert np.finfo(LD).eps < 1e-18
    c = cases[k]
    want, f64 = qs.reference(c, LD), qs.reference(c, np.float64)
    W = c["W"]
    special = [r for r in (c["row_out"], c["row_om"]) if r is not None]
    assert (W > 2) == (c["row_out"] is not None) and (c["row_om"] is not None) == (W > 2 and "Om" in c["names"])
    plain = np.setdiff1d(np.arange(W), special)
    for name in QUANTITIES + ("logl",):
        if want[name] is not None:
            assert np.all(np.isfinite(want[name][plain])), (name, qs.describe(c))
    assert np.all(np.isfinite(want["logp"][plain])) and np.all(want["logp"][special] == -np.inf)
    assert np.all(np.isfinite(want["chi2_parts"][special, 1]))
    if c["row_out"] is not None:  # only the box makes this row special
        assert np.all(np.isfinite(want["chi2_parts"][c["row_out"]])) and np.isfinite(want["logl"][c["row_out"]])
    # the NaN-skipping sum has NaN terms to skip.  With Om = -0.05 E^2 turns negative near z = 1.8 at w0 = -1 and earlier
    # for w0 well below it, so whether the lowest grids (shared_above: the quasars end below the SNe) reach that point hangs
    # on the drawn w0 and z: it holds on the committed seeds, and this assertion is what notices a later change of the draw
    # that loses it (then lower Om in quasar_shapes.build_case, not this check).  One or two quasars may all sit below it.
    if c["row_om"] is not None:
        assert np.isnan(want["mu_qsr"][c["row_om"]]).any() or c["n_qsr"] < 3, qs.describe(c)
    worst = 0.0
    for name in QUANTITIES:
        if want[name] is None:
            continue
        fin = np.isfinite(want[name])
        assert np.array_equal(np.isfinite(f64[name]), fin), (name, qs.describe(c))
        err, size = np.abs(f64[name][fin] - want[name][fin]), np.abs(want[name][fin])
        assert np.all(err[size == 0] == 0)  # the chi^2 of an absent block is 0 in both
        if np.any(size > 0):
            worst = max(worst, float(np.max(err[size > 0] / size[size > 0])))
    fin = np.isfinite(want["logl"])
    assert np.array_equal(np.isfinite(f64["logl"]), fin)
    worst = max(worst, float(np.max(np.abs(f64["logl"][fin] - want["logl"][fin]) / qs.logl_scale(want)[fin])))
    print(f"{qs.describe(c)}: float64 against long double {worst:.2e}")
    assert worst <= 1e-12, qs.describe(c)


def test_every_list_of_the_sweep_is_reached(cases):
    seeded = cases[:qs.N_DEFAULT]

    def seen(key):
        return {c[key] for c in seeded}

    assert seen("n_grid") == set(qs.N_GRID) and seen("n_qsr") == set(qs.N_QSR) and seen("n_sn") == set(qs.N_SN)
    assert seen("n_bao") == set(qs.N_BAO) and seen("W") == set(qs.WALKERS) and seen("nkp") == set(qs.NKP)
    assert seen("z_top_mode") == set(qs.Z_TOP) and seen("solve") == {"auto", "blocked"}
    assert {c["sn_grid_mode"] for c in seeded if c["n_sn"]} == set(qs.SN_GRID)
    assert {c["sn_zhel"] for c in seeded if c["n_sn"]} == {False, True}
    assert {c["bao_z_mode"] for c in seeded if c["n_bao"] > 1} == set(qs.BAO_Z)
    assert sum(c["h0_free"] for c in seeded) == qs.N_DEFAULT // 2
    assert {c["fixed"] for c in seeded if c["fixed"] and (c["fixed"] != "offset" or c["n_sn"])} == set(qs.FIXABLE)
    assert sum(c["fixed"] is not None for c in seeded) == qs.N_DEFAULT // 4
    assert any(c["scale"] for c in seeded) and all(v != 1.0 for c in seeded for v in c["scale"].values())
    for c in seeded:
        z, G = c["qsr"][0], c["n_grid"]
        nodes = np.linspace(0.0, c["z_top"], G)
        if c["n_qsr"] >= 6:  # on node 1, on the top node (or the one below), inside the first interval, repeated
            assert nodes[1] in z and (nodes[-1] in z or nodes[-2] in z) and np.any((z > 0) & (z < nodes[1]))
            assert np.unique(z).size < z.size
        if c["z_top_mode"] == "below":
            assert np.any(z > c["z_top"])
        if c["z_top_mode"] == "above":
            assert np.all(z[c["qsr_specials"]:] < c["z_top"])  # every drawn redshift; one of the special ones sits ON the top node
        if c["sn_grid_mode"] == "shared_above":
            assert np.any(c["sn"][0] > c["z_top"]) and c["sn_z_top"] == 0.0
        if c["sn_grid_mode"] == "own":
            assert c["sn_z_top"] == np.max(c["sn"][0])
    assert any(nodes_top in c["qsr"][0] for c in seeded for nodes_top in [c["z_top"]])
    bao = [c for c in seeded if c["n_bao"]]
    assert any(np.any(c["bao"][0] > c["z_top"]) for c in bao)
    assert {int(q) for c in bao for q in c["bao"][2]} == {0, 1, 2}
    for c in bao:
        bz, cov = c["bao"][0], c["bao"][3]
        if c["n_bao"] > 1:
            n_distinct = np.unique(bz).size
            assert {"distinct": n_distinct == bz.size, "equal": n_distinct <= 2, "pairs": 1 < n_distinct < bz.size}[c["bao_z_mode"]]
            assert np.count_nonzero(cov - np.diag(np.diag(cov))) > 0 and np.all(np.linalg.eigvalsh(cov) > 0)
    for name, force in qs.FIXED_CASES.items():
        c = qs.fixed_case(name)
        assert c["n_grid"] == 8192 and (c["sn_z_top"] > 0) == (name == "two_grids_8192") and c["n_sn"] > 0


# ---- chain sums ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_t", cs.N_T)
def test_chain_bound_holds_for_the_segment_order_and_is_sharp(n_t):
    assert np.finfo(LD).eps < 1e-18
    x = cs.series(n_t, 8, seed=n_t)
    mean_ld, d = cs.reference_mean(x)
    got_mean = cs.segment_mean(x)
    assert np.all(np.abs(got_mean - mean_ld.astype(np.float64)) <= cs.mean_bound(x))
    lags = sorted({t for t in (0, 1, 15, 16, 17, n_t // 2, n_t - 1) if 0 <= t < n_t})
    for tau in lags:
        ref, bound = cs.reference_lagsum(x, d, tau), cs.lagsum_bound(x, d, tau)
        got = cs.segment_lagsum(x, got_mean, tau)
        err = np.abs(got - ref.astype(np.float64))
        assert np.all(err <= 0.2 * bound), (n_t, tau, float(np.max(err / bound)))
        # sharpness: one product of median size (the median of d_t^2 over the series) is far outside the bound
        if n_t >= 15:
            med = np.median((d * d).astype(np.float64), axis=0)
            assert np.all(bound <= 3e-6 * med), (n_t, tau, float(np.max(bound / med)))
