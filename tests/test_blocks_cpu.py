"""CPU: the long-double restatement of the small blocks (tests/blocks_reference.py) deserves to judge the kernel -- it reproduces
what the reference itself computed (the fixtures' theory, cmb_dist, chi2_parts, chi2_cmb), agrees with the float64 oracle
(oracle/oracle_np.py) on every case of the sweep (tests/blocks_shapes.py), and is finite on every row of every case -- and the
sweep covers what it is there for.  cf_small_blocks_form's argument errors are reported without a device; its reports under the
CF_TUNE strings need a handle, hence a device: tests/test_gpu_blocks_shapes.py."""
import numpy as np
import pytest

import blocks_reference as B
import blocks_shapes as S
from conftest import golden
from oracle import oracle_np as onp

LD = np.longdouble


def _fixture_lk(pkg, name):
    """The oracle descriptor of a fixture's small blocks (no SN block: nothing here reads it)."""
    d = pkg.cmb_data.PLANCK_ACT
    g = golden(name)
    base = golden("bao_desi_cmb_des5y") if name == "bao_desi_cmb_des5y_cpl" else g
    slots, fde, kw = {
        "bao_desi_cmb_des5y": (dict(H0=1, obh2=2, och2=3), onp.FDE_LCDM, dict(cmb_mode=1)),
        "bao_desi_cmb_des5y_cpl": (dict(H0=1, obh2=2, och2=3, w0=5, wa=6), onp.FDE_CPL, dict(cmb_mode=1)),
        "bao_desi_fs_lya_cmb": (dict(H0=0, obh2=1, och2=2, w0=3, wa=4), onp.FDE_CPL, dict(cmb_mode=1)),
        "bao_desi_des5y_bbn_theta_star": (dict(H0=1, obh2=2, och2=3, w0=4), onp.FDE_THAWING, dict(cmb_mode=2, bao_dh_exact=True)),
        "sn_des5y_cmb": (dict(H0=1, obh2=2, och2=3), onp.FDE_LCDM, dict(cmb_mode=1)),
    }[name]
    inv = d["cmb_inv_cov"]
    if kw["cmb_mode"] == 2:  # bao/desi_des5y_bbn_theta_star.py:110-111
        inv = np.zeros((3, 3))
        inv[1, 1] = 1.0 / d["cmb_cov"][1, 1]
    if "bao_z" in base:
        kw.update(bao_z=base["bao_z"], bao_val=base["bao_val"], bao_qty=base["bao_qty"], bao_inv_cov=base["bao_inv_cov"], rd_fit=d["rd_fit"])
    phys = {k: d[k] for k in ("or_h2", "omnu_h2", "o_gamma_h2", "nu_m0", "nu_rho0", "nu_qs_sq", "nu_ws")}
    return g, onp.Likelihood(ndim=g["thetas"].shape[1], z_max=float(g["z_max"]), ez_model=onp.EZ_PHYSICAL, fde=fde,
                             **{k: onp.Slot(i) for k, i in slots.items()}, cmb_prior=d["cmb_prior"], cmb_inv_cov=inv,
                             zstar_fit=d["zstar_fit"], **phys, **kw)


@pytest.mark.parametrize("name", ["bao_desi_cmb_des5y", "bao_desi_cmb_des5y_cpl", "bao_desi_fs_lya_cmb", "bao_desi_des5y_bbn_theta_star",
                                  "sn_des5y_cmb"])
def test_reference_reproduces_the_fixtures(pkg, name):
    """At the bars tests/test_oracle_golden.py and tests/test_variants.py hold the oracle to for the same keys: theory 1e-12,
    cmb_dist 1e-13, chi2_parts 1e-10, chi2_cmb 1e-9, chi2_bao 1e-10."""
    g, lk = _fixture_lk(pkg, name)
    m, data = B.from_oracle(lk, pkg.cmb_data.ZSTAR_CONSTS)
    ref = B.reference(m, data, g["thetas"])
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    checked = 0
    if "theory" in g:
        k = g["theory"].shape[0]
        np.testing.assert_allclose(f64(ref["bao_theory"][:k]), g["theory"], rtol=1e-12)
        checked += 1
    if "cmb_dist" in g:
        k = g["cmb_dist"].shape[0]
        np.testing.assert_allclose(f64(ref["cmb_vector"][:k]), g["cmb_dist"], rtol=1e-13)
        checked += 1
    if "chi2_parts" in g:  # (sn, bao, cmb)
        np.testing.assert_allclose(f64(ref["chi2_bao"]), g["chi2_parts"][:, 1], rtol=1e-10)
        np.testing.assert_allclose(f64(ref["chi2_cmb"]), g["chi2_parts"][:, 2], rtol=1e-10)
        checked += 1
    if "chi2_cmb" in g:
        k = g["chi2_cmb"].shape[0]
        np.testing.assert_allclose(f64(ref["chi2_cmb"][:k]), g["chi2_cmb"], rtol=1e-9)
        checked += 1
    if "chi2_bao" in g:
        k = g["chi2_bao"].shape[0]
        np.testing.assert_allclose(f64(ref["chi2_bao"][:k]), g["chi2_bao"], rtol=1e-10)
        checked += 1
    assert checked >= 1


def test_reference_reproduces_the_chronometer_fixture(pkg):
    """ohd/cc.py on the 38 real chronometers: the fixture's chi^2 is the chronometer block's, also through oracle_np.chi2_cc."""
    g = golden("ohd_cc")
    lk = onp.Likelihood(ndim=3, z_max=float(np.max(g["cc_z"]) + 0.1), H0=onp.Slot(0), Om=onp.Slot(1), fcc=onp.Slot(2), cc_z=g["cc_z"],
                        cc_h=g["cc_h"], cc_inv_cov=np.linalg.inv(g["cc_cov"]), cc_logdet=np.linalg.slogdet(g["cc_cov"])[1])
    m, data = B.from_oracle(lk, pkg.cmb_data.ZSTAR_CONSTS)
    ref = B.reference(m, data, g["thetas"])
    want = np.array([onp.chi2_cc(lk, th) for th in g["thetas"]])
    np.testing.assert_allclose(np.asarray(ref["chi2_cc"], dtype=np.float64), want, rtol=1e-10)
    np.testing.assert_allclose(want, g["chi2"], rtol=1e-10)


def test_the_sweep_covers_what_it_is_there_for():
    size = [c for c in S.CASES.values() if c["group"] == "size"]
    assert {c["n_bao"] for c in size} == S.N_BAO_SET and {c["n_cc"] for c in size} == S.N_CC_SET and {c["n_gl"] for c in size} == S.N_GL_SET
    assert all(c["ez_model"] == S.PHYSICAL and c["fde"] == S.CPL and c["cmb_mode"] == 1 for c in size) and 8 <= len(size) <= 12
    # VirtualLaneSum<16>: pushes mod 4 takes every value (the fixtures' shapes give 1 and 3 only)
    pushes = {-(-n // 16) % 4 for c in size for n in (c["n_bao"], c["n_cc"], c["n_gl"])}
    assert pushes == {0, 1, 2, 3}
    models = [c for c in S.CASES.values() if c["group"] == "model"]
    assert {(c["ez_model"], c["fde"]) for c in models} == {(e, f) for e in (0, 1) for f in (0, 1, 2, 3)}
    assert all((c["n_bao"], c["n_cc"]) == (17, 33) and c["cmb_mode"] == (1 if c["ez_model"] else 0) for c in models)
    opts = list(S.CASES.values())
    assert {c["cmb_mode"] for c in opts} == {0, 1, 2, 3} and {c["rd"] for c in opts} == {"slot", "fit", "fit_late"}
    assert {c["dh_exact"] for c in opts} == {True, False} and {c["f_inverse"] for c in opts if c["n_cc"]} == {True, False}
    alone = {(bool(c["n_bao"]), bool(c["n_cc"]), bool(c["cmb_mode"])) for c in opts}
    assert {(True, False, False), (False, True, False), (False, False, True)} <= alone
    assert {c["n_grid"] for c in opts if c["edges"]} == {6, 64, 4000}
    for name in S.EDGE_CASES:  # first interval, either side of a node, last interval, at and above z_max
        z, zg = S.data(name)["bao"]["z"], np.linspace(0, S.Z_MAX, num=S.CASES[name]["n_grid"])
        node = zg[len(zg) // 2]
        assert 0 < z[0] < zg[1] and 0 < node - z[1] <= 1e-9 and 0 < z[2] - node <= 1e-9 and zg[-2] < z[3] < zg[-1]
        assert z[4] == zg[-1] == S.Z_MAX and z[5] > S.Z_MAX
    for name, c in S.CASES.items():
        d = S.data(name)
        if c["n_bao"] >= 4:
            assert set(d["bao"]["qty"]) == {0, 1, 2, 3}, name
        if not c["edges"] and c["n_bao"]:
            assert np.all((d["bao"]["z"] > 0) & (d["bao"]["z"] < S.Z_MAX)), name
        for blk in ("bao", "cc"):
            if d[blk] is not None:
                K = d[blk]["inv_cov"]
                assert np.array_equal(K, K.T) and np.all(np.linalg.eigvalsh(K) > 0), (name, blk)
                if K.shape[0] > 1:
                    assert np.abs(K - np.diag(np.diag(K))).max() > 0, (name, blk)  # correlated


@pytest.mark.parametrize("name", list(S.CASES))
def test_rows_lie_where_the_reference_is_finite(name):
    c, th = S.CASES[name], S.rows(name)
    assert th.shape == (S.N_ROWS, S.NDIM) == (33, 8)
    for j, col in enumerate(S.COLS):
        assert np.all((th[:, j] >= S.BOX[col][0]) & (th[:, j] <= S.BOX[col][1])), col
    assert th[S.ROW_WA_ZERO, 5] == 0.0 and not np.signbit(th[S.ROW_WA_ZERO, 5]) and np.any(th[:, 5] > 0) and np.any(th[:, 5] < 0)
    assert np.all(th[:, 4] + th[:, 5] <= 0)
    assert np.all(B.finite_box(S.model(name), S.data(name), th)), name
    ref = S.reference(name)
    for key, v in ref.items():
        assert np.all(np.isfinite(v)), (name, key)
    for key in ("scale_bao", "scale_cmb", "scale_cc"):
        if key in ref:
            assert np.all(ref[key] > 0) and np.all(ref[key] >= np.abs(ref["chi2" + key[5:]])), (name, key)
    bad = S.bad_rows(name)
    assert np.isnan(bad[S.ROW_NAN, 0]) and np.all(bad[S.ROW_BAD, :4] < 0)
    assert np.array_equal(np.delete(bad, [S.ROW_NAN, S.ROW_BAD], axis=0), np.delete(th, [S.ROW_NAN, S.ROW_BAD], axis=0))
    del c


@pytest.mark.parametrize("name", list(S.CASES))
def test_reference_agrees_with_the_float64_oracle(name):
    """1e-11 relative for the theory outputs, 1e-11 x the chi^2's scale for a chi^2 (a tenth of the kernel's bar)."""
    lk, th, ref = S.oracle_likelihood(name), S.rows(name), S.reference(name)
    c = S.CASES[name]
    got = {}
    rows = np.arange(S.N_ROWS)
    if c["n_bao"]:
        got["bao_theory"] = np.array([onp.bao_theory(lk, th[r]) for r in rows])
        got["chi2_bao"] = np.array([onp.chi2_bao(lk, th[r]) for r in rows])
        got["r_drag"] = np.asarray(ref["r_drag"][rows], dtype=np.float64)  # (the oracle has no separate r_d output)
    if c["cmb_mode"]:
        got["cmb_vector"] = np.array([onp.cmb_distances(lk, th[r]) for r in rows])
        got["chi2_cmb"] = np.array([onp.chi2_cmb(lk, th[r]) for r in rows])
        got["z_star"] = np.array([onp.z_star(lk.zstar_fit, th[r, 2], th[r, 3] + th[r, 2] + lk.omnu_h2) for r in rows])
    if c["n_cc"]:
        got["chi2_cc"] = np.array([onp.chi2_cc(lk, th[r]) for r in rows])
    r = S.ratios(name, got, sel=rows, bar=1e-11)
    print(f"{name}: oracle vs reference, worst error / (1e-11 x scale): " + ", ".join(f"{k} {v:.2e}" for k, v in r.items()))
    assert all(v < 1.0 for v in r.values()), (name, r)


def test_inverse_in_long_double_is_an_inverse():
    rng = np.random.default_rng(3)
    for n in (1, 2, 17, 64):
        C = S._cov(rng, rng.uniform(1.0, 50.0, n))
        K = S.inv_spd(C)
        assert np.abs(K @ C - np.eye(n)).max() < 1e-12 * np.linalg.cond(C)


def test_small_blocks_form_reports_argument_errors(pkg):
    lib, L = pkg.lib(), pkg._lib
    assert "cf_small_blocks_form" in L.EXPORTS
    assert lib.cf_small_blocks_form(None, 33) == -1  # CF_ERR_INVALID, as cf_walker_form
    assert b"cf_small_blocks_form" in lib.cf_last_error()
    assert lib.cf_walker_form(None, 33) == -1
    assert {S.FORM_CODE[f] for f in S.FORMS} == {16 + 256, 64 + 256, 64 + 512}


def test_create_rejects_what_the_kernel_cannot_take(pkg):
    """cf_create validates before any device work (the same here and on a GPU): a compressed-CMB block on the late-time flat model
    (no radiation up to z*) for every dark-energy form, Gauss-Legendre node counts outside 1..256, blocks of more than 64 data, and
    a BAO block on a grid of fewer than 6 nodes."""
    def kwargs(name, **changes):
        kw = S.engine_kwargs(pkg, name)
        for key, v in changes.items():
            if isinstance(v, dict):
                kw[key] = dict(kw[key], **v)
            else:
                kw[key] = v
        return kw

    full = S.engine_kwargs(pkg, "model_physical_cpl")
    for fde in (S.LCDM, S.WCDM, S.THAWING, S.CPL):
        with pytest.raises(pkg.CosmofitError, match="CF_ERR_INVALID.*CMB block needs CF_EZ_PHYSICAL"):
            pkg.LikelihoodEngine(**kwargs("model_physical_cpl", ez_model=pkg._lib.CF_EZ_LATE_FLAT, fde=fde))
    with pytest.raises(pkg.CosmofitError, match="CF_ERR_INVALID.*1..256 Gauss-Legendre"):
        pkg.LikelihoodEngine(**kwargs("model_physical_cpl", cmb=dict(n_gl=257)))
    big = 65
    K = np.eye(big)
    with pytest.raises(pkg.CosmofitError, match="CF_ERR_INVALID.*n_bao must be in 0..64"):
        pkg.LikelihoodEngine(**kwargs("model_physical_cpl", bao=dict(z=np.linspace(0.1, 2.0, big), val=np.ones(big), qty=np.zeros(big, dtype=np.int32),
                                                                   inv_cov=K)))
    with pytest.raises(pkg.CosmofitError, match="CF_ERR_INVALID.*n_cc must be in 0..64"):
        pkg.LikelihoodEngine(**kwargs("model_physical_cpl", cc=dict(z=np.linspace(0.1, 2.0, big), h=np.ones(big), inv_cov=K)))
    with pytest.raises(pkg.CosmofitError, match="CF_ERR_INVALID.*n_grid >= 6"):
        pkg.LikelihoodEngine(**kwargs("model_physical_cpl", n_grid=5))
    assert full["cmb"]["n_gl"] == 65
