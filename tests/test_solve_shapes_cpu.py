"""CPU: the parts of the inverse-GEMM solve sweep that need no GPU (the GPU part is tests/test_gpu_solve_shapes.py).

* the long-double reference of tests/solve_reference.py against the float64 numpy oracle on every base set;
* cf_solve_form over the shape table x its batch sizes reaches every launch-time form the sweep is there for -- the condition
  that keeps the GPU sweep from going vacuous: if a default moves, EXTEND tests/solve_shapes.py, do not relax these assertions;
* child processes under each CF_TUNE string of the sweep report the forced values, and a mistyped key reports the defaults."""
import numpy as np
import pytest

import solve_reference
import solve_shapes as S


@pytest.mark.parametrize("n,n_rb,nt_last", [s[:3] for s in S.SIZES])
def test_longdouble_reference_agrees_with_the_float64_oracle(n, n_rb, nt_last):
    for fixed in ((False, True) if n in S.N_FIXED_MU else (False,)):
        lk = S.oracle_likelihood(n, fixed)
        base = S.base_rows(n)
        assert base.shape == (S.n_base(n), 4) and np.unique(base, axis=0).shape[0] == base.shape[0]
        ref = solve_reference.reference(lk, base)
        rel = np.max(np.abs(ref["chi2_f64"] - ref["chi2"]) / ref["chi2"])
        print(f"N={n} fixed_mu={fixed}: max |oracle float64 - long double| / chi^2 = {rel:.2e} over {base.shape[0]} rows, "
              f"chi^2 in [{ref['chi2'].min():.4g}, {ref['chi2'].max():.4g}]")
        assert np.all(np.isfinite(ref["chi2"])) and np.all(ref["chi2"] > 0)
        assert rel < 1e-13
        # log P: -inf for the row outside the box only; the row on the box face is inside
        assert np.flatnonzero(np.isneginf(ref["logp"])).tolist() == [S.ROW_OUTSIDE]
        ok = np.isfinite(ref["logp"])
        want = np.array([S.onp.log_probability(lk, t) for t in base[ok]])
        np.testing.assert_allclose(ref["logp"][ok], want, rtol=1e-13)


def test_shape_table_arithmetic():
    for n, n_rb, nt_last, _ in S.SIZES:
        f = S.default_form(n, 4096)
        assert (f["n_rb"], f["nt_last"]) == (n_rb, nt_last), (n, f)
    for n in (251, 31):  # the stride of batch_rows reaches every base row
        assert sorted(set(S.batch_rows(n, n).tolist())) == list(range(n))


@pytest.fixture(scope="module")
def child_forms(pkg, tmp_path_factory):
    """cf_solve_form in fresh processes: without CF_TUNE over the whole table ("" -> forms-default), and under each string of the
    sweep, a mistyped key and no key over the worker's batch sizes."""
    d = tmp_path_factory.mktemp("solve_forms")
    out = S.run_workers(("",), d, mode="forms-default")
    forced = S.run_workers(S.TUNES + ("gemm_nq=1,small_maxx=0", ""), d, mode="forms")
    return out[""], forced


def test_default_forms_cover_every_path_of_the_sweep(child_forms):
    table, _ = child_forms
    forms = []
    for n, n_rb, nt_last, _ in S.SIZES:
        for W in S.w_list(n):
            f = S.form_dict(table[f"{n}:{W}:form"])
            del f["frag_order"]
            assert f == S.default_form(n, W), (n, W, f, S.default_form(n, W))
            assert (f["n_rb"], f["nt_last"]) == (n_rb, nt_last)
            forms.append((n, W, f))
    have = lambda pred: [(n, W) for n, W, f in forms if pred(n, W, f)]
    assert have(lambda n, W, f: f["kernel"] == 0) and have(lambda n, W, f: f["kernel"] == 1)
    for pw in (16, 32):
        assert have(lambda n, W, f: f["kernel"] == 1 and f["panel_width"] == pw), pw
    for tpw in (1, 2):
        assert have(lambda n, W, f: f["kernel"] == 0 and f["tpw"] == tpw), tpw
    for t in (1, 2, 3, 4):  # in the throughput kernel, which is the one that trims, at more than one row block
        assert have(lambda n, W, f: f["kernel"] == 1 and f["n_rb"] > 1 and f["nt_last"] == t), t
    assert have(lambda n, W, f: f["kernel"] == 1 and f["panel_width"] == 32 and f["split_levels"] == 0)
    assert have(lambda n, W, f: f["split_levels"] == 1 and f["n_rb"] == 2)                       # one split, one whole
    assert have(lambda n, W, f: f["split_levels"] == f["n_rb"] - 1 and f["n_rb"] > 2)            # every level but the top one
    assert have(lambda n, W, f: f["split_levels"] == 6 and f["n_rb"] - 1 > 6)
    for snake in (0, 1):
        assert have(lambda n, W, f: f["kernel"] == 1 and f["snake"] == snake), snake
    # a last panel group that is partly empty
    assert have(lambda n, W, f: f["n_groups"] > 1 and f["n_groups"] * f["panels_per_group"] > -(-W // f["panel_width"]))
    # the small-batch kernel past 4096 shares (no LDS staging of the last arriver's sums), both tile counts
    for tpw in (1, 2):
        assert have(lambda n, W, f: f["kernel"] == 0 and 64 * f["n_rb"] > 4096 and f["tpw"] == tpw), tpw
    # a second half that is empty (W mod 32 in 1..16) under half units
    assert have(lambda n, W, f: f["split_levels"] > 0 and 1 <= W % 32 <= 16)


def test_forced_forms_in_child_processes(child_forms):
    _, forced = child_forms
    for k, tune in enumerate(S.TUNES):
        for n in S.N_SMALL:
            for W in S.W_WORKER:
                S.check_forced(k, n, W, S.form_dict(forced[tune][f"{n}:{W}:form"]))
    # every string changes some form of the worker's list, or the GPU comparison under it would compare the default with itself
    # (the last string's other keys -- gemm_diag_skip, small_lds_cap, sn_parts -- are not part of the form: gemm_trim shows there)
    for tune in S.TUNES:
        assert any(not np.array_equal(forced[tune][key], forced[""][key]) for key in forced[""]), tune
    # ... which is what a mistyped key does: silently the defaults
    typo = forced["gemm_nq=1,small_maxx=0"]
    assert all(np.array_equal(typo[key], forced[""][key]) for key in forced[""])
    for n in S.N_SMALL:
        for W in S.W_WORKER:
            f = S.form_dict(forced[""][f"{n}:{W}:form"])
            del f["frag_order"]
            assert f == S.default_form(n, W)


def test_solve_form_rejects_bad_arguments(pkg):
    import ctypes as C

    out = (C.c_int32 * 10)()
    lib = pkg.lib()
    for n, W in ((0, 16), (-1, 16), ((1 << 20) + 1, 16), (100, 0), (100, -5)):
        assert lib.cf_solve_form(n, W, C.byref(out)) == -1, (n, W)
    assert lib.cf_solve_form(100, 16, None) == -1
    assert lib.cf_solve_form(1 << 20, 1 << 20, C.byref(out)) == 0 and out[3] == (1 << 20) // 64
