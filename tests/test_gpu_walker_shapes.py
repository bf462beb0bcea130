"""
The per-walker SN stage -- the generic kernel, the workgroup form in both residual layouts and the streaming form -- over the models,
grids, SN forms and data edges of tests/walker_shapes.py, against a long-double reference of the residual rows
(tests/walker_reference.py) read through cf_last_residuals, and against oracle_np for chi^2 and log P.

* Form asserted, not assumed: every worker (tests/walker_forms_worker.py, one fresh process per CF_TUNE string) asserts through
  walker_form, solve_form and the accessor's layout that the form its string asks for is the one that ran.
* Residual rows: |row - reference| <= 1e-12 + 4 env per (walker, SN), env = 2^-52 (5 / ln 10) (1 + z) / |z_cosmo| (what one ulp of
  1 + z in z_cosmo moves a residual by: 1e-12 alone cannot hold below z ~ 0.01; tests/test_walker_shapes_cpu.py holds the float64
  oracle to 1e-13 + 2 env on the same cases).  Pairs with z_cosmo <= 0 and the NaN row are compared by finite / non-finite.
* Padding: rows n_sn .. n_ld - 1 of every walker are exactly 0.0 in every form and layout.
* chi^2 and log P against oracle_np at rtol 1e-10; NaN chi^2 exactly where the references say, log P = -inf there and outside the box.
* Same bits: the streaming form and both layouts of the workgroup form agree in every bit of rows, chi^2 and log P.  The generic
  kernel is held to the tolerance only; whether its bits agree is printed.
* Layouts back to back on one handle, and the automatic switch of every model family at 4096 walkers.
"""
import numpy as np
import pytest

import walker_shapes as S

LD = np.longdouble
RTOL = 1e-10
MODES = tuple(S.FORMS)
SAME_BITS_MODES = ("stream", "wg_default", "wg_rows")


@pytest.fixture(scope="module")
def forms(tmp_path_factory):
    d = tmp_path_factory.mktemp("walker_shapes")
    return S.run_workers([(m, S.FORMS[m][0]) for m in MODES], d)


@pytest.fixture(scope="module")
def auto(tmp_path_factory):
    d = tmp_path_factory.mktemp("walker_shapes_auto")
    return S.run_workers([("auto", "")], d)["auto"]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _ratio(rows, ref, sel=None):
    """(largest (|err| - 1e-12) / env, largest |err| / tol, where) over the fully compared pairs of the reference rows `sel`."""
    sel = np.arange(rows.shape[0]) if sel is None else sel
    n = ref["delta"].shape[1]
    full = ~ref["class_only"][sel]
    err = np.abs(rows[:, :n].astype(LD) - ref["delta"][sel])
    with np.errstate(all="ignore"):
        b = np.where(full, (err - LD(1e-12)) / ref["env"][sel], -np.inf)
        q = np.where(full, err / ref["tol"][sel], 0)
    q = np.where(np.isnan(q), np.inf, q)
    k = np.unravel_index(int(np.argmax(q)), q.shape)
    return float(np.max(b)), float(q[k]), k


def _check_rows(tag, rows, ref, n_sn, sel=None):
    sel = np.arange(rows.shape[0]) if sel is None else sel
    b, q, k = _ratio(rows, ref, sel)
    print(f"{tag}: {rows.shape[0]} walkers x {n_sn} SNe, worst |err| / tol = {q:.3f} at (walker {k[0]}, SN {k[1]}), "
          f"largest (|err| - 1e-12) / env = {b:.3f}")
    assert q <= 1.0, f"{tag}: residual of (walker {k[0]}, SN {k[1]}) is {q:.3f} x (1e-12 + 4 env) from the reference"
    assert np.array_equal(np.isfinite(rows[:, :n_sn]), np.isfinite(ref["delta"][sel].astype(np.float64))), \
        f"{tag}: finite / non-finite residuals differ from the reference"
    pad = rows[:, n_sn:]
    assert np.array_equal(_bits(pad), np.zeros(pad.shape, dtype=np.uint64)), f"{tag}: padding rows {np.unique(np.nonzero(pad)[1]) + n_sn}"
    return b


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", S.RESIDUAL_CASES)
def test_residual_rows_against_the_long_double_reference(forms, name, mode):
    rows, ref, n_sn = forms[mode][f"{name}:rows"], S.reference(name), S.CASES[name]["n_sn"]
    assert rows.shape == (S.N_ROWS, S.n_ld_of(n_sn)) and int(forms[mode][f"{name}:layout"]) == S.expected_form(name, mode)[1]
    _check_rows(f"{name} [{mode}]", rows, ref, n_sn)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(S.CASES))
def test_padding_rows_are_zero(forms, name, mode):
    n_sn = S.CASES[name]["n_sn"]
    pad = forms[mode][f"{name}:rows"][:, n_sn:]
    assert pad.shape == (S.N_ROWS, S.n_ld_of(n_sn) - n_sn)
    assert np.array_equal(_bits(pad), np.zeros(pad.shape, dtype=np.uint64)), f"walkers {np.unique(np.nonzero(pad)[0])}"


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", S.RESIDUAL_CASES)
def test_non_finite_classes_match(forms, name, mode):
    got, ref, n_sn = forms[mode], S.reference(name), S.CASES[name]["n_sn"]
    ref_finite = np.isfinite(ref["delta"].astype(np.float64))
    assert np.array_equal(np.isfinite(got[f"{name}:rows"][:, :n_sn]), ref_finite)
    chi2, logp = got[f"{name}:chi2"], got[f"{name}:logp"]
    bad = ~ref_finite.all(axis=1)
    outside = ref["out_of_box"] | ref["bad_row"]
    assert np.array_equal(np.isnan(chi2), bad) and np.all(np.isfinite(chi2[~bad]))
    # -inf outside the strict box (sn/pantheon.py:88-93) and, by the library's contract, where chi^2 is NaN (finalize_value: emcee
    # aborts on a NaN log-probability); never NaN
    assert np.array_equal(np.isneginf(logp), outside | bad) and np.all(np.isfinite(logp[~(outside | bad)]))
    if S.CASES[name]["form"] in ("pm1", "weights"):  # the special rows did what they are there for
        assert bad[S.ROW_ZNEG] and bad[S.ROW_NAN] and outside[S.ROW_OOB] and not bad[S.ROW_OOB]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", S.CHI2_CASES)
def test_chi2_and_log_probability_against_the_oracle(forms, name, mode):
    want = S.oracle_values(name)
    for kind in ("chi2", "logp"):
        got, ref = forms[mode][f"{name}:{kind}"], want[kind]
        if kind == "logp":  # the library's contract: a NaN chi^2 inside the box is log P = -inf (finalize_value), not the oracle's NaN
            ref = np.where(np.isnan(ref), -np.inf, ref)
        ok = np.isfinite(ref)
        assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isneginf(got), np.isneginf(ref)), f"{name}:{kind}"
        rel = np.abs(got[ok] - ref[ok]) / np.abs(ref[ok])
        print(f"{name} [{mode}] {kind}: {int(ok.sum())} finite rows, largest relative error {rel.max():.2e}")
        assert rel.max() <= RTOL, f"{name}:{kind}: row {np.flatnonzero(ok)[int(np.argmax(rel))]} is {rel.max():.2e} from oracle_np"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(S.CASES))
def test_streaming_and_workgroup_forms_give_the_same_bits(forms, name):
    kinds = ("rows", "chi2", "logp") + (("logl",) if S.CASES[name]["growth"] else ())
    a = forms[SAME_BITS_MODES[0]]
    for kind in kinds:
        for mode in SAME_BITS_MODES[1:]:
            x, y = a[f"{name}:{kind}"], forms[mode][f"{name}:{kind}"]
            diff = np.argwhere(_bits(x) != _bits(y))
            assert x.shape == y.shape and diff.size == 0, f"{name}:{kind}: stream and {mode} differ at {diff[:6].tolist()}"
        g = forms["generic"][f"{name}:{kind}"]
        print(f"{name}:{kind}: generic kernel bits {'agree' if np.array_equal(_bits(g), _bits(a[f'{name}:{kind}'])) else 'DIFFER'}"
              f" ({int((_bits(g) != _bits(a[f'{name}:{kind}'])).sum())} of {g.size})")
    if S.CASES[name]["growth"]:
        assert np.isfinite(a[f"{name}:logl"]).sum() >= 25


@pytest.mark.gpu
def test_measured_envelope_per_form(forms):
    """Printed for profiles/NOTES_walker_shapes.md: per form, the largest (|err| - 1e-12) / env over every case (the tolerance allows
    4), and the largest relative error of chi^2 and log P against oracle_np."""
    for mode in MODES:
        worst_b, worst_rel = (-np.inf, ""), {"chi2": (0.0, ""), "logp": (0.0, "")}
        for name in S.RESIDUAL_CASES:
            b, _, _ = _ratio(forms[mode][f"{name}:rows"], S.reference(name))
            worst_b = max(worst_b, (b, name))
        for name in S.CHI2_CASES:
            want = S.oracle_values(name)
            for kind in worst_rel:
                got, ref = forms[mode][f"{name}:{kind}"], want[kind]
                ok = np.isfinite(ref) & np.isfinite(got)
                worst_rel[kind] = max(worst_rel[kind], (float(np.max(np.abs(got[ok] - ref[ok]) / np.abs(ref[ok]))), name))
        print(f"[{mode}] B = {worst_b[0]:.3f} ({worst_b[1]}), chi2 rel {worst_rel['chi2'][0]:.2e} ({worst_rel['chi2'][1]}), "
              f"logp rel {worst_rel['logp'][0]:.2e} ({worst_rel['logp'][1]})")
        assert worst_b[0] <= 4.0


@pytest.mark.gpu
def test_layouts_back_to_back_on_one_handle(auto):
    name = S.B2B_CASE
    ref, want, n_sn = S.reference(name), S.oracle_values(name), S.CASES[name]["n_sn"]
    for k, W in enumerate(S.W_BACK_TO_BACK + (S.W_BACK_TO_BACK[0],)):
        sel = S.b2b_rows(W)
        rows, chi2 = auto[f"b2b:{k}:rows"], auto[f"b2b:{k}:chi2"]
        assert int(auto[f"b2b:{k}:layout"]) == (1 if W <= 160 else 0) and rows.shape == (W, S.n_ld_of(n_sn))
        _check_rows(f"{name}: batch {k} of {W} walkers", rows, ref, n_sn, sel)
        five = np.flatnonzero(np.isin(sel, S.B2B_FIVE))
        assert five.size >= 5
        rel = np.abs(chi2[five] - want["chi2"][sel[five]]) / np.abs(want["chi2"][sel[five]])
        print(f"batch {k} of {W} walkers: chi2 of rows {S.B2B_FIVE}: largest relative error {rel.max():.2e}")
        assert rel.max() <= RTOL


@pytest.mark.gpu
def test_automatic_switch_of_every_family(auto):
    names = sorted(n for n, c in S.CASES.items() if c["group"] == "model")
    got = dict(zip(names, auto["auto:walker_form_4096"].tolist()))
    in_budget = {n: int(not (S.CASES[n]["fde"] == S.CPL or (S.CASES[n]["ez_model"] == S.PHYSICAL and S.CASES[n]["fde"] == S.WCDM)))
                 for n in names}
    print(auto["log"])
    assert sum(in_budget.values()) == 5 and got == in_budget, got
    for name in S.AUTO_CASES:
        ref, n_sn = S.reference(name), S.CASES[name]["n_sn"]
        big, small = auto[f"auto:{name}:rows4096"], auto[f"auto:{name}:rows33"]
        _check_rows(f"{name}: 33 rows inside {S.W_AUTO} walkers (streaming form)", big, ref, n_sn)
        _check_rows(f"{name}: 33 rows alone (workgroup form, fragment order)", small, ref, n_sn)
        for kind in ("rows", "chi2_", "logp_"):
            x, y = auto[f"auto:{name}:{kind}4096"], auto[f"auto:{name}:{kind}33"]
            assert np.array_equal(_bits(x), _bits(y)), f"{name}:{kind}: rows {np.unique(np.argwhere(_bits(x) != _bits(y))[:, 0])} differ"
