"""GPU (-m gpu): small_blocks_kernel<MODEL, FDE, LANES, ROLES> (csrc/cosmofit_kernels.hip: z* / r_drag fits, compressed-CMB
integrals, cosmic chronometers, BAO) over its three launch forms, block sizes, models and options (tests/blocks_shapes.py), against
a long-double reference (tests/blocks_reference.py).

* Form asserted, not assumed: every worker asserts through cf_small_blocks_form that the form its CF_TUNE string asks for is the one
  that runs (an unknown key is silently ignored), one fresh process per string (tests/blocks_forms_worker.py).
* Same bits: every output of parts() and chi_squared of every case has ONE bit pattern in the 16 x 1, 64 x 1 and 64 x 2 forms, alone
  and inside a 2049-walker batch across the automatic switch, and in the first W rows of a batch evaluated alone.
* Against the reference: bao_theory, the CMB vector, z* and r_drag within the project's 1e-10 relative; each block's chi^2 within
  1e-10 x its scale (blocks_reference: sum |d_i||K_ij||d_j| + 2 sum |g_i||t_i|, what the theory bar propagates to).
* A NaN row and a row outside every positive-base assumption change no other row of their workgroup.
Every test prints its worst error as a fraction of its bar; the measured values are in profiles/NOTES_small_blocks.md."""
import numpy as np
import pytest

import blocks_shapes as S

pytestmark = pytest.mark.gpu
BAR = 1e-10
GENERIC = "walker_generic=1"
TYPO = "sb_wide_maxx=0,sb_roles=0,wide_max=0,sb_roles_max"  # no key of the library: silently ignored


@pytest.fixture(scope="module")
def gpu(pkg):
    if pkg.lib().cf_device_count() < 1:
        pytest.fail("GPU tests need an MI355X; no HIP device visible (there is no fallback path)")
    return pkg


@pytest.fixture(scope="module")
def workers(gpu, tmp_path_factory):
    jobs = [("forced", tune) for tune in S.FORMS.values()] + [("auto", ""), ("generic", GENERIC), ("typo", TYPO)]
    return S.run_workers(jobs, tmp_path_factory.mktemp("blocks_forms"))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _got(result, prefix):
    return {key: result[f"{prefix}:{key}"] for key in S.OUTPUTS if f"{prefix}:{key}" in result}


def _row_diff(a, b):
    """rows whose bit patterns differ"""
    return np.flatnonzero(np.any((_bits(a) != _bits(b)).reshape(a.shape[0], -1), axis=1))


def _assert_bars(name, got, what, sel=None):
    r = S.ratios(name, got, sel=sel, bar=BAR)
    print(f"{name} [{what}]: worst error / bar: " + ", ".join(f"{k} {v:.2e}" for k, v in r.items()))
    bad = {k: v for k, v in r.items() if not v < 1.0}
    assert not bad, f"{name} [{what}]: outputs past the bar of {BAR} (error / bar): {bad}; case {S.CASES[name]}"
    return r


@pytest.mark.parametrize("name", list(S.CASES))
def test_three_forms_give_one_bit_pattern(gpu, workers, name):
    got = {form: _got(workers[("forced", tune)], name) for form, tune in S.FORMS.items()}
    base = got[(16, 1)]
    assert set(base) >= {"chi2", "chi2_bao", "chi2_cmb", "chi2_cc", "cmb_vector", "z_star", "r_drag"}
    assert ("bao_theory" in base) == bool(S.CASES[name]["n_bao"])
    for form in ((64, 1), (64, 2)):
        for key, v in base.items():
            bad = _row_diff(v, got[form][key])
            assert bad.size == 0, (f"{name}: {key} of rows {bad} differs between 16 x 1 and {form[0]} x {form[1]}; first: "
                                   f"{v[bad[0]]!r} vs {got[form][key][bad[0]]!r}; case {S.CASES[name]}")


@pytest.mark.parametrize("name", list(S.CASES))
def test_sixteen_lane_form_meets_the_reference(gpu, workers, name):
    got = _got(workers[("forced", S.FORMS[(16, 1)])], name)
    for key, v in got.items():
        assert np.all(np.isfinite(v)), f"{name}: {key} is not finite on rows inside the box"
    _assert_bars(name, got, "16 x 1")
    # the total is the three blocks' sum (absent blocks 0): four ulp cover any order of the two additions
    total = (got["chi2_cmb"] + got["chi2_bao"]) + got["chi2_cc"]
    assert np.all(np.abs(got["chi2"] - total) <= 4 * np.spacing(total)), f"{name}: chi_squared is not the sum of its blocks"


@pytest.mark.parametrize("name", S.SWITCH_CASES)
def test_automatic_switch_keeps_the_bits(gpu, workers, name):
    """No CF_TUNE: 33 walkers take 64 x 2, 2049 take 16 x 1 (asserted in the worker); the 33 rows alone, inside the 2049-row batch
    and in the forced forms are one bit pattern."""
    auto = workers[("auto", "")]
    forced = _got(workers[("forced", S.FORMS[(16, 1)])], name)
    small, big = _got(auto, name), _got(auto, name + ":big")
    for key, v in forced.items():
        for what, other in (("33 walkers, default form", small[key]), (f"inside {S.W_LARGE} walkers, default form", big[key])):
            bad = _row_diff(v, other)
            assert bad.size == 0, f"{name}: {key} of rows {bad} differs between the forced 16 x 1 form and {what}"


@pytest.mark.parametrize("name", (S.LARGEST_SIZE_CASE, "model_late_cpl", "opt_cmb_mode3"))
def test_first_rows_alone_give_their_bits_in_the_batch(gpu, name):
    """In this process (no CF_TUNE: 64 x 2): the first W rows evaluated alone against the same rows of the 33-row batch."""
    with S.engine(gpu, name) as eng:
        assert eng.small_blocks_form(S.N_ROWS) == (64, 2), "this test needs a process without CF_TUNE sb_* keys"
        full = S.evaluate(eng, S.rows(name))
        for W in S.W_SHAPES:
            part = S.evaluate(eng, S.rows(name)[:W])
            for key, v in part.items():
                bad = _row_diff(v, full[key][:W])
                assert bad.size == 0, f"{name}: {key} of rows {bad} of a {W}-walker batch differs from the 33-walker batch"
    _assert_bars(name, full, "64 x 2, in process")


@pytest.mark.parametrize("form", list(S.FORMS))
def test_a_bad_row_changes_no_neighbour(gpu, workers, form):
    """NaN in H0 of row 16, row 17 outside every positive-base assumption: 2, 4 or 16 walkers share a workgroup's LDS and shuffles,
    and only those two rows may change."""
    result = workers[("forced", S.FORMS[form])]
    keep = np.setdiff1d(np.arange(S.N_ROWS), [S.ROW_NAN, S.ROW_BAD])
    for name in S.CASES:
        good, bad = _got(result, name), _got(result, name + ":bad")
        for key, v in good.items():
            diff = np.intersect1d(_row_diff(v, bad[key]), keep)
            assert diff.size == 0, f"{name} {form}: {key} of rows {diff} changed when rows {S.ROW_NAN} and {S.ROW_BAD} went bad"
        assert not np.isfinite(bad["chi2"][S.ROW_NAN]), f"{name} {form}: a NaN H0 gave chi^2 = {bad['chi2'][S.ROW_NAN]!r}"


@pytest.mark.parametrize("name", S.EDGE_CASES)
def test_generic_per_walker_kernel_at_the_grid_edges(gpu, workers, name):
    """CF_TUNE walker_generic=1 (walker_form == 2, asserted in the worker): the generic kernel copies the table nodes out; judged by
    the reference alone -- bits against the lean kernel are not claimed."""
    _assert_bars(name, _got(workers[("generic", GENERIC)], name), "generic per-walker kernel")


def test_mistyped_keys_report_and_run_the_defaults(gpu, workers):
    """The worker asserts (64, 2) up to 2048 walkers and (16, 1) above under the mistyped string; its outputs are the default bits."""
    name = S.SWITCH_CASES[1]
    typo, auto = _got(workers[("typo", TYPO)], name), _got(workers[("auto", "")], name)
    for key, v in auto.items():
        assert _row_diff(v, typo[key]).size == 0, key


def test_form_query_without_small_blocks_and_with_bad_arguments(gpu):
    import solve_shapes

    with solve_shapes.engine(gpu, 17) as eng:  # an SN-only engine: no BAO, CMB or chronometer block
        assert eng.small_blocks_form(33) is None and gpu.lib().cf_small_blocks_form(eng._h, 33) == 0
    with S.engine(gpu, "opt_cc_only") as eng:
        assert gpu.lib().cf_small_blocks_form(eng._h, 33) == S.FORM_CODE[(64, 2)]
        assert gpu.lib().cf_small_blocks_form(eng._h, S.W_LARGE) == S.FORM_CODE[(16, 1)]
        for W in (0, -5):
            with pytest.raises(gpu.CosmofitError, match="CF_ERR_INVALID.*cf_small_blocks_form"):
                eng.small_blocks_form(W)
