"""GPU (-m gpu): the inverse-GEMM solve kernels (tri_gemm_chi2_kernel<NP,2>, tri_gemm_small_kernel<PF,FRAG,TPW>) over factor
sizes, batch bands and CF_TUNE knobs (tests/solve_shapes.py), against a long-double reference (tests/solve_reference.py).

* Against the reference: every row of every batch within the project's parity bar RTOL = 1e-10 of the long-double chi^2, and of
  log P where that is finite; the row outside the box exactly -inf; nonfinite_count 0.
* Same bits everywhere: every occurrence of a base row has ONE bit pattern -- in every batch of the default list and under all
  seven CF_TUNE strings (one fresh process each, tests/solve_forms_worker.py); DESIGN.md section 5: "none changes a result".
* Form asserted, not assumed: cf_solve_form of every (N, W) equals the rules written out in solve_shapes.default_form, in this
  process and in every worker, so a knob that did not take effect fails here instead of comparing the default with itself.
  tests/test_solve_shapes_cpu.py asserts that these forms cover every path the sweep is there for.
The worst relative errors as measured are recorded in profiles/NOTES_solve_shapes.md; the bar stays the project's 1e-10."""
import functools
import time

import numpy as np
import pytest

import solve_reference
import solve_shapes as S

pytestmark = pytest.mark.gpu
RTOL = 1e-10


@pytest.fixture(scope="module")
def gpu(pkg):
    if pkg.lib().cf_device_count() < 1:
        pytest.fail("GPU tests need an MI355X; no HIP device visible (there is no fallback path)")
    return pkg


@functools.lru_cache(maxsize=None)
def _reference(n, fixed):
    return solve_reference.reference(S.oracle_likelihood(n, fixed), S.base_rows(n))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _where(n, W, tune, form, i, b):
    panel, half, lane = S.position(i, form["panel_width"])
    return (f"N={n} W={W} CF_TUNE={tune!r} form={form}: walker {i} (base row {b}; panel {panel}, half {half}, lane column {lane})")


def _check_batch(n, W, tune, form, ref, canon, chi2, logp, worst):
    """One batch against the reference and against the canonical bits of its base rows."""
    B = ref["chi2"].size
    rows = S.batch_rows(W, B)
    assert chi2.shape == logp.shape == (W,)
    rel_c = np.abs(chi2 - ref["chi2"][rows]) / ref["chi2"][rows]
    fin = np.isfinite(ref["logp"][rows])
    with np.errstate(invalid="ignore"):
        rel_p = np.abs(logp[fin] - ref["logp"][rows][fin]) / np.abs(ref["logp"][rows][fin])
    key = (n, form["kernel"], form["panel_width"])
    worst[key] = max(worst.get(key, 0.0), float(np.nanmax(rel_c)), float(np.nanmax(rel_p)) if rel_p.size else 0.0)
    i = int(np.nanargmax(np.where(np.isnan(rel_c), np.inf, rel_c)))
    assert rel_c[i] < RTOL, f"chi^2 {chi2[i]!r} vs {ref['chi2'][rows[i]]!r} (rel {rel_c[i]:.3e}): " + _where(n, W, tune, form, i, rows[i])
    assert rel_p.size == 0 or np.all(rel_p < RTOL), f"log P rel {np.nanmax(rel_p):.3e}: N={n} W={W} CF_TUNE={tune!r} form={form}"
    assert np.array_equal(np.isneginf(logp), rows == S.ROW_OUTSIDE), f"-inf rows: N={n} W={W} CF_TUNE={tune!r} form={form}"
    for kind, got in (("chi2", chi2), ("logp", logp)):
        bad = np.flatnonzero(_bits(got) != canon[kind][rows])
        assert bad.size == 0, (f"{kind}: {bad.size} of {W} rows differ in bits from the same base row elsewhere; first: got {got[bad[0]]!r}, "
                               f"canonical {canon[kind][rows[bad[0]]].view(np.float64)!r}: " + _where(n, W, tune, form, bad[0], rows[bad[0]]))


_sweeps = {}


def _default_sweep(gpu, n, fixed=False, eng=None):
    """Every batch of the default list on one engine (once per process): checked against the reference and for one bit pattern per
    base row.  Returns dict(canon = bits per base row, worst = {(N, kernel, panel width): rel}, forms = {W: form})."""
    if (n, fixed) in _sweeps:
        return _sweeps[(n, fixed)]
    ref, base = _reference(n, fixed), S.base_rows(n)
    B = base.shape[0]
    own = eng is None
    eng = S.engine(gpu, n, fixed) if own else eng
    try:
        assert eng.info()["solve_mode"] == gpu.engine.solve_mode_of("inverse")
        got, forms = {}, {}
        for W in S.w_list(n):
            theta = base[S.batch_rows(W, B)]
            form = eng.solve_form(W)
            frag = form.pop("frag_order")
            # this process runs without CF_TUNE: the form is the default one (and the CPU test asserts what those cover)
            assert form == S.default_form(n, W), (n, W, form, S.default_form(n, W))
            if fixed:  # the generic per-walker kernel: residuals in walker rows into every solve kernel
                assert eng.walker_form(W) == 2 and frag == 0, (n, W, eng.walker_form(W), frag)
            else:
                assert eng.walker_form(W) != 2 and frag == int(form["kernel"] == 0), (n, W, eng.walker_form(W), frag)
            forms[W] = form
            got[W] = (eng.chi_squared(theta), eng.log_probability(theta))
        assert eng.info()["nonfinite_count"] == 0
    finally:
        if own:
            eng.close()
    # canonical bits: the largest batch holds every base row; its first occurrence of each
    W0 = max(W for W in got if W >= B)
    first = np.array([int(np.flatnonzero(S.batch_rows(W0, B) == b)[0]) for b in range(B)])
    canon = dict(chi2=_bits(got[W0][0])[first], logp=_bits(got[W0][1])[first])
    worst = {}
    for W, (chi2, logp) in got.items():
        _check_batch(n, W, "", forms[W], ref, canon, chi2, logp, worst)
    for (nn, kernel, pw), rel in sorted(worst.items()):
        print(f"N={nn} fixed_mu={fixed} kernel={'throughput' if kernel else 'small-batch'} panel width {pw}: worst relative error {rel:.2e}")
    _sweeps[(n, fixed)] = dict(canon=canon, worst=worst, forms=forms)
    return _sweeps[(n, fixed)]


@pytest.mark.parametrize("n", S.N_SMALL)
def test_default_batches_meet_the_reference_with_one_bit_pattern_per_row(gpu, n):
    sweep = _default_sweep(gpu, n)
    assert {f["kernel"] for f in sweep["forms"].values()} == {0, 1}


@pytest.mark.parametrize("n", S.N_FIXED_MU)
def test_generic_kernel_residuals_into_every_solve_form(gpu, n):
    """fixed_mu on every seventh SN: the generic walker_kernel writes the residuals in walker rows; both small-batch widths and both
    throughput widths read them.  Reference and one bit pattern per row as above; the handle reports row-ordered small batches."""
    sweep = _default_sweep(gpu, n, fixed=True)
    seen = {(f["kernel"], f["panel_width"], f["tpw"]) for f in sweep["forms"].values()}
    assert {(0, 16, 1), (0, 16, 2), (1, 16, 0), (1, 32, 0)} <= seen


@pytest.fixture(scope="module")
def workers(gpu, tmp_path_factory):
    return S.run_workers(S.TUNES, tmp_path_factory.mktemp("solve_forms"))


@pytest.mark.parametrize("n", S.N_SMALL)
def test_every_tune_string_gives_the_default_bits(gpu, workers, n):
    canon, ref = _default_sweep(gpu, n)["canon"], _reference(n, False)
    worst = {}
    for k, tune in enumerate(S.TUNES):
        r = workers[tune]
        for W in S.W_WORKER:
            form = S.form_dict(r[f"{n}:{W}:form"])
            S.check_forced(k, n, W, form)  # the knob took effect
            _check_batch(n, W, tune, form, ref, canon, r[f"{n}:{W}:chi2"], r[f"{n}:{W}:logp"], worst)


@pytest.fixture(scope="module")
def big_engine(gpu):
    S.data(S.N_LARGE)  # (the seeded data and its Cholesky factor are not part of the create time)
    t0 = time.perf_counter()
    eng = S.engine(gpu, S.N_LARGE)
    print(f"N={S.N_LARGE}: LikelihoodEngine created in {time.perf_counter() - t0:.2f} s")
    yield eng
    eng.close()


def test_factor_past_4096_shares(gpu, big_engine):
    """N = 4097, 65 row blocks: tri_gemm_small_kernel without the LDS staging of the last arriver's sums (via_lds false), and the
    throughput kernel one row past 64 row blocks."""
    t0 = time.perf_counter()
    sweep = _default_sweep(gpu, S.N_LARGE, eng=big_engine)
    print(f"N={S.N_LARGE}: sweep over W = {S.W_LARGE} in {time.perf_counter() - t0:.2f} s")
    assert {(f["kernel"], f["tpw"]) for f in sweep["forms"].values()} >= {(0, 1), (0, 2), (1, 0)}
    assert all(64 * f["n_rb"] > 4096 for f in sweep["forms"].values())


@pytest.mark.parametrize("W", [1793, 8193])
def test_device_entry_point_gives_the_host_calls_bits(gpu, W):
    import torch

    n = 449
    base = S.base_rows(n)
    theta = base[S.batch_rows(W, base.shape[0])]
    with S.engine(gpu, n) as eng:
        dev = torch.device("cuda:0")
        th = torch.from_numpy(theta).to(dev)
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        for kind, host in ((gpu.CF_OUT_CHI2, eng.chi_squared), (gpu.CF_OUT_LOGP, eng.log_probability)):
            want = host(theta)
            out = torch.full((W,), float("nan"), dtype=torch.float64, device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            eng.eval_device(th.data_ptr(), W, out.data_ptr(), kind, side.cuda_stream)
            side.synchronize()
            got = out.cpu().numpy()
            bad = np.flatnonzero(_bits(got) != _bits(want))
            assert bad.size == 0, f"N={n} W={W} kind={kind}: rows {bad[:8]} differ: {got[bad[:4]]} vs {want[bad[:4]]}, form {eng.solve_form(W)}"
    canon = _default_sweep(gpu, n)["canon"]
    assert np.array_equal(_bits(want), canon["logp"][S.batch_rows(W, base.shape[0])])
