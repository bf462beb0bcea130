"""GPU (-m gpu): the prior / output epilogue (finalize_value, csrc/cosmofit_kernels.hip) through every kernel that applies it at a
small size -- finalize_kernel, trsm_chi2_kernel, tri_gemm_small_kernel with one and two threads per walker, tri_gemm_chi2_kernel's
panel_last_arriver<1> and <2> -- with every field of cf_epilogue filled to its limit (tests/epilogue_shapes.py), against the
long-double restatement of the Python reference (tests/epilogue_reference.py).

For every case, route, W and the three output kinds, through the host entry points and through eval_device on a side stream:
* route      the engine reports the solve mode, and cf_solve_form the (kernel, panel width, threads per walker), that W is listed under;
* paths      eval_device gives the host call's bits;
* position   every occurrence of a base row in a batch has one bit pattern;
* exact      -inf exactly where the reference says, NaN in chi^2 exactly on the NaN rows, finite everywhere else, no row skipped;
* counter    nonfinite_count grows per evaluation by exactly the number of rows the reference counts (log L and log P differ: log L
             has no box), by 0 for chi^2;
* epilogue   with c = the engine's own plain chi^2 of the row (a twin engine without priors, bounds, wall or Gaussian terms, same
             route and W): |got - finalize(case, row, c, kind)| <= 2^-52 (T + 4) sum |term| + n 2 2^-52 max(1, |ln f|) per logarithm
             (epilogue_reference.bound) -- this judges only what finalize_value adds to c; wall rows (lp - 1e8) included;
* end to end chi^2 and log P within the project's 1e-10 of oracle_np, for the cases it can state (no growth block, no quasars).
The worst ratio to the bound per route is printed and recorded in profiles/NOTES_epilogue.md."""
import functools

import numpy as np
import pytest

import epilogue_reference as ER
import epilogue_shapes as S
from oracle import oracle_np as onp

pytestmark = pytest.mark.gpu
RTOL = 1e-10
LD = np.longdouble
PAIRS = [(name, route) for name, case in S.CASES.items() for route in case["routes"]]
_worst = {}  # route of ROUTE_TABLE -> (ratio to the bound, where)


@pytest.fixture(scope="module")
def gpu(pkg):
    if pkg.lib().cf_device_count() < 1:
        pytest.fail("GPU tests need an MI355X; no HIP device visible (there is no fallback path)")
    return pkg


def _bits(a):
    """Bit patterns with every NaN mapped to one (a NaN's payload is not part of the result)."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    return np.where(np.isnan(a), np.float64(np.nan), a).view(np.uint64)


def _label(route, W):
    return next(lab for lab, r, ws in S.ROUTE_TABLE if r == route and W in ws)


def _check_route(gpu, eng, route, W):
    info = eng.info()
    if route == "finalize":
        assert eng.n_sn == 0, "finalize_kernel is the route of an engine without an SN block"
        return
    assert info["solve_mode"] == gpu.engine.solve_mode_of(route), (route, info["solve_mode"])
    if route == "inverse":
        form = eng.solve_form(W)
        assert (form["kernel"], form["panel_width"], form["tpw"]) == S.INVERSE_FORMS[W], f"W={W} is listed under {S.INVERSE_FORMS[W]}: {form}"


_sweeps = {}


def _sweep(gpu, name, route):
    """Every W of the route on the case's engine and on its twin (once per process) ->
    {W: dict(host, dev: {kind: [W]}, counted: {(path, kind): growth of nonfinite_count}, c: {kind: [W] the twin's plain chi^2})}."""
    if (name, route) in _sweeps:
        return _sweeps[(name, route)]
    import torch

    case, base = S.CASES[name], S.base_rows(name)
    kinds = {ER.CHI2: gpu.CF_OUT_CHI2, ER.LOGL: gpu.CF_OUT_LOGL, ER.LOGP: gpu.CF_OUT_LOGP}
    dev = torch.device("cuda:0")
    side = torch.cuda.Stream(dev)
    out = {}
    with gpu.LikelihoodEngine(**S.engine_kwargs(gpu, name, route)) as eng, gpu.LikelihoodEngine(**S.twin_kwargs(gpu, name, route)) as twin:
        for W in S.W_LIST[route]:
            _check_route(gpu, eng, route, W)
            _check_route(gpu, twin, route, W)
            theta = np.ascontiguousarray(base[S.batch_rows(W)])
            th = torch.from_numpy(theta).to(dev)
            res = dict(host={}, dev={}, counted={})
            host = {ER.CHI2: eng.chi_squared, ER.LOGL: eng.log_likelihood, ER.LOGP: eng.log_probability}
            for kind, code in kinds.items():
                n0 = eng.info()["nonfinite_count"]
                res["host"][kind] = host[kind](theta)
                n1 = eng.info()["nonfinite_count"]
                buf = torch.full((W,), 12345.0, dtype=torch.float64, device=dev)  # a row skipped keeps this
                side.wait_stream(torch.cuda.current_stream(dev))
                eng.eval_device(th.data_ptr(), W, buf.data_ptr(), code, side.cuda_stream)
                side.synchronize()
                res["dev"][kind] = buf.cpu().numpy()
                res["counted"]["host", kind], res["counted"]["dev", kind] = n1 - n0, eng.info()["nonfinite_count"] - n1
            c = twin.chi_squared(theta)
            # the quasar kernel adds sum ln(sigma^2 + s^2) to the chi^2 of log L / log P: -2 log L of the twin (exact: x -0.5, + 0)
            c_l = -2.0 * twin.log_likelihood(theta) if case["quasar"] else c
            res["c"] = {ER.CHI2: c, ER.LOGL: c_l, ER.LOGP: c_l}
            out[W] = res
    _sweeps[(name, route)] = out
    return out


@functools.lru_cache(maxsize=None)
def _walk(name, kind, r, c_bits):
    return ER.walk(S.CASES[name], S.base_rows(name)[r], np.uint64(c_bits).view(np.float64), kind)


def _per_row(name, route, W, kind, values, what):
    """[41] the one value of each base row in the batch (asserted: one bit pattern per base row), NaN where W < 41 leaves it out."""
    rows = S.batch_rows(W)
    bits = _bits(values)
    first = np.full(S.B, -1)
    first[rows[::-1]] = np.arange(W)[::-1]
    bad = np.flatnonzero(bits != bits[first[rows]])
    assert bad.size == 0, (f"{name} {route} W={W} {kind}: {what} of walker {bad[0]} (base row {rows[bad[0]]}, lane {bad[0] % S.panel_width(route, W)} "
                           f"of panel {bad[0] // S.panel_width(route, W)}) is {values[bad[0]]!r}, of walker {first[rows[bad[0]]]} {values[first[rows[bad[0]]]]!r}")
    return first


@pytest.mark.parametrize("name,route", PAIRS)
def test_route_paths_and_position(gpu, name, route):
    """The route is the one listed; eval_device gives the host call's bits; a base row has one bit pattern wherever it sits."""
    for W, res in _sweep(gpu, name, route).items():
        for kind in ER.KINDS:
            host, dev = res["host"][kind], res["dev"][kind]
            assert host.shape == dev.shape == (W,)
            bad = np.flatnonzero(_bits(host) != _bits(dev))
            assert bad.size == 0, f"{name} {route} W={W} {kind}: eval_device differs from the host call in rows {bad[:8]}: {dev[bad[:4]]} vs {host[bad[:4]]}"
            _per_row(name, route, W, kind, host, "the result")
            _per_row(name, route, W, kind, res["c"][kind], "the twin's plain chi^2")


@pytest.mark.parametrize("name,route", PAIRS)
def test_exact_results_and_counter(gpu, name, route):
    case = S.CASES[name]
    nan_rows = S.nan_chi2_rows(name)
    for W, res in _sweep(gpu, name, route).items():
        rows = S.batch_rows(W)
        c = res["c"]
        assert np.array_equal(np.isnan(c[ER.CHI2]), nan_rows[rows]), f"{name} {route} W={W}: the twin's chi^2 is not NaN exactly on the NaN rows"
        assert np.array_equal(~np.isfinite(c[ER.LOGL]), nan_rows[rows])
        for kind in ER.KINDS:
            got = res["host"][kind]
            w = [_walk(name, kind, int(r), int(_bits(c[kind][i:i + 1])[0])) for i, r in enumerate(rows)]
            ctx = f"{name} {route} W={W} {kind}"
            want_neginf = np.array([np.isneginf(x["value"]) for x in w])
            bad = np.flatnonzero(np.isneginf(got) != want_neginf)
            assert bad.size == 0, f"{ctx}: -inf rows differ at walkers {bad[:8]} (base rows {rows[bad[:8]]}): got {got[bad[:4]]}, reference {[w[i]['reason'] for i in bad[:4]]}"
            want_nan = nan_rows[rows] if kind == ER.CHI2 else np.zeros(W, dtype=bool)
            bad = np.flatnonzero(np.isnan(got) != want_nan)
            assert bad.size == 0, f"{ctx}: NaN rows differ at walkers {bad[:8]} (base rows {rows[bad[:8]]}): {got[bad[:4]]}"
            assert np.all(np.isfinite(got[~want_neginf & ~want_nan])), ctx
            wall = np.array([x["reason"] == "wall" for x in w])
            assert np.all((got[wall] < -0.9e8) & (got[wall] > -1.1e8)), f"{ctx}: wall rows {got[wall][:4]}"
            if W >= S.B:  # every base row is in the batch: the wall rows are met wherever there is a wall
                assert wall.any() == (case["cpl_wall"] and kind != ER.CHI2), ctx
            counted = sum(x["counted"] for x in w)
            assert kind != ER.CHI2 or counted == 0
            for path in ("host", "dev"):
                assert res["counted"][path, kind] == counted, f"{ctx} ({path}): nonfinite_count grew by {res['counted'][path, kind]}, the reference counts {counted} rows"


@pytest.mark.parametrize("name,route", PAIRS)
def test_epilogue_on_its_own_within_the_rounding_bound(gpu, name, route):
    for W, res in _sweep(gpu, name, route).items():
        for kind in ER.KINDS:
            got, c = res["host"][kind], res["c"][kind]
            first = _per_row(name, route, W, kind, got, "the result")
            for r in np.flatnonzero(first >= 0):
                i = first[r]
                w = _walk(name, kind, int(r), int(_bits(c[i:i + 1])[0]))
                if not np.isfinite(w["value"]):
                    continue  # (judged exactly in test_exact_results_and_counter)
                err, bound = abs(LD(got[i]) - w["value"]), ER.bound(w)
                ratio = float(err / bound) if bound > 0 else (0.0 if err == 0 else np.inf)
                lab = _label(route, W)
                if ratio > _worst.get(lab, (-1.0, ""))[0]:
                    _worst[lab] = (ratio, f"{name} W={W} {kind} base row {r} ({w['reason']})")
                assert err <= bound, (f"{name} {route} W={W} {kind} base row {r} (walker {i}, {w['reason']}): got {got[i]!r}, reference {w['value']!r} "
                                      f"from c = {c[i]!r}: error {float(err):.3e} is {ratio:.2f} x the bound {float(bound):.3e}")
    print(f"{name} {route}: worst ratio to the bound so far per route: " + "; ".join(f"{k}: {v[0]:.3f}" for k, v in sorted(_worst.items())))


@functools.lru_cache(maxsize=None)
def _oracle(name):
    lk = S.oracle_likelihood(name)
    with np.errstate(all="ignore"):
        return (np.array([onp.chi_squared(lk, row) for row in S.base_rows(name)]),
                np.array([onp.log_probability(lk, row) for row in S.base_rows(name)]))


@pytest.mark.parametrize("name,route", [p for p in PAIRS if p[0] in S.ORACLE_CASES])
def test_end_to_end_against_the_oracle(gpu, name, route):
    chi2, logp = _oracle(name)
    for W, res in _sweep(gpu, name, route).items():
        rows = S.batch_rows(W)
        for kind, want in ((ER.CHI2, chi2[rows]), (ER.LOGP, logp[rows])):
            got = res["host"][kind]
            ok = np.isfinite(want)
            rel = np.abs(got[ok] - want[ok]) / np.abs(want[ok])
            assert np.all(np.isfinite(got[ok])) and (rel.size == 0 or rel.max() < RTOL), \
                f"{name} {route} W={W} {kind}: worst relative error {np.nanmax(rel):.3e} at walker {np.flatnonzero(ok)[np.nanargmax(rel)]}"
            if kind == ER.LOGP:  # outside the box the oracle has -inf too; where its log L is NaN the product has -inf
                assert np.all(np.isneginf(got[~ok])), f"{name} {route} W={W}: {got[~ok][:4]}"


def test_worst_ratio_per_route_report(gpu):
    """Not an assertion of its own: prints what the bound test measured on every route of the table (run after it in file order)."""
    for lab, _, ws in S.ROUTE_TABLE:
        ratio, where = _worst.get(lab, (float("nan"), "not run"))
        print(f"{lab} (W = {ws}): worst |got - reference| / bound = {ratio:.3f} at {where}")
    assert not _worst or set(_worst) == {lab for lab, _, _ in S.ROUTE_TABLE}
