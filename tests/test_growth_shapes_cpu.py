"""CPU: the cases of tests/growth_shapes.py and the bars of tests/test_gpu_growth_shapes.py are fair before anything runs on a GPU.

  conditions   for every case the restatement (tests/growth_reference.py) evaluated in float64 is within 1e-13 of its long-double
               self on the theory and on chi^2: the GPU bars (1e-12, 1e-10) ask for nothing float64 cannot give.  H(z) likewise:
               its float64 floor is stated and the GPU bar of cf_eval_hz is two orders above it.
  order        against scipy's DOP853 on the second-order equation the restatement's error falls 12-20 x per doubling of S:
               it is the fourth-order scheme the header describes, and at S = 1024 it sits where tests/test_fs8.py says the
               kernel sits against the five scripts' converged fixtures.
  sharpness    a dropped w_a z a term, 1 + z for a in the wCDM slope, half or twice the steps, interior slopes at a grid end and
               midpoint coefficients taken at the step start each move some case's theory by more than 100 GPU bars.
  reach        every value of every axis occurs at least twice and with different partners, every (MODEL, FDE, C) is launched,
               and the data hold the edges the module's docstring promises.
  refusals     cf_create turns the malformed growth blocks down before any device work (the same on a machine without a GPU).
"""
import collections

import numpy as np
import pytest

import derived_reference as R
import growth_reference as G
import growth_shapes as GS
from conftest import golden

LD = np.longdouble
THEORY_BAR, CHI2_BAR, HZ_BAR = 1e-12, 1e-10, 1e-13   # the GPU file's
IDS = [c.name for c in GS.CASES]


def _theory(b, S=None, dt=LD, defect=None, rows=slice(None)):
    c, f = b["case"], b["engine"]["fs8"]
    return G.theory(b["model"], b["theta"][rows], f["z"], a_init=c.a_init, S=S or c.S, n_agrid=c.a_grid, dt=dt, defect=defect)


def _rel(a, b):
    return float(np.max(np.abs(a.astype(LD) / b - 1)))


# ---- conditions ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", IDS)
def test_float64_can_meet_the_bars(pkg, name):
    b = GS.build(pkg, GS.BY_NAME[name])
    c, f = b["case"], b["engine"]["fs8"]
    assert _rel(_theory(b, dt=np.float64), _theory(b)) < 1e-13
    q = G.ap_factor(b["model"], b["theta"], f["z"], f["fid"])
    want = G.chi2(b["model"], b["theta"], f, S=c.S, q=q)
    if c.z0_exact:   # q = 0 at z = 0: chi^2 is not a number, on any side
        assert not np.isfinite(want.astype(np.float64)).any()
        return
    assert np.isfinite(want.astype(np.float64)).all() and (want > 0).all()
    assert _rel(G.chi2(b["model"], b["theta"], f, S=c.S, q=q, dt=np.float64), want) < 1e-13


def _scan_f64(M):
    """the step products in float64 in the association the kernel's header comment describes: the C steps of a lane multiplied
    together, an inclusive doubling scan over the 64 lanes of a wave, the earlier waves' totals folded in one by one (later
    steps on the left), then the lane's own steps again.  M [S, 2, 2] -> P [S + 1, 2, 2], P[i] = M[i - 1] ... M[0]."""
    S = M.shape[0]
    C = S // 256
    lane = M.reshape(256, C, 2, 2)[:, 0].copy()
    for j in range(1, C):
        lane = M.reshape(256, C, 2, 2)[:, j] @ lane
    incl, d = lane.copy(), 1
    while d < 64:
        take = (np.arange(256) % 64) >= d
        incl = np.where(take[:, None, None], incl @ np.roll(incl, d, axis=0), incl)
        d *= 2
    excl = np.roll(incl, 1, axis=0)
    excl[np.arange(256) % 64 == 0] = np.eye(2)
    for t in range(64, 256):
        for v in range(t // 64 - 1, -1, -1):
            excl[t] = excl[t] @ incl[64 * v + 63]
    out = np.empty((S + 1, 2, 2))
    for t in range(256):
        cur = excl[t]
        for j in range(C):
            out[C * t + j] = cur
            cur = M[C * t + j] @ cur
    out[S] = cur
    return out


@pytest.mark.parametrize("name", [c.name for c in GS.CASES if c.index < 16 or c.S == 2048])
def test_the_scan_association_fits_the_bar(pkg, name):
    """what the tree of 2 x 2 products costs in float64, measured on the host: delta' and delta at every step boundary from the
    scanned prefixes against the long-double sequential ones, for row 0.  The GPU bar is 1e-12."""
    b = GS.build(pkg, GS.BY_NAME[name])
    c = b["case"]
    x0, h, s, p, M = G.step_matrices(b["model"], b["theta"][:1], c.a_init, c.S, np.float64)
    got = _scan_f64(M[0]) @ np.array([c.a_init, 1.0])
    _, _, dprime, _, delta1 = G.integrate(b["model"], b["theta"][:1], c.a_init, c.S)
    assert _rel(got[:, 1], dprime[0]) < 1e-13 and _rel(got[-1:, 0], delta1) < 1e-13


def test_float64_floor_of_H_of_z(pkg):
    """cf_eval_hz is judged by derived_reference.H_of_z at 1e-13: two orders above what float64 arithmetic on the same
    expression loses (measured 3.3e-16 at most over the eight models, z up to 500; the bound asserted is 1e-15)."""
    worst = 0.0
    for case in GS.CASES[:8]:
        b = GS.build(pkg, case)
        m, th = b["model"], b["theta"][:1]
        z = GS.hz_redshifts(1000, b["engine"]["z_max"])
        _, c = R._cosmo(m, th)
        want = R.H_of_z(m, R._col(c), z.astype(LD))
        c64 = G._cast(R._col(c), np.float64)
        e2 = G.e2_and_slope(m, c64, 1.0 + z, np.float64)[0]
        assert e2.dtype == np.float64
        worst = max(worst, _rel(c64["H0"] * np.sqrt(e2), want))
        e2_ld = G.e2_and_slope(m, R._col(c), 1 + z.astype(LD))[0]   # the restatement's E^2 IS derived_reference's
        assert _rel(c["H0"][:, None] * np.sqrt(e2_ld), want) < 1e-18
    print(f"float64 floor of H(z): {worst:.1e}")
    assert worst < 1e-15 and HZ_BAR >= 100 * worst


# ---- order ---------------------------------------------------------------------------------------------------------------------
def _late(fde):
    params = dict(H0=("fixed", 70.0), Om=(0, 1.0), s8=(1, 1.0))
    if fde:
        params["w0"] = (2, 1.0)
    if fde == R.CPL:
        params["wa"] = (3, 1.0)
    return R.Model(ndim=4, params=params, z_max=3.0, fde=fde)


ORDER = [  # (a_init, fde, theta = (Om, sigma8, w0, wa))
    (10**-2.15, R.LCDM, (0.15, 0.8, 0.0, 0.0)),
    (10**-2.7, R.WCDM, (0.15, 0.8, -1.3, 0.0)),
    (10**-2.7, R.WCDM, (0.5, 0.8, -0.7, 0.0)),
    (10**-2.7, R.THAWING, (0.5, 0.8, -0.6, 0.0)),
    (10**-2.15, R.CPL, (0.5, 0.8, -0.8, -0.9)),
    (1 / 201, R.CPL, (0.15, 0.8, -1.2, 0.4)),
    (0.3, R.WCDM, (0.15, 0.8, -0.7, 0.0)),
]


@pytest.mark.parametrize("a_init,fde,theta", ORDER)
def test_fourth_order_against_the_converged_solution(a_init, fde, theta):
    m = _late(fde)
    th = np.array([theta])
    z = golden("fs8_fs8")["fs8_z"]   # the scripts' 56 redshifts, 0.001 .. 1.944
    truth = G.converged(m, th[0], z, a_init=a_init)
    err = {S: _rel(G.theory(m, th, z, a_init=a_init, S=S)[0], truth) for S in (256, 512, 1024, 2048)}
    print(f"a_init {a_init:.3g} fde {fde}: " + ", ".join(f"S={S} {e:.1e}" for S, e in err.items()))
    for S in (256, 512, 1024):
        if err[2 * S] > 1e-11:
            assert 12 < err[S] / err[2 * S] < 20, (S, err)
    assert err[2048] < 1e-10 and err[256] < 2e-7
    if fde == R.LCDM:   # the figures the sweep was planned with (1.1e-10 and 7.7e-12 at S = 1024 and 2048)
        assert 2e-8 < err[256] < 3.5e-8 and 1.0e-10 < err[1024] < 1.2e-10 and 7e-12 < err[2048] < 8.5e-12


def _fixture_cases():
    import test_fs8 as T
    return T.CASES, T.THEORY_VS_TIGHT


@pytest.mark.parametrize("name", ["fs8_fs8", "bao_desi_cmb_union3_fs8", "ohd_cc_fs8", "fs8_fs8_cmb", "bao_desi_fs_lya_cc_fs8"])
def test_restatement_reproduces_the_converged_fixtures(name):
    """... within THEORY_VS_TIGHT at the library's default 1024 steps on the script's own a-grid, and where tests/test_fs8.py
    says the kernel sits: its worst rows 2e-10 .. 3e-10 away (measured here: 4e-11 .. 2.4e-10 per fixture)."""
    cases, bar = _fixture_cases()
    g = golden(name)
    m = GS.model_of_oracle(cases[name](g))
    nt, span = len(g["theory"]), g["a_span"]
    t = G.theory(m, g["thetas"][:nt], g["fs8_z"], a_init=float(span[0]), S=1024, n_agrid=len(span))
    gap = _rel(t, g["theory_tight"].astype(LD))
    print(f"{name}: {gap:.1e}")
    assert gap < bar and gap < 3e-10
    if name in ("bao_desi_cmb_union3_fs8", "ohd_cc_fs8"):
        assert gap > 2e-10
    half = G.theory(m, g["thetas"][:nt], g["fs8_z"], a_init=float(span[0]), S=512, n_agrid=len(span))
    assert _rel(half, g["theory_tight"].astype(LD)) > 4e-10   # a wrong S is visible even at the fixtures' own bar's scale


# ---- sharpness -----------------------------------------------------------------------------------------------------------------
def _moved(pkg, defect=None, S_factor=None, select=lambda c: True):
    best = 0.0
    for case in GS.CASES:
        if not select(case):
            continue
        b = GS.build(pkg, case)
        rows = slice(0, min(case.W, 3))
        if defect is not None:
            got = _theory(b, defect=defect, rows=rows)
        else:
            got = _theory(b, S=int(case.S * S_factor), rows=rows)
        best = max(best, _rel(got, _theory(b, rows=rows)))
    return best


@pytest.mark.parametrize("defect,select", [
    ("cpl_drop_wa_za", lambda c: c.fde == R.CPL and c.index < 32),
    ("wcdm_zp1_for_a", lambda c: c.fde == R.WCDM and c.index < 32),
    ("interior_slopes_at_ends", lambda c: c.a_grid > 0 and c.n_fs8 >= 56 and c.index < 32),
    ("midpoint_at_step_start", lambda c: c.index < 8),
])
def test_the_bar_sees_a_wrong_formula(pkg, defect, select):
    moved = _moved(pkg, defect=defect, select=select)
    print(f"{defect}: moves the theory by {moved:.1e}")
    assert moved > 100 * THEORY_BAR


@pytest.mark.parametrize("factor", [0.5, 2])
def test_the_bar_sees_a_wrong_step_count(pkg, factor):
    moved = _moved(pkg, S_factor=factor, select=lambda c: c.index < 16 and 256 < c.S < 2048)
    print(f"{factor} x the steps: moves the theory by {moved:.1e}")
    assert moved > 100 * THEORY_BAR


@pytest.mark.parametrize("name", [c.name for c in GS.ROUNDING])
def test_rounding_cases_tell_the_two_schemes_apart(pkg, name):
    """a request of 257 / 513 / 1025 steps must run 512 / 1024 / 2048: the GPU file wants the theory within 1e-12 of that scheme
    and MORE than 1e-10 from the one below, which the two schemes themselves must allow: they are 1.2e-10 or more apart, twenty
    times the 1e-12 the kernel may use up"""
    b = GS.build(pkg, GS.BY_NAME[name])
    c = b["case"]
    assert c.S == 2 * (c.steps - 1) and G.effective_steps(c.steps) == c.S
    assert _rel(_theory(b, S=c.S // 2), _theory(b)) > 1.2e-10


# ---- reach ---------------------------------------------------------------------------------------------------------------------
def test_every_axis_value_occurs_twice_with_different_partners():
    axes = {"pair": lambda c: (c.ez_model, c.fde), "steps": lambda c: c.steps, "n_fs8": lambda c: c.n_fs8,
            "a_init": lambda c: c.a_init, "a_grid": lambda c: c.a_grid, "block": lambda c: c.block, "W": lambda c: c.W}
    want = {"pair": GS.PAIRS, "steps": GS.STEPS_REQUESTED, "n_fs8": GS.N_FS8, "a_init": GS.A_INIT, "a_grid": GS.A_GRID,
            "block": GS.BLOCKS, "W": GS.WALKERS}
    assert 40 <= len(GS.CASES) <= 60
    for ax, get in axes.items():
        seen = collections.defaultdict(list)
        for c in GS.CASES:
            seen[get(c)].append(c)
        assert set(seen) == set(want[ax]), ax
        for value, cs in seen.items():
            assert len(cs) >= 2, (ax, value)
            for other, get_other in axes.items():
                if other != ax:
                    assert len({get_other(c) for c in cs}) >= 2, (ax, value, other)
    assert {(c.ez_model, c.fde, c.C) for c in GS.CASES} == {(m, f, C) for m, f in GS.PAIRS for C in (1, 2, 4, 8)}
    assert all(any(c.steps == s and c.S == e for c in GS.CASES) for s, e in zip(GS.STEPS_REQUESTED, GS.STEPS_EFFECTIVE))
    assert all(G.effective_steps(c.steps) == c.S for c in GS.CASES)
    assert {c.ferr_free for c in GS.CASES} == {True, False} and {c.n_grid for c in GS.CASES} == {513, 4000}
    exact = [c for c in GS.CASES if c.z0_exact]
    assert len(exact) >= 2 and len({c.a_grid for c in exact}) >= 2 and len({c.n_fs8 for c in exact}) >= 2


def test_dark_energy_rows_are_on_both_sides(pkg):
    w0, wa = collections.defaultdict(set), set()
    for case in GS.CASES:
        if case.fde:
            b = GS.build(pkg, case)
            names = GS.names_of(case)
            w0[case.fde].add(float(b["theta"][0, names.index("w0")]))
            if case.fde == R.CPL:
                wa.add(float(b["theta"][0, names.index("wa")]))
    assert min(w0[R.WCDM]) < -1 < max(w0[R.WCDM]) and all(w != -1 for w in w0[R.THAWING]) and len(w0[R.THAWING]) >= 2
    assert min(wa) < 0 < max(wa)


@pytest.mark.parametrize("name", IDS)
def test_the_data_hold_the_promised_edges(pkg, name):
    b = GS.build(pkg, GS.BY_NAME[name])
    c, f, th, box = b["case"], b["engine"]["fs8"], b["theta"], b["engine"]["bounds"]
    z = f["z"]
    a = 1.0 / (1.0 + z)
    assert z.size == c.n_fs8 and np.all(z >= 0) and np.all(a >= c.a_init) and np.all(f["fid"] > 0)
    assert np.all(np.linalg.eigvalsh(f["inv_cov"]) > 0) and np.abs(f["inv_cov"]).min() > 0   # dense, positive definite
    inside = np.all((box[:, 0] < th) & (th < box[:, 1]), axis=1)
    assert inside[0] and (c.W < 3 or (not inside[1] and inside[3 if c.W > 3 else 0]))
    if c.ferr_free:
        assert np.all(th[:, GS.names_of(c).index("fs8err")] != 1) and abs(th[0, GS.names_of(c).index("fs8err")] - 1) > 1e-2
    for zz in b["z_at"], z:
        if zz.size > 2:
            assert np.any(np.diff(zz) < 0) and np.any(np.diff(zz) > 0)   # unsorted
    assert b["z_at"][1] == 0.0 and 1.0 / (1.0 + b["z_at"][0]) >= c.a_init > 1.0 / (1.0 + np.nextafter(b["z_at"][0], np.inf))
    if c.n_fs8 < 4:
        return
    assert np.sum(a == 1.0) == 1 and (0.0 in z) == c.z0_exact
    edge = z.max()
    assert 1.0 / (1.0 + edge) >= c.a_init and not 1.0 / (1.0 + np.nextafter(edge, np.inf)) >= c.a_init
    assert z.size - np.unique(z).size == 1                                  # one duplicate pair
    x0 = np.log(c.a_init)
    pos = (np.log(a) - x0) / (-x0 / c.S)                                    # in steps
    on_boundary = np.abs(pos - np.rint(pos)) < 1e-9
    inner = on_boundary & (np.rint(pos) > 0) & (np.rint(pos) < c.S)
    assert inner.sum() >= 2
    if c.n_fs8 >= 5:
        assert np.any(inner & (np.rint(pos) % c.C == 0)) and (c.C == 1 or np.any(inner & (np.rint(pos) % c.C != 0)))
    if c.n_fs8 >= 56:
        lanes = GS.step_of(a[~on_boundary], c.a_init, c.S) // c.C
        assert set(lanes // 64) == {0, 1, 2, 3}
        if c.a_grid:
            nodes = G.a_grid(c.a_init, c.a_grid)
            assert nodes[-1] == 1.0 and np.isin(a, nodes[1:-1]).any()
            i = np.clip(np.searchsorted(nodes, a, side="left") - 1, 0, len(nodes) - 2)
            assert 0 in i and len(nodes) - 2 in i
            li, flags = GS.window_of(a, nodes)
            got = set(zip(li.tolist(), flags.tolist()))
            if c.a_grid == 4:
                assert got == {(0, 3), (1, 3), (2, 3)}
            elif c.a_grid == 5:
                assert {fl for _, fl in got} == {1, 2} and {(0, 1), (2, 2)} <= got
            else:
                assert {fl for _, fl in got} == {0, 1, 2} and {(0, 1), (2, 2), (1, 0)} <= got


def test_small_a_grids_are_reached_with_many_data():
    for n_agrid in (4, 5, 7, 1000):
        assert sum(1 for c in GS.CASES if c.a_grid == n_agrid and c.n_fs8 >= 56) >= 2, n_agrid


# ---- refusals: before any device work -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("change,message", [
    (dict(steps=2049), "fs8_steps"), (dict(steps=-1), "fs8_steps"), (dict(a_grid=1), "fs8_n_agrid"), (dict(a_grid=3), "fs8_n_agrid"),
    (dict(a_init=0.0), "fs8_a_init"), (dict(a_init=1.0), "fs8_a_init"), ("below_a_init", "a_init <= a <= 1"), ("n65", "n_fs8"),
])
def test_cf_create_refuses_a_malformed_growth_block(pkg, change, message):
    b = GS.build(pkg, GS.CASES[9])   # growth alone, 64 data
    kw = dict(b["engine"])
    fs8 = dict(kw["fs8"])
    if change == "below_a_init":
        fs8["z"] = fs8["z"].copy()
        fs8["z"][np.argmax(fs8["z"])] = np.nextafter(fs8["z"].max(), np.inf)   # one ulp beyond the accepted edge
    elif change == "n65":
        fs8.update(z=np.append(fs8["z"], 0.5), val=np.append(fs8["val"], 0.4), fid=np.append(fs8["fid"], 1.0), inv_cov=np.eye(65))
    else:
        fs8.update(change)
    kw["fs8"] = fs8
    with pytest.raises(pkg.CosmofitError, match=f"CF_ERR_INVALID.*{message}"):
        pkg.LikelihoodEngine(**kw)
