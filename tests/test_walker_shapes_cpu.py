"""CPU: the long-double residual reference of the per-walker SN stage (tests/walker_reference.py) agrees with the float64 oracle
(oracle/oracle_np.py: sn_parts) on every case of the sweep (tests/walker_shapes.py) under 1e-13 + B env with B <= 2; the
fragment-order formula the GPU test un-permutes with is a bijection of a panel; the sweep covers what it is there for (models,
grids, both outcomes of the streaming guard, the node boundaries, the BAO stencils) and meets the two conditions its tolerance
rests on; cf_last_residuals reports its argument errors without a device.

env_i = 2^-52 (5 / ln 10) (1 + z_i) / |z_cosmo_i| is what one ulp of 1 + z in z_cosmo moves a residual by; the GPU test's tolerance
is 1e-12 + 4 env (tests/test_gpu_walker_shapes.py)."""
import ctypes as C

import numpy as np
import pytest

import walker_shapes as S

LD = np.longdouble
ORACLE_FLOOR, ORACLE_B_MAX = LD(1e-13), 2.0


@pytest.mark.parametrize("name", S.CHI2_CASES)
def test_reference_agrees_with_the_float64_oracle(name):
    ref, got = S.reference(name), S.oracle_values(name)["delta"]
    full = ~ref["class_only"]
    assert np.all(np.isfinite(ref["delta"][full].astype(np.float64))), "a fully compared pair is not finite in the reference"
    # compared by class: the reference is not finite exactly where the oracle is not (z_cosmo <= 0: log10 of a distance <= 0; NaN row)
    assert np.array_equal(np.isfinite(got), np.isfinite(ref["delta"].astype(np.float64))), name
    if _has_v(name):
        assert not np.isfinite(ref["delta"][ref["class_only"]].astype(np.float64)).any()
    err = np.abs(got.astype(LD) - ref["delta"])[full]
    B = float(np.max((err - ORACLE_FLOOR) / ref["env"][full])) if err.size else 0.0
    print(f"{name}: {int(full.sum())} pairs, oracle worst |err| {float(err.max()):.2e}, B = {B:.3f}")
    assert B <= ORACLE_B_MAX, f"{name}: the float64 oracle needs B = {B:.3f} in 1e-13 + B env"


def _has_v(name):
    return S.CASES[name]["form"] in ("pm1", "weights")


@pytest.mark.parametrize("n_ld", [64, 128, 576])
def test_fragment_order_is_a_bijection_of_a_panel(n_ld):
    w, i = np.meshgrid(np.arange(16), np.arange(n_ld), indexing="ij")
    idx = S.frag_index(w, i, n_ld)
    assert np.array_equal(np.sort(idx.ravel()), np.arange(16 * n_ld))
    # a second panel is the first one, 16 n_ld doubles on
    assert np.array_equal(S.frag_index(w + 16, i, n_ld), idx + 16 * n_ld)
    # and rows_of_buffer undoes it
    buf = np.zeros(32 * n_ld)
    W = 21
    ww, ii = np.meshgrid(np.arange(W), np.arange(n_ld), indexing="ij")
    buf[S.frag_index(ww, ii, n_ld)] = 1000.0 * ww + ii
    assert np.array_equal(S.rows_of_buffer(buf, 1, W, n_ld - 3), 1000.0 * ww + ii)
    assert np.array_equal(S.rows_of_buffer((1000.0 * ww + ii).ravel().tolist() + [0.0] * ((32 - W) * n_ld), 0, W, n_ld - 3),
                          1000.0 * ww + ii)


def test_case_set_covers_models_grids_and_forms():
    cases = S.CASES.values()
    assert {(c["ez_model"], c["fde"]) for c in cases if c["group"] == "model"} == {(m, f) for m in (0, 1) for f in range(4)}
    for c in cases:
        if c["group"] == "model":
            assert (c["n_sn"], c["n_grid"], c["form"]) == (130, 1000, "pm1")
    for tag in ("thawing", "physwcdm"):
        assert {c["n_grid"] for c in cases if c["group"] == "grid" and tag in c["name"]} == set(S.GRIDS)
        assert {c["n_grid"] for c in cases if c["group"] == "grid_generic" and tag in c["name"]} == set(S.GRIDS_GENERIC)
    assert {(c["form"], c["n_sn"]) for c in cases if c["group"] == "form"} == {(f, n) for f in S.SN_FORMS for n in S.N_SN_SET}
    assert {c["n_grid"] for c in cases if c["group"] == "edges"} == {1000, 4096}
    assert all(S.streamable(n) == (c["group"] != "grid_generic") for n, c in S.CASES.items())
    assert all(c["n_sn"] <= 513 for c in cases) and len(S.CASES) == len(S.RESIDUAL_CASES) + 2


@pytest.mark.parametrize("name", list(S.CASES))
def test_rows_and_guard(name):
    case, th, sn = S.CASES[name], S.rows(name), S.sn_data(name)
    assert th.shape == (S.N_ROWS, S.NDIM)
    ordinary = np.setdiff1d(np.arange(S.N_ROWS), S.SPECIAL_ROWS)
    assert np.all((S.BOUNDS[:, 0] < th[ordinary]) & (th[ordinary] < S.BOUNDS[:, 1])) and ordinary.size == 27
    assert th[S.ROW_WA_ZERO, 6] == 0.0 and np.isnan(th[S.ROW_NAN, S.COL_V]) and th[S.ROW_OOB, 1] > S.BOUNDS[1, 1]
    assert np.all(th[:, 5] + np.nan_to_num(th[:, 6]) <= 0.0)
    z = sn["z_cmb"]
    assert z.size == case["n_sn"] and np.all(z[z < S.Z_SN_MIN] > 0)
    if not case["edges"]:
        assert z.min() >= S.Z_SN_MIN and abs(S.Z_SN_MIN / (300.0 / S.C_KM_S) - 4) < 0.01  # four times the largest in-box |z_pec|
    fast = S.fast_path(name)
    has_v = case["form"] in ("pm1", "weights")
    assert not fast[S.ROW_NAN] or not has_v
    assert fast[ordinary].all(), "an in-box row fails the guard"
    if has_v and case["n_grid"] > S.SEG:  # a multi-segment grid: both outcomes, on either side of the bound
        a, shift = S.shift_bound(name, th[:, S.COL_V])
        assert fast[S.ROW_IN] and not fast[S.ROW_OUT] and not fast[S.ROW_FAR]
        assert 0 < S.GUARD_NODES - shift[S.ROW_IN] < 1e-6 and 0 < shift[S.ROW_OUT] - S.GUARD_NODES < 1e-6
        assert shift[S.ROW_FAR] > 2 * S.GUARD_NODES and a[S.ROW_FAR] <= S.A_FAR_CAP  # three times the bound, or the cap (one SN)
    if has_v:  # ROW_ZNEG does what it is there for: the lowest SN, and in the ordinary cases nothing else
        ref = S.reference(name)
        low = int(np.argmin(z))
        assert ref["nonpos"][S.ROW_ZNEG, low]
        if not case["edges"]:
            assert ref["nonpos"][S.ROW_ZNEG].sum() == 1


def test_every_multi_segment_grid_sees_both_guard_outcomes():
    grids = {}
    for name, c in S.CASES.items():
        if S.streamable(name) and c["n_grid"] > S.SEG:
            grids.setdefault(c["n_grid"], set()).update(S.fast_path(name).tolist())
    assert set(grids) == {513, 1000, 1024, 1025, 1100, 3585, 4095, 4096}
    assert all(v == {True, False} for v in grids.values()), grids


@pytest.mark.parametrize("name", ["edges_g1000", "edges_g4096"])
def test_edges_cases_sit_at_the_boundaries(name):
    case, z, zg = S.CASES[name], S.sn_data(name)["z_cmb"], S.grid_of(name)
    G, step = case["n_grid"], S.grid_of(name)[1]
    assert 2.4e-3 < step < 2.41e-3
    for n in S.EDGE_NODES:
        zn = zg[n]
        d = (z - zn) / step
        assert np.any(np.abs(d) < 1.0), f"no SN within one node of node {n}"
        if n != 0:
            for lo, hi in ((-1.1e-3, -0.9e-3), (0.9e-3, 1.1e-3)):
                assert np.any((d > lo) & (d < hi)), f"node {n}: no SN 1e-3 of a spacing away"
            assert np.nextafter(zn, -np.inf) in z and np.nextafter(zn, np.inf) in z
    assert case["z_max"] in z and np.any(z > case["z_max"] * 1.01)
    assert all(v in z for v in S.Z_LOW) and np.sum(z < S.Z_SN_MIN) == 2 + 4  # the two low SNe and the four next to node 1
    # the segment each SN is packed for, restated from cf_stream_node / cf_stream_segment
    n_seg = (G + S.SEG - 1) // S.SEG
    node = np.where(z >= case["z_max"], G - 2, np.minimum((z * ((G - 1) / case["z_max"])).astype(int), G - 2))
    seg = np.minimum((node + S.HALO // 2) // S.SEG, n_seg - 1)
    if G == 4096:
        assert S.EMPTY_SEGMENT not in seg and set(seg) == set(range(8)) - {S.EMPTY_SEGMENT}
    else:
        assert set(seg) == {0, 1}


def test_aux_case_stencils():
    st, G = S.bao_stencils("aux_physical_cpl"), S.CASES["aux_physical_cpl"]["n_grid"]
    assert G == 1100 and st.shape == (8, 2)
    assert st[0, 0] == 0 and st[3, 1] == G - 1
    assert st[1, 0] < 512 <= st[1, 1] and st[2, 0] < 1024 <= st[2, 1]


@pytest.mark.parametrize("name", S.RESIDUAL_CASES)
def test_tolerance_conditions(name):
    """(a) 1e-12 + 4 env exceeds 2e-12 only for pairs of the two SNe at z <= 5e-4.  (b) pairs compared by class only because
    z_cosmo <= 0 are at most 2 % of the case's pairs -- not counting the NaN row, which is 1 / 33 of every case by construction,
    and the one pair ROW_ZNEG exists to make (with one SN it is 1 / 33 as well) -- and 25 in-box rows are compared in full."""
    ref, z = S.reference(name), S.sn_data(name)["z_cmb"]
    finite_rows = ~ref["bad_row"]
    full = ~ref["class_only"]
    wide = full & (ref["tol"] > LD(2e-12))
    assert not wide[:, z > 5e-4].any(), f"(a): tolerance above 2e-12 at SNe {np.unique(np.nonzero(wide[:, z > 5e-4])[1])}"
    nonpos = ref["nonpos"] & finite_rows[:, None]
    nonpos[S.ROW_ZNEG, int(np.argmin(z))] = False
    assert nonpos.sum() <= 0.02 * nonpos.size, f"(b): {int(nonpos.sum())} of {nonpos.size} pairs have z_cosmo <= 0"
    in_box_full = finite_rows & ~ref["out_of_box"] & full.all(axis=1)
    assert in_box_full.sum() >= 25, f"(b): {int(in_box_full.sum())} in-box rows are compared in full"
    assert ref["bad_row"].sum() == 1 and ref["bad_row"][S.ROW_NAN]
    assert ref["out_of_box"][S.ROW_OOB] and ref["out_of_box"].sum() >= 1


def test_last_residuals_reports_argument_errors(pkg):
    lib, L = pkg.lib(), pkg._lib
    assert "cf_last_residuals" in L.EXPORTS
    buf, layout = np.zeros(64 * 48), C.c_int32(7)
    assert lib.cf_last_residuals(None, 33, buf.ctypes.data_as(C.c_void_p), C.byref(layout)) == -1  # CF_ERR_INVALID, as cf_walker_form
    assert b"cf_last_residuals" in lib.cf_last_error() and layout.value == 7 and not buf.any()
    assert lib.cf_last_residuals(None, 33, None, None) == -1
    assert lib.cf_walker_form(None, 33) == -1
    assert [S.expected_form("model_late_lcdm", m) for m in S.FORMS] == [(1, 0), (0, 1), (0, 0), (2, 0)]
    assert {S.expected_form("gridgen_thawing_g8192", m) for m in S.FORMS} == {(2, 0)}
