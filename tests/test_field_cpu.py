"""CPU: the extended-precision restatement of field.py against the fixture made by running the script itself, the status rule
and monotonicity on the rows of the GPU tests, cf_field's argument checks (before any HIP call), Model.from_recipe and the
argument checks and chunk arithmetic of quintessence.bands."""
import ctypes as C

import numpy as np
import pytest

import field_reference as fr
import field_shapes as fs
from conftest import golden


@pytest.fixture(scope="module")
def fixture_rows():
    g = golden("field")
    nodes = g["nodes"]
    a_nodes = np.linspace(1e-8, 5, 5000)[nodes]
    refs = [fr.row("thawing", *p, a_q=a_nodes, phi_q=2000, t_q=1000) for p in g["theta"]]
    return g, refs


def test_restatement_matches_the_script(fixture_rows):
    """Rows of field.py itself (its own and seven seeded ones) within the bars of field_shapes; the script forms 1 + w as
    1 + (-1 + x), the restatement directly, which is why phi is compared in units of the row's largest phi."""
    g, refs = fixture_rows
    got = dict(phi_a=g["phi"], t_a=g["t"], K_a=g["K"], V_a=g["V"], phi_grid=g["phi_plot"], V_phi=g["V_of_phi"], t_grid=g["t_plot"],
               a_t=g["a_of_t"], phi_t=g["phi_of_t"], phi_today=g["scalars"][:, 0], t_today=g["scalars"][:, 1],
               hubble_time=g["scalars"][:, 2])
    thin = []
    for r in refs:
        assert r["status"] == 0
        t = dict(r)
        for k, step in (("phi_grid", 10), ("V_phi", 10), ("t_grid", 10), ("a_t", 10), ("phi_t", 10)):
            t[k] = r[k][::step]
        thin.append(t)
    assert (g["sizes"] == [2000, 1000]).all()
    worst = fs.compare(got, thin)
    print("restatement vs script, error / bar:", {k: f"{v:.1e}" for k, v in sorted(worst.items())})
    assert set(worst) >= {"phi_a", "t_a", "K_a", "V_a", "phi_grid", "V_phi", "t_grid", "a_t", "phi_t", "phi_today", "t_today", "hubble_time"}
    assert max(worst.values()) <= 1.0, worst


def test_script_loses_digits_where_the_restatement_does_not(fixture_rows):
    """The reason for the scaled bar: relative to phi itself the script's early nodes are off by far more than 1e-10."""
    g, refs = fixture_rows
    rel = max(float(np.max(np.abs(g["phi"][i][1:32] - r["phi_a"][1:32]) / r["phi_a"][1:32])) for i, r in enumerate(refs))
    assert 1e-9 < rel < 1e-4


@pytest.mark.parametrize("name", sorted(fs.MODELS))
def test_status_and_monotonicity_of_the_test_rows(pkg, name):
    """The rows of the GPU tests as the restatement sees them, and the Model of each case: its slot map must read back the
    physical rows the theta layout was made from (what ``field_shapes.effective`` assumes of the kernel's slot read-out)."""
    phys = fs.physical(name, 65, seed=11)
    m = pkg.quintessence.Model(n_a=257, **fs.MODELS[name])
    th = fs.theta_of(name, phys)
    assert m.ndim == th.shape[1] and m._desc.n_par == (4 if m.fde == "cpl" else 3)
    seen = np.zeros_like(phys)
    for s, n in enumerate(pkg._lib.FIELD_PARS[:m._desc.n_par]):
        par = m._desc.par[s]
        seen[:, s] = par.fixed if par.idx < 0 else par.scale * th[:, par.idx]
    np.testing.assert_array_equal(seen, fs.effective(name, th))
    refs = fs.reference_rows(name, fs.theta_of(name, phys), 257)
    planted = fs.planted(name, 65)
    assert sorted(planted.values()) == ([2, 2] if fs.MODELS[name]["fde"] == "thawing" else [1, 2, 2]) and fs.planted(name, 2) == {}
    for i, r in enumerate(refs):
        assert r["status"] == planted.get(i, 0), (name, i)
        if r["status"] == 1:
            assert np.isnan(r["phi_max"]) and np.isfinite(float(r["t_max"]))
        elif r["status"] == 2:
            assert np.isnan(r["t_max"])
        else:
            assert np.all(np.diff(r["phi"]) > 0) and np.all(np.diff(r["t"]) > 0), (name, i)


def test_fixture_rows_are_strictly_increasing(fixture_rows):
    for r in fixture_rows[1]:
        assert np.all(np.diff(r["phi"]) > 0) and np.all(np.diff(r["t"]) > 0)
        assert np.all(np.diff(r["phi"].astype(np.float64)) > 0) and np.all(np.diff(r["t"].astype(np.float64)) > 0)


def test_interpolation_rules_match_scipy_and_numpy():
    """A check of the yardstick alone (it needs nothing of the library): the two rules of tests/field_reference.py are scipy's
    and numpy's."""
    from scipy.interpolate import interp1d

    rng = np.random.default_rng(0)
    x = np.cumsum(rng.uniform(0.1, 1.0, 40))
    y = rng.standard_normal(40)
    xq = np.concatenate([rng.uniform(x[0] - 3, x[-1] + 3, 200), x[[0, 5, 39]]])
    want = interp1d(x, y, bounds_error=False, fill_value="extrapolate")(xq)
    assert np.allclose(fr.interp1d_extrap(xq, x.astype(fr.LD), y.astype(fr.LD)).astype(float), want, rtol=1e-13, atol=1e-13)
    assert np.allclose(fr.np_interp(xq, x.astype(fr.LD), y.astype(fr.LD)).astype(float), np.interp(xq, x, y), rtol=1e-13, atol=1e-13)
    assert fr.np_interp(x[[5]], x.astype(fr.LD), y.astype(fr.LD))[0] == y[5]


# ---- cf_field: every refusal comes before the first HIP call ----------------------------------------------------------------
def _desc(L, **over):
    d = L.cf_field_desc()
    d.struct_size, d.fde, d.n_a, d.ndim, d.n_par = C.sizeof(L.cf_field_desc), L.CF_FDE_THAWING, 64, 3, 3
    d.a_min, d.a_max, d.orh2 = 1e-8, 5.0, 4.1835e-05
    for s in range(4):
        d.par[s].idx, d.par[s].scale, d.par[s].fixed = (s if s < 3 else -1), 1.0, 0.0
    for k, v in over.items():
        if k.startswith("par"):
            s, f = int(k[3]), k[5:]
            setattr(d.par[s], f, v)
        else:
            setattr(d, k, v)
    return d


def test_field_layouts_match_c(pkg, tmp_path):
    import os
    import subprocess

    from conftest import ROOT

    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "cosmofit.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu", '
            "sizeof(cf_field_desc), sizeof(cf_field_queries), sizeof(cf_field_out), offsetof(cf_field_desc, par), "
            "offsetof(cf_field_queries, n_aq), offsetof(cf_field_out, status)); return 0;}")
    (tmp_path / "sz.c").write_text(prog)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "sz.c"), "-o", str(tmp_path / "sz")], check=True)
    vals = list(map(int, subprocess.run([str(tmp_path / "sz")], capture_output=True, text=True, check=True).stdout.split()))
    L = pkg._lib
    assert vals == [C.sizeof(L.cf_field_desc), C.sizeof(L.cf_field_queries), C.sizeof(L.cf_field_out), L.cf_field_desc.par.offset,
                    L.cf_field_queries.n_aq.offset, L.cf_field_out.status.offset]
    assert pkg.lib().cf_abi_version() == 11


def test_entry_points_validate_before_any_hip_call(pkg):
    L, lib = pkg._lib, pkg.lib()
    theta = np.array([[66.53, 0.312, -0.763]])
    buf = np.zeros(4096 + 8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    big = C.c_void_p(p(buf).value)

    def call(desc, S=1, q=None, o=None, fn="cf_field"):
        q = q if q is not None else L.cf_field_queries()
        o = o if o is not None else L.cf_field_out()
        if fn == "cf_field":
            return lib.cf_field(C.byref(desc), p(theta), S, C.byref(q), C.byref(o))
        return lib.cf_field_device(C.byref(desc), p(theta), S, C.byref(q), C.byref(o), None)

    def queries(**kw):
        q = L.cf_field_queries()
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    def outs(*names):
        o = L.cf_field_out()
        for n in names:
            setattr(o, n, big)
        return o

    cases = [
        (dict(desc=_desc(L, struct_size=8)), "struct_size"),
        (dict(desc=_desc(L, fde=L.CF_FDE_LCDM)), "LCDM has no field"),
        (dict(desc=_desc(L, fde=7)), "fde must be"),
        (dict(desc=_desc(L, n_a=15)), r"n_a must be in 16\.\.8192"),
        (dict(desc=_desc(L, n_a=8193)), r"n_a must be in 16\.\.8192"),
        (dict(desc=_desc(L, a_min=0.0)), "a_min < 1 < a_max"),
        (dict(desc=_desc(L, a_min=1.0)), "a_min < 1 < a_max"),
        (dict(desc=_desc(L, a_max=1.0)), "a_min < 1 < a_max"),
        (dict(desc=_desc(L, a_max=np.inf)), "a_min < 1 < a_max"),
        (dict(desc=_desc(L, a_min=np.nan)), "a_min < 1 < a_max"),
        (dict(desc=_desc(L, orh2=-1.0)), "orh2"),
        (dict(desc=_desc(L, ndim=0)), "ndim"),
        (dict(desc=_desc(L, ndim=65)), "ndim"),
        (dict(desc=_desc(L, par0_idx=3)), "column of H0"),
        (dict(desc=_desc(L, par2_idx=-2)), "column of w0"),
        (dict(desc=_desc(L, par1_scale=np.nan)), "scale of Om"),
        (dict(desc=_desc(L, par1_idx=-1, par1_fixed=np.inf)), "fixed value of Om"),
        (dict(desc=_desc(L, n_par=4)), "wa must be given exactly when"),
        (dict(desc=_desc(L, fde=L.CF_FDE_CPL)), "wa must be given exactly when"),
        (dict(desc=_desc(L, fde=L.CF_FDE_CPL, n_par=4, par3_idx=3)), "column of wa"),
        (dict(desc=_desc(L), S=-1), "S out of range"),
        (dict(desc=_desc(L), S=2**31), "S out of range"),
        (dict(desc=_desc(L), q=queries(a_q=big, n_aq=0)), "a_q and n_aq"),
        (dict(desc=_desc(L), q=queries(n_aq=3)), "a_q and n_aq"),
        (dict(desc=_desc(L), q=queries(a_q=big, n_aq=4097)), "at most 4096"),
        (dict(desc=_desc(L), q=queries(n_phi=4097)), "at most 4096"),
        (dict(desc=_desc(L), q=queries(n_t=-1)), "negative query count"),
        (dict(desc=_desc(L), q=queries(phi_q=big, n_phi=0)), "phi_q needs"),
        (dict(desc=_desc(L), q=queries(t_q=big, n_t=0)), "t_q needs"),
        (dict(desc=_desc(L), o=outs("w_a")), "without a_q"),
        (dict(desc=_desc(L), o=outs("V_phi")), "n_phi = 0"),
        (dict(desc=_desc(L), o=outs("a_t")), "n_t = 0"),
        (dict(desc=_desc(L), q=queries(phi_q=big, n_phi=4), o=outs("phi_grid")), "phi_grid is written only"),
        (dict(desc=_desc(L), q=queries(t_q=big, n_t=4), o=outs("t_grid")), "t_grid is written only"),
    ]
    for fn in ("cf_field", "cf_field_device"):
        for kw, msg in cases:
            with pytest.raises(pkg.CosmofitError, match=f"CF_ERR_INVALID: {fn}: .*{msg}"):
                L.check(call(fn=fn, **kw))
        assert lib.cf_field(None, p(theta), 1, None, None) == -1
        assert call(_desc(L), S=0, fn=fn) == 0  # no rows: a no-op, with or without a device
    if lib.cf_device_count() == 0:
        with pytest.raises(pkg.CosmofitError, match="CF_ERR_NO_DEVICE"):
            L.check(call(_desc(L), q=queries(n_phi=4), o=outs("a_phi")))


def test_launches_cover_the_rows_once_in_grids_the_device_takes(pkg):
    """cf_field_device runs one workgroup of 512 threads per row: 10^7 rows in one grid would be more threads than a launch may
    hold.  The cut into grids is host arithmetic of the library, checked here for every size up to the largest S accepted."""
    L, lib = pkg._lib, pkg.lib()
    cap = L.CF_FIELD_LAUNCH_ROWS
    assert cap * 512 <= 2**31 and cap == 1 << 22
    for S in (0, 1, 65, cap - 1, cap, cap + 1, 8388608, 8388609, 10**7, 3 * cap, 2**31 - 1):
        n = lib.cf_field_launch_count(S)
        assert n == -(-S // cap)
        at = 0
        for k in range(n):
            b, e = C.c_int64(), C.c_int64()
            lib.cf_field_launch_range(S, k, C.byref(b), C.byref(e))
            assert b.value == at and 1 <= e.value - b.value <= cap
            at = e.value
        assert at == S
        for k in (-1, n, n + 5):
            b, e = C.c_int64(-7), C.c_int64(-7)
            lib.cf_field_launch_range(S, k, C.byref(b), C.byref(e))
            assert (b.value, e.value) == (S, S)
    assert lib.cf_field_launch_count(-3) == 0
    assert lib.cf_field_launch_count(10**7) == 3  # a chain of the size the feature is for


# ---- the Python layer ---------------------------------------------------------------------------------------------------------
def test_model_from_recipe(pkg):
    Q = pkg.quintessence
    m = Q.Model.from_recipe("bao/desi_des5y_H0trgb.py")  # (offset, H0, rd, Om, w0)
    assert (m.fde, m.columns, m.scale, m.fixed, m.ndim) == ("thawing", {"H0": 1, "Om": 3, "w0": 4}, {}, {}, 5)
    m = Q.Model.from_recipe("bao/desi_fs_lya.py", n_a=257)  # (h, Om, w0)
    assert (m.columns, m.scale, m.ndim, m.n_a) == ({"H0": 0, "Om": 1, "w0": 2}, {"H0": 100.0}, 3, 257)
    assert m._desc.par[0].scale == 100.0 and m._desc.par[3].idx == -1 and m._desc.n_par == 3
    m = Q.Model.from_recipe(pkg.scripts.RECIPES["bao/desi_pantheon_rd.py"])  # (offset, H0, Om, rd, w0)
    assert (m.columns, m.ndim) == ({"H0": 1, "Om": 2, "w0": 4}, 5)
    for name, msg in (("bao/desi_cmb_union3.py", "physical densities"), ("bao/desi_des5y_omh2.py", "Omega_m h"),
                      ("bao/desi_des5y_cc.py", "no scalar field")):
        with pytest.raises(ValueError, match=msg):
            Q.Model.from_recipe(name)
    with pytest.raises(KeyError):
        Q.Model.from_recipe("bao/nothing.py")


def test_model_argument_checks(pkg):
    Q = pkg.quintessence
    cols = {"H0": 0, "Om": 1, "w0": 2}
    for kw, msg in ((dict(fde="lcdm", columns=cols), "no scalar field"), (dict(fde="cubic", columns=cols), "unknown fde"),
                    (dict(columns={"H0": 0, "Om": 1}), "w0 must be given once"), (dict(columns=dict(cols, wa=3)), "cpl"),
                    (dict(fde="cpl", columns=cols), "wa must be given once"), (dict(columns=cols, fixed={"Om": 0.3}), "Om must be given once"),
                    (dict(columns=cols, scale={"wa": 2.0}), "no column"), (dict(columns=dict(cols, s8=3)), "unknown parameter"),
                    (dict(columns=cols, n_a=15), "n_a"), (dict(columns=cols, n_a=8193), "n_a"), (dict(columns=cols, a_min=2.0), "a_min"),
                    (dict(columns=cols, a_max=0.5), "a_min"), (dict(columns=cols, orh2=-1.0), "orh2"), (dict(columns=cols, ndim=2), "ndim"),
                    (dict(columns={"H0": 0, "Om": 1, "w0": -1}), "index"), (dict(columns={"H0": 0, "Om": 1}, fixed={"w0": np.nan}), "finite")):
        with pytest.raises(ValueError, match=msg):
            Q.Model(**kw)
    m = Q.Model(fde="cpl", columns={"H0": 0, "Om": 1, "w0": 2}, fixed={"wa": -0.2})
    assert m._desc.n_par == 4 and m._desc.par[3].idx == -1 and m._desc.par[3].fixed == -0.2 and m.ndim == 3


def test_bands_argument_checks_and_chunks(pkg):
    import torch

    Q, D = pkg.quintessence, pkg.derived
    m = Q.Model(columns={"H0": 0, "Om": 1, "w0": 2})
    x = torch.zeros((10, 3), dtype=torch.float64)
    for args, kw, msg in (((m, x, "V_x", [1.0]), {}, "unknown quantity"), ((m, x, "V_phi"), {}, "needs the points"),
                          ((m, x, "t_today", [1.0]), {}, "takes no x"), ((m, x, "V_a", [np.nan]), {}, "finite"),
                          ((m, x, "V_a", []), {}, "non-empty"), ((m, x, "V_a", [1.0]), dict(q=[1.5]), "quantile levels"),
                          ((m, x[0], "V_a", [1.0]), {}, "samples"), ((m, x, "V_a", [1.0]), dict(max_bytes=0), "max_bytes"),
                          ((m, x.float(), "V_a", [1.0]), {}, "float64"), ((m, x[:, :2], "V_a", [1.0]), {}, r"\[n, 3\]"),
                          ((object(), x, "V_a", [1.0]), {}, "Model"), ((m, x, "V_a", [1.0]), {}, "MI355X"),
                          ((m, x, "V_a", [1.0]), dict(weights=torch.ones(9, dtype=torch.float64)), "weights")):
        with pytest.raises(ValueError, match=msg):
            Q.bands(*args, **kw)
    for fn in (Q.reconstruct,):
        with pytest.raises(ValueError, match="MI355X"):
            fn(m, x)
        with pytest.raises(ValueError, match="own grid"):
            fn(m, x, phi=4097)
        with pytest.raises(ValueError, match="non-empty"):
            fn(m, x, a=[])
    assert Q.pieces(1) == [(0, 1)] and Q.pieces(4096) == [(0, 4096)] and Q.pieces(4097) == [(0, 4096), (4096, 4097)]
    assert Q.pieces(3 * 4096) == [(0, 4096), (4096, 8192), (8192, 12288)] and Q.pieces(0) == [(0, 0)]
    assert Q.MAX_NQ == pkg._lib.CF_CURVE_MAX_NZ == 4096  # bands shares derived.band_chunk, whose cap is the curves' launch
    assert D.band_chunk(3000, 2000, 2**31) == 2000 and D.band_chunk(10**6, 2000, 2**31) == 67 and D.band_chunk(10**7, 9, 1) == 1
