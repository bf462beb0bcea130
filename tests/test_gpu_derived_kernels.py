"""GPU (-m gpu): cf_derived_device / cf_curves_device (csrc/cosmofit_derived.hip) called directly on torch buffers, as
derived.py calls them.  The judges are the fixture the reference computed (tests/golden/derived.npz), the long-double
restatement (tests/derived_reference.py, bar 1e-10; q0, j0 and wa cross zero: absolute 1e-12) and the engine's own one-theta
accessors (``parts``, ``H_z``, ``DM_z``, ``bao_theory_at``: bar 1e-12).

What fixed-order sums promise is asserted exactly: a row has the same bits at every S, at every position, alone or beside
every other quantity; a NaN row leaves its neighbours' bits alone; every output buffer is followed by a sentinel that must
survive.  Every test prints the largest error it saw per quantity (``-s`` shows them; profiles/NOTES_derived.md quotes them)."""
import ctypes as C

import numpy as np
import pytest
import torch

import derived_reference as R
import derived_shapes as DS
from conftest import golden

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LD = np.longdouble
SENTINEL = -7.25e300
PAD = 64
S_SET = (1, 63, 64, 65, 257, 4097)
REL_REF, ABS0, REL_ENGINE = 1e-10, 1e-12, 1e-12
ZERO_CROSSING = ("q0", "j0", "wa")


@pytest.fixture(scope="module")
def lib(pkg):
    if pkg.lib().cf_device_count() < 1:
        pytest.fail("GPU tests need an MI355X; no HIP device visible (there is no fallback path)")
    return pkg._lib, pkg.lib()


@pytest.fixture(scope="module")
def engines(pkg, lib):
    cache = {}

    def get(case, n_grid=4000):
        if (case, n_grid) not in cache:
            cache[case, n_grid] = pkg.LikelihoodEngine(**DS.engine_kwargs(pkg, case, n_grid))
        return cache[case, n_grid]

    yield get
    for e in cache.values():
        e.close()


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _consts(pkg, case):
    L = pkg._lib
    c = L.cf_derived_consts()
    c.struct_size = C.sizeof(L.cf_derived_consts)
    comp = DS.comp_of(pkg, case)
    if comp is not None:
        c.zdrag_fit[:] = list(comp["zdrag_fit"])
        c.rdrag_fit[:] = list(comp["rd_fit"])
        c.has_rdrag_fit = 1
        c.zeq_or_h2 = comp["zeq_or_h2"]
    return c


def _codes(pkg, names):
    L = pkg._lib
    codes = np.array([L.DERIVED_CODES["H@"] if n.startswith("H@") else L.DERIVED_CODES[n] for n in names], dtype=np.int32)
    args = np.array([float(n[2:]) if n.startswith("H@") else 0.0 for n in names], dtype=np.float64)
    return codes, args


def _derived(pkg, lib, eng, case, theta, names):
    """cf_derived_device into a buffer PAD longer than [S, n_q]: numpy [S, n_q]; the tail must keep its sentinel."""
    L, so = lib
    dth = torch.from_numpy(np.ascontiguousarray(theta)).to(DEV)
    S, nq = theta.shape[0], len(names)
    codes, args = _codes(pkg, names)
    c = _consts(pkg, case)
    buf = torch.full((S * nq + PAD,), SENTINEL, dtype=torch.float64, device=DEV)
    L.check(so.cf_derived_device(eng._h, dth.data_ptr(), S, codes.ctypes.data_as(C.c_void_p), args.ctypes.data_as(C.c_void_p), nq,
                                 C.cast(C.pointer(c), C.c_void_p), buf.data_ptr(), _stream()))
    out = buf.cpu().numpy()
    assert (out[S * nq:] == SENTINEL).all(), "cf_derived_device wrote outside its [S, n_q] block"
    return out[: S * nq].reshape(S, nq)


def _curves(pkg, lib, eng, theta, z, quantity):
    L, so = lib
    dth = torch.from_numpy(np.ascontiguousarray(theta)).to(DEV)
    dz = torch.from_numpy(np.ascontiguousarray(z, dtype=np.float64)).to(DEV)
    S, nz = theta.shape[0], len(z)
    buf = torch.full((S * nz + PAD,), SENTINEL, dtype=torch.float64, device=DEV)
    L.check(so.cf_curves_device(eng._h, dth.data_ptr(), S, L.CURVE_CODES[quantity], dz.data_ptr(), nz, buf.data_ptr(), _stream()))
    out = buf.cpu().numpy()
    assert (out[S * nz:] == SENTINEL).all(), "cf_curves_device wrote outside its [S, nz] block"
    return out[: S * nz].reshape(S, nz)


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def _judge(name, got, want, rel_bar, tag):
    """got float64, want long double: relative bar, or the absolute one for the quantities that cross zero."""
    err = np.abs(got.astype(LD) - want)
    if name in ZERO_CROSSING:
        worst = float(err.max())
        print(f"{tag} {name}: max abs err {worst:.2e}")
        assert worst <= ABS0, (tag, name, worst)
    else:
        worst = float((err / np.abs(want)).max())
        print(f"{tag} {name}: max rel err {worst:.2e}")
        assert worst <= rel_bar, (tag, name, worst)


# ---- scalar quantities -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", DS.CASES)
def test_every_code_against_fixture_and_restatement_at_every_S(pkg, lib, engines, case):
    eng, base = engines(case), DS.thetas(case)
    names = DS.applicable_scalars(pkg, case)
    assert set(DS.COLUMNS[case]) <= set(names)
    ref = _derived(pkg, lib, eng, case, base, names)  # the canonical values: the fixture's 300 rows, every code at once
    want = R.scalars(DS.model(pkg, case), base, names)
    for j, name in enumerate(names):
        _judge(name, ref[:, j], want[:, j], REL_REF, f"{case} vs restatement")
    fixture = DS.expected(case)
    for j, name in enumerate(DS.COLUMNS[case]):
        _judge(name, ref[:, names.index(name)], fixture[:, j].astype(LD), REL_REF, f"{case} vs fixture")
    n = base.shape[0]
    for S in S_SET:  # a row keeps its bits at every S and at every position (row i of the batch is fixture row (7 i + 3) mod n)
        pick = (7 * np.arange(S) + 3) % n
        got = _derived(pkg, lib, eng, case, base[pick], names)
        assert _same_bits(got, ref[pick]), (case, S)
    for j, name in enumerate(names):  # ... and alone (n_q = 1)
        one = _derived(pkg, lib, eng, case, base[:65], [name])
        assert _same_bits(one[:, 0], ref[:65, j]), (case, name)
    rev = _derived(pkg, lib, eng, case, base[:65], names[::-1])
    assert _same_bits(rev[:, ::-1], ref[:65])


@pytest.mark.parametrize("case", ["desi_cmb_thawing", "desi_cmb_union3_fs8", "desi_des5y_obh2_theta_star", "cmb_cmb"])
def test_fits_and_cmb_distances_against_engine_parts(pkg, lib, engines, case):
    """z_star, r_drag and the compressed-CMB vector as the likelihood's own kernel evaluates them (cf_eval_parts)."""
    eng, th = engines(case), DS.thetas(case)[:64]
    parts = eng.parts(th)
    mode = DS.comp_of(pkg, case)["cmb_mode"]
    names = ["z_star"] + (["r_drag"] if case != "cmb_cmb" else []) + (["R", "lA"] if mode == 1 else ["theta_star100"])
    got = _derived(pkg, lib, eng, case, th, names)
    want = {"z_star": parts["z_star"], "r_drag": parts["r_drag"], "R": parts["cmb_vector"][:, 0], "lA": parts["cmb_vector"][:, 1],
            "theta_star100": 100 * parts["cmb_vector"][:, 0]}
    for j, name in enumerate(names):
        _judge(name, got[:, j], want[name].astype(LD), REL_ENGINE, f"{case} vs engine.parts")


def test_cmb_quantities_against_the_mirror_blobs(pkg, lib, engines):
    """cmb/cmb.py's blobs (100 theta*, r*, D_M* / Gpc, z*) as likelihoods.CmbOnly.blobs derives them from cf_eval_parts, and R."""
    th = DS.thetas("cmb_cmb")[:64]
    lk = pkg.likelihoods.CmbOnly()
    try:
        blobs, vec = lk.blobs(th), lk.engine.parts(th)["cmb_vector"]
    finally:
        lk.engine.close()
    got = _derived(pkg, lib, engines("cmb_cmb"), "cmb_cmb", th, ["theta_star100", "rs_star", "DM_star", "z_star", "R"])
    got[:, 2] /= 1000
    for j, name in enumerate(["theta_star100", "rs_star", "DM_star/Gpc", "z_star"]):
        _judge(name, got[:, j], blobs[:, j].astype(LD), REL_ENGINE, "cmb_cmb vs CmbOnly.blobs")
    _judge("R", got[:, 4], vec[:, 0].astype(LD), REL_ENGINE, "cmb_cmb vs CmbOnly.blobs")


@pytest.mark.parametrize("case", ["desi_cmb_union3_fs8", "desi_union3_bbn_thaw", "cmb_cmb"])
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_non_finite_entry_stays_in_its_row_and_its_columns(pkg, lib, engines, case, bad):
    eng, base = engines(case), DS.thetas(case)[:130].copy()
    names = DS.applicable_scalars(pkg, case)
    clean = _derived(pkg, lib, eng, case, base, names)
    kw = DS.engine_kwargs(pkg, case)
    reads = {"H0": ["H0", "h"], "obh2": ["obh2"], "och2": ["och2"], "Om": ["Om"], "s8": ["S8"], "w0": ["w0"]}
    for slot, p in kw["params"].items():
        th = base.copy()
        th[64, p.idx] = bad
        got = _derived(pkg, lib, eng, case, th, names)
        rows = np.arange(130) != 64
        assert _same_bits(got[rows], clean[rows]), (case, slot)
        for name in reads[slot]:
            if name in names:
                assert np.isnan(got[64, names.index(name)]), (case, slot, name)
        # a column that does not read the slot keeps its bits: w0 never depends on H0, H0 never on anything else
        for name, others in (("w0", ("H0", "obh2", "och2", "Om", "s8")), ("H0", ("obh2", "och2", "Om", "s8", "w0"))):
            if slot in others and name in names:
                assert _same_bits(got[64, names.index(name)], clean[64, names.index(name)]), (case, slot, name)
    unused = [k for k in range(base.shape[1]) if k not in {p.idx for p in kw["params"].values()}]
    for k in unused:  # a theta column no slot reads (dM, v) changes nothing
        th = base.copy()
        th[64, k] = bad
        assert _same_bits(_derived(pkg, lib, eng, case, th, names), clean), (case, k)


def test_errors_name_the_quantity(pkg, lib, engines):
    L, so = lib
    th = torch.zeros((4, 6), dtype=torch.float64, device=DEV)
    out = torch.zeros((4 * 40,), dtype=torch.float64, device=DEV)

    def call(case, names, n_q=None, consts=True):
        codes, args = _codes(pkg, names)
        c = _consts(pkg, case)
        return so.cf_derived_device(engines(case)._h, th.data_ptr(), 4, codes.ctypes.data_as(C.c_void_p), args.ctypes.data_as(C.c_void_p),
                                    len(names) if n_q is None else n_q, C.cast(C.pointer(c), C.c_void_p) if consts else None,
                                    out.data_ptr(), _stream())

    for case, name, what in (("desi_cmb_thawing", "S8", "sigma8"), ("desi_union3_bbn", "rs_star", "Gauss-Legendre"),
                             ("desi_union3_bbn", "och2", "och2 slot"), ("desi_union3_bbn", "z_star", "compressed-CMB"),
                             ("cmb_cmb", "rd", "r_d slot")):
        with pytest.raises(pkg.CosmofitError, match=f"CF_ERR_INVALID.*: {name} needs .*{what}"):
            L.check(call(case, ["H0", name]))
    with pytest.raises(pkg.CosmofitError, match="CF_ERR_INVALID.*z_drag needs cf_derived_consts"):
        L.check(call("cmb_cmb", ["z_drag"], consts=False))
    with pytest.raises(pkg.CosmofitError, match="CF_ERR_INVALID.*r_drag needs r_drag coefficients"):
        L.check(call("cmb_cmb", ["r_drag"], consts=False))
    for n_q in (0, 33):
        with pytest.raises(pkg.CosmofitError, match="CF_ERR_INVALID.*n_q"):
            L.check(call("cmb_cmb", ["H0"] * 33, n_q=n_q))
    assert (out == 0).all()
    codes = np.array([17], dtype=np.int32)
    with pytest.raises(pkg.CosmofitError, match="unknown quantity code 17"):
        L.check(so.cf_derived_device(engines("cmb_cmb")._h, th.data_ptr(), 4, codes.ctypes.data_as(C.c_void_p), None, 1, None,
                                     out.data_ptr(), _stream()))
    z = torch.zeros((8,), dtype=torch.float64, device=DEV)
    for nz in (0, 4097):
        with pytest.raises(pkg.CosmofitError, match="CF_ERR_INVALID.*nz"):
            L.check(so.cf_curves_device(engines("cmb_cmb")._h, th.data_ptr(), 4, 0, z.data_ptr(), nz, out.data_ptr(), _stream()))
    with pytest.raises(pkg.CosmofitError, match="CF_ERR_INVALID.*DV_rd needs .*r_d slot"):
        L.check(so.cf_curves_device(engines("cmb_cmb")._h, th.data_ptr(), 4, 2, z.data_ptr(), 8, out.data_ptr(), _stream()))
    with pytest.raises(pkg.CosmofitError, match="unknown curve code 7"):
        L.check(so.cf_curves_device(engines("cmb_cmb")._h, th.data_ptr(), 4, 7, z.data_ptr(), 8, out.data_ptr(), _stream()))
    # S = 0 is a no-op, also with null buffers
    codes, args = _codes(pkg, ["H0"])
    L.check(so.cf_derived_device(engines("cmb_cmb")._h, None, 0, codes.ctypes.data_as(C.c_void_p), args.ctypes.data_as(C.c_void_p), 1, None,
                                 None, _stream()))
    L.check(so.cf_curves_device(engines("cmb_cmb")._h, None, 0, 0, None, 8, None, _stream()))
    torch.cuda.synchronize()
    assert (out == 0).all()


def test_host_twins_have_the_device_bits(pkg, lib, engines):
    case = "desi_cmb_thawing"
    eng, th = engines(case), DS.thetas(case)[:70]
    names = DS.applicable_scalars(pkg, case)
    spec = pkg.derived.Spec(eng, names + ["DM@0.51", "DV_rd@1.3"], **DS.consts(pkg, case))
    host = spec.host_columns(th)
    assert _same_bits(host[:, : len(names)], _derived(pkg, lib, eng, case, th, names))
    assert _same_bits(host[:, len(names)], _curves(pkg, lib, eng, th, [0.51], "DM")[:, 0])
    assert _same_bits(host[:, len(names) + 1], _curves(pkg, lib, eng, th, [1.3], "DV_rd")[:, 0])
    assert _same_bits(eng.derived(th[3], ["Om", "rd"]), host[3, [names.index("Om"), names.index("rd")]])


def test_cf_derived_beyond_one_piece_has_the_device_bits(pkg, lib, engines):
    """cf_derived stages its rows through the device in pieces of 65536: 65537 rows cross one boundary, so the second piece's
    row is read from behind the first's and its two columns land behind them."""
    L, so = lib
    case, S = "desi_cmb_thawing", 65537
    eng, base = engines(case), DS.thetas(case)[:40]
    th = np.ascontiguousarray(base[(7 * np.arange(S) + 3) % 40])
    names = DS.applicable_scalars(pkg, case)[:2]
    codes, args = _codes(pkg, names)
    c = _consts(pkg, case)
    out = np.full((S, 2), SENTINEL)
    L.check(so.cf_derived(eng._h, th.ctypes.data, S, codes.ctypes.data_as(C.c_void_p), args.ctypes.data_as(C.c_void_p), 2,
                          C.cast(C.pointer(c), C.c_void_p), out.ctypes.data))
    assert np.isfinite(out).all() and (out != SENTINEL).all()
    assert _same_bits(out, _derived(pkg, lib, eng, case, th, names))


# ---- curves ------------------------------------------------------------------------------------------------------------------
def _late_pchip_kwargs(pkg, n_grid):
    """likelihoods.DesiBao: late-time flat, thawing, h as the parameter, fixed r_d, D_H by PCHIP of the grid."""
    g = golden("bao_desi_cmb")
    P = pkg.Param
    return dict(ndim=3, z_max=float(np.max(g["bao_z"]) + 0.1), n_grid=n_grid, fde=pkg.CF_FDE_THAWING,
                params=dict(H0=P(0, scale=100.0), Om=P(1), w0=P(2), rd=P(fixed=147.09)),
                bao=dict(z=g["bao_z"], val=g["bao_val"], qty=g["bao_qty"], inv_cov=g["bao_inv_cov"]))


CURVE_ENGINES = ("desi_cmb_thawing", "desi_union3_bbn", "late_pchip")


@pytest.fixture(scope="module")
def curve_setup(pkg, engines):
    cache = {}

    def get(name, n_grid):
        if (name, n_grid) not in cache:
            if name == "late_pchip":
                kw = _late_pchip_kwargs(pkg, n_grid)
                th = np.array([[0.68, 0.31, -0.85], [0.72, 0.26, -0.6], [0.61, 0.42, -0.999]])
                cache[name, n_grid] = (pkg.LikelihoodEngine(**kw), R.model_of(kw), th, True)
            else:
                cache[name, n_grid] = (engines(name, n_grid), DS.model(pkg, name, n_grid), DS.thetas(name)[:3], False)
        return cache[name, n_grid][:3]

    yield get
    for eng, _, _, own in cache.values():
        if own:
            eng.close()


def _z_set(nz, z_max):
    """z = 0, the grid's end, beyond it, unsorted: what a caller may pass."""
    if nz == 1:
        return np.array([z_max + 0.37])
    if nz == 2:
        return np.array([z_max, 0.0])
    rng = np.random.default_rng(nz)
    return np.concatenate([rng.uniform(0.0, z_max, nz - 5), [z_max + 0.5, 0.0, z_max, 1e-9, np.nextafter(z_max, 0)]])


@pytest.mark.parametrize("n_grid", [16, 4000])
@pytest.mark.parametrize("nz", [1, 2, 200])
@pytest.mark.parametrize("name", CURVE_ENGINES)
def test_curves_against_the_one_theta_accessors_and_the_restatement(pkg, lib, curve_setup, name, nz, n_grid):
    eng, model, th = curve_setup(name, n_grid)
    z = _z_set(nz, model.z_max)
    got = {q: _curves(pkg, lib, eng, th, z, q) for q in R.CURVES}
    qty = {"DV_rd": 0, "DM_rd": 1, "DH_rd": 2, "F_AP": 3}
    with np.errstate(all="ignore"):
        for r in range(th.shape[0]):
            dm = eng.DM_z(th[r], z)
            want = {"H": eng.H_z(th[r], z), "DM": dm, "mu": 25 + 5 * np.log10((1 + z) * dm)}
            want.update({q: eng.bao_theory_at(th[r], z, code) for q, code in qty.items()})
            for q in R.CURVES:  # 0 at z = 0 and -inf for mu there are equal on both sides; F_AP = 0 / D_H likewise
                ok = np.isclose(got[q][r], want[q], rtol=REL_ENGINE, atol=0.0, equal_nan=True)
                assert ok.all(), (name, q, r, float(np.nanmax(np.abs(got[q][r] / want[q] - 1)[~ok])))
        worst = {}
        for q in R.CURVES:
            ref = R.curves(model, th, z, q)
            ok = np.isclose(got[q].astype(LD), ref, rtol=REL_REF, atol=0.0, equal_nan=True)
            fin = np.isfinite(ref) & (ref != 0)
            worst[q] = float(np.max(np.abs(got[q].astype(LD)[fin] / ref[fin] - 1))) if fin.any() else 0.0
            assert ok.all(), (name, q, worst[q])
    print(f"{name} G={n_grid} nz={nz} vs restatement: " + ", ".join(f"{q} {v:.1e}" for q, v in worst.items()))


@pytest.mark.parametrize("name", CURVE_ENGINES)
def test_a_curve_row_keeps_its_bits_at_every_S_and_position(pkg, lib, curve_setup, engines, name):
    eng, model, _ = curve_setup(name, 4000)
    base = DS.thetas(name)[:40] if name != "late_pchip" else np.random.default_rng(5).uniform([0.55, 0.15, -1.0], [0.8, 0.45, -0.4], (40, 3))
    z = _z_set(2, model.z_max)
    for q in ("DM", "DV_rd"):
        ref = _curves(pkg, lib, eng, base, z, q)
        for S in S_SET:
            pick = (7 * np.arange(S) + 3) % 40
            assert _same_bits(_curves(pkg, lib, eng, base[pick], z, q), ref[pick]), (name, q, S)
        wide = _curves(pkg, lib, eng, base[:5], np.concatenate([[0.7, 1.9], z, [0.2]]), q)  # ... and beside other redshifts
        assert _same_bits(wide[:, 2:4], ref[:5]), (name, q)


def test_cf_curves_beyond_one_piece_has_the_device_bits(pkg, lib, curve_setup):
    """cf_curves stages 65536 * 16 / nz rows per piece: at nz = 4096 that is 256, so 257 rows cross one boundary and the second
    piece's curve lands behind the first 256."""
    L, so = lib
    eng, model, _ = curve_setup("late_pchip", 16)
    S, nz = 257, 4096
    th = np.ascontiguousarray(np.random.default_rng(6).uniform([0.55, 0.15, -1.0], [0.8, 0.45, -0.4], (S, 3)))
    z = np.linspace(0.0, model.z_max, nz)
    out = np.full((S, nz), SENTINEL)
    L.check(so.cf_curves(eng._h, th.ctypes.data, S, L.CURVE_CODES["DM"], z.ctypes.data, nz, out.ctypes.data))
    assert np.isfinite(out).all() and (out != SENTINEL).all()
    assert _same_bits(out, _curves(pkg, lib, eng, th, z, "DM"))


@pytest.mark.parametrize("n_grid", [16, 4000])
def test_a_non_finite_row_or_redshift_gives_nan_and_nothing_else(pkg, lib, curve_setup, n_grid):
    eng, model, _ = curve_setup("desi_cmb_thawing", n_grid)
    base = DS.thetas("desi_cmb_thawing")[:9].copy()
    z = _z_set(200, model.z_max)
    for q in ("DM", "DV_rd", "H"):
        clean = _curves(pkg, lib, eng, base, z, q)
        th = base.copy()
        th[4, 0] = np.nan
        got = _curves(pkg, lib, eng, th, z, q)
        rows = np.arange(9) != 4
        assert _same_bits(got[rows], clean[rows]) and np.isnan(got[4]).all(), q
        zb = z.copy()
        zb[[3, 77]] = [np.nan, np.inf]
        got = _curves(pkg, lib, eng, base, zb, q)
        cols = np.ones(200, dtype=bool)
        cols[[3, 77]] = False
        assert _same_bits(got[:, cols], clean[:, cols]) and np.isnan(got[:, ~cols]).all(), q
