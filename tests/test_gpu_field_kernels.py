"""GPU (-m gpu): field_kernel (csrc/cosmofit_field.hip) through cf_field_device / cf_field, at the smallest shapes that can break
the node loop, the cumulative sums with their carries, and the searches (tests/field_shapes.py), against the extended-precision
restatement of field.py (tests/field_reference.py) and against the fixture the script itself produced (tests/golden/field.npz).

The bars are those of field_shapes.compare (1e-10, scaled as each quantity is); the status vector must equal the restatement's;
only the planted rows are left out of the comparison of values, and their neighbours must match.  What a fixed summation order
promises is asserted exactly: the same bits alone and at any position of a larger call, from an own grid and from that grid
given back, from device and from host pointers.  Every test prints its largest error over bar per quantity (``-s``;
profiles/NOTES_field.md quotes them)."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import field_reference as fr
import field_shapes as fs
from conftest import golden

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENTINEL = -7.25e300


@pytest.fixture(scope="module")
def Q(pkg):
    if pkg.lib().cf_device_count() < 1:
        pytest.fail("GPU tests need an MI355X; no HIP device visible (there is no fallback path)")
    return pkg.quintessence


def _model(Q, name, n_a, **kw):
    return Q.Model(n_a=n_a, **fs.MODELS[name], **kw)


def _np(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


def _report(label, worst):
    print(f"{label}: error / bar " + ", ".join(f"{k} {v:.1e}" for k, v in sorted(worst.items())))
    assert worst and max(worst.values()) <= 1.0, (label, worst)


def _given_queries(name, theta, n_a, counts, seed):
    """a_q, phi_q, t_q for a batch: the ranges come from row 0's restatement ([0, 1.2 phi_max], [-1 Gyr, 1.2 t_max])."""
    r0 = fs.reference_rows(name, theta[:1], n_a)[0]
    a_q = fs.a_queries(counts[0], n_a, 1e-8, 5.0, seed)
    phi_q = fs.x_queries(counts[1], 0.0, 1.2 * float(r0["phi_max"]), seed + 1, negative=-0.01 * float(r0["phi_max"]))
    t_q = fs.x_queries(counts[2], -1.0, 1.2 * float(r0["t_max"]), seed + 2, negative=-0.5)
    return a_q, phi_q, t_q


def _check(Q, name, n_a, S, counts, seed, own=False):
    theta = fs.theta_of(name, fs.physical(name, S, seed))
    m = _model(Q, name, n_a)
    if own:
        a_q, phi_q, t_q = fs.a_queries(counts[0], n_a, 1e-8, 5.0, seed), counts[1], counts[2]
    else:
        a_q, phi_q, t_q = _given_queries(name, theta, n_a, counts, seed)
    got = _np(Q.reconstruct(m, torch.from_numpy(theta).to(DEV), a=a_q, phi=phi_q, t=t_q))
    refs = fs.reference_rows(name, theta, n_a, a_q=a_q, phi_q=phi_q, t_q=t_q)
    assert got["status"].dtype == np.int32 and got["status"].tolist() == [r["status"] for r in refs]
    planted = fs.planted(name, S)
    assert got["status"].tolist() == [planted.get(i, 0) for i in range(S)]
    # phi_q < 0 is interp1d's extrapolation along the nearly vertical first segment: meaningless in the script too, not compared
    skip = None if own else {k: np.nan_to_num(phi_q, nan=0.0) < 0 for k in ("a_phi", "V_phi")}
    worst = fs.compare(got, refs, skip_rows=set(planted), skip_points=skip)
    for i in planted:  # what a planted row still delivers, and what it must not
        st = got["status"][i]
        assert np.isnan(got["phi_a"][i]).all() and np.isnan(got["a_phi"][i]).all() and np.isnan(got["phi_t"][i]).all()
        assert np.isnan(got["phi_today"][i]) and np.isnan(got["phi_max"][i])
        if st == 1:
            assert np.isfinite(got["t_today"][i]) and np.isfinite(got["t_max"][i])
            worst_t = fs.compare({k: got[k][i:i + 1] for k in ("t_a", "a_t", "t_today", "t_max", "hubble_time", "w_a", "K_a", "V_a")}, [refs[i]])
            assert max(worst_t.values()) <= 1.0, worst_t
        else:
            assert all(np.isnan(got[k][i]).all() for k in ("t_a", "w_a", "K_a", "V_a", "a_t", "t_today", "t_max", "hubble_time"))
    return worst


CASES = [(name, n_a, fs.S_SIZES[i % 3], tuple(fs.N_Q[(i + j) % 4] for j in range(3)))
         for i, (name, n_a) in enumerate(itertools.product(sorted(fs.MODELS), fs.N_A))]


@pytest.mark.parametrize("name,n_a,S,counts", CASES, ids=[f"{c[0]}-na{c[1]}-S{c[2]}-q{'x'.join(map(str, c[3]))}" for c in CASES])
def test_given_queries_against_the_restatement(Q, name, n_a, S, counts):
    _report(f"{name} n_a={n_a} S={S} nq={counts}", _check(Q, name, n_a, S, counts, seed=1000 + n_a))


@pytest.mark.parametrize("name", sorted(fs.MODELS))
@pytest.mark.parametrize("n_a", [16, 65, 5000, 8192])
def test_own_grids_against_the_restatement(Q, name, n_a):
    counts = {16: (2, 1, 2), 65: (65, 257, 65), 5000: (257, 65, 257), 8192: (1, 2, 1)}[n_a]
    _report(f"own grids {name} n_a={n_a} nq={counts}", _check(Q, name, n_a, 65, counts, seed=2000 + n_a, own=True))


def test_every_row_count_with_every_query_count(Q):
    worst = {}
    for S, nq in itertools.product(fs.S_SIZES, fs.N_Q):
        for k, v in _check(Q, "thawing", 65, S, (nq, nq, nq), seed=S * 1000 + nq).items():
            worst[k] = max(worst.get(k, 0.0), v)
    _report("thawing n_a=65, S x nq", worst)


def test_more_points_than_one_launch_takes(Q):
    theta = fs.theta_of("thawing", fs.physical("thawing", 2, 5))
    m = _model(Q, "thawing", 64)
    a_q = np.exp(np.random.default_rng(3).uniform(np.log(1e-8), np.log(5.0), 4097))
    x = torch.from_numpy(theta).to(DEV)
    got = _np(Q.reconstruct(m, x, a=a_q, phi=7, t=a_q[:4097] * 2.0))
    assert got["phi_a"].shape == (2, 4097) and got["a_t"].shape == (2, 4097) and got["a_phi"].shape == (2, 7)
    _report("4097 points in pieces", fs.compare(got, fs.reference_rows("thawing", theta, 64, a_q=a_q, phi_q=7, t_q=a_q * 2.0)))
    tail = _np(Q.reconstruct(m, x, a=a_q[4096:], t=a_q[4096:] * 2.0))
    assert _bits(got["V_a"][:, 4096:], tail["V_a"]) and _bits(got["phi_a"][:, 4096:], tail["phi_a"]) and _bits(got["a_t"][:, 4096:], tail["a_t"])


@pytest.mark.parametrize("name,n_a", [("thawing", 5000), ("thawing_h", 257), ("cpl", 65), ("wcdm", 8192)])
def test_a_row_has_the_same_bits_alone_and_at_any_position(Q, name, n_a):
    rows = fs.theta_of(name, fs.physical(name, 3, 77))
    batch = fs.theta_of(name, fs.physical(name, 130, 78))
    pos = (0, 64, 129)
    for p, r in zip(pos, rows):
        batch[p] = r
    batch[1, 0] = np.nan  # a bad row beside row 0
    m = _model(Q, name, n_a)
    a_q, phi_q, t_q = _given_queries(name, rows, n_a, (65, 65, 65), 9)
    for kw in (dict(a=a_q, phi=phi_q, t=t_q), dict(a=a_q, phi=33, t=17)):
        big = _np(Q.reconstruct(m, torch.from_numpy(batch).to(DEV), **kw))
        assert big["status"][1] == 2 and (big["status"][list(pos)] == 0).all()
        for p, r in zip(pos, rows):
            alone = _np(Q.reconstruct(m, torch.from_numpy(r[None]).to(DEV), **kw))
            for k, v in alone.items():
                if v.ndim >= 1 and v.shape[0] == 1 and big[k].shape[0] == 130:
                    assert _bits(v[0], big[k][p]), (k, p)


@pytest.mark.parametrize("name,n_a", [("thawing", 5000), ("cpl", 63)])
def test_own_grids_given_back_give_the_same_bits(Q, name, n_a):
    rows = fs.theta_of(name, fs.physical(name, 2, 31))
    m = _model(Q, name, n_a)
    for r in rows:
        x = torch.from_numpy(r[None]).to(DEV)
        own = _np(Q.reconstruct(m, x, phi=65, t=257))
        back = _np(Q.reconstruct(m, x, phi=own["phi_grid"][0], t=own["t_grid"][0]))
        for k in ("a_phi", "V_phi", "a_t", "phi_t"):
            assert _bits(own[k], back[k]), k
        assert own["phi_grid"][0, 0] == 0.0 and own["phi_grid"][0, -1] == own["phi_max"][0]
        assert own["t_grid"][0, -1] == min(1.5 * own["t_today"][0], 0.95 * own["t_max"][0])


def test_host_pointers_give_the_bits_of_device_pointers(Q):
    for name, n_a in (("thawing_h", 5000), ("wcdm_fixed", 64)):
        theta = fs.theta_of(name, fs.physical(name, 65, 41))
        m = _model(Q, name, n_a)
        a_q, phi_q, t_q = _given_queries(name, theta, n_a, (65, 2, 257), 4)
        for kw in (dict(a=a_q, phi=phi_q, t=t_q), dict(phi=5, t=9), dict()):
            dev, host = _np(Q.reconstruct(m, torch.from_numpy(theta).to(DEV), **kw)), Q.reconstruct_host(m, theta, **kw)
            assert sorted(dev) == sorted(host)
            for k in dev:
                assert _bits(dev[k], np.ascontiguousarray(host[k])), (name, k)


def test_host_pointers_beyond_one_piece_give_the_bits_of_device_pointers(pkg, Q):
    """cf_field stages 2^22 / (its widest query set) rows per piece: with the 4096 scale factors a call accepts at most that is
    1024, so 1025 rows cross one boundary and the second piece's row lands behind the first's in a per-point output, in scalars
    and in status.  16 nodes keep it cheap."""
    L, lib = pkg._lib, pkg.lib()
    n_aq = L.CF_FIELD_MAX_NQ
    S = (1 << 22) // n_aq + 1
    theta = fs.theta_of("thawing", fs.physical("thawing", S, 17))
    m = _model(Q, "thawing", 16)
    a_q = np.exp(np.random.default_rng(18).uniform(np.log(1e-8), np.log(5.0), n_aq))
    host = dict(phi_a=np.full((S, n_aq), SENTINEL), scalars=np.full((S, L.CF_FIELD_NSCALAR), SENTINEL), status=np.full(S, -1, dtype=np.int32))
    q, o = L.cf_field_queries(), L.cf_field_out()
    q.a_q, q.n_aq = a_q.ctypes.data, n_aq
    for k, v in host.items():
        setattr(o, k, v.ctypes.data)
    L.check(lib.cf_field(C.byref(m._desc), theta.ctypes.data, S, C.byref(q), C.byref(o)))
    x, daq = torch.from_numpy(theta).to(DEV), torch.from_numpy(a_q).to(DEV)
    dev = dict(phi_a=torch.full((S, n_aq), SENTINEL, dtype=torch.float64, device=DEV),
               scalars=torch.full((S, L.CF_FIELD_NSCALAR), SENTINEL, dtype=torch.float64, device=DEV),
               status=torch.full((S,), -1, dtype=torch.int32, device=DEV))
    q, o = L.cf_field_queries(), L.cf_field_out()
    q.a_q, q.n_aq = daq.data_ptr(), n_aq
    for k, v in dev.items():
        setattr(o, k, v.data_ptr())
    L.check(lib.cf_field_device(C.byref(m._desc), x.data_ptr(), S, C.byref(q), C.byref(o), torch.cuda.current_stream(DEV).cuda_stream))
    assert host["status"].tolist() == [fs.planted("thawing", S).get(i, 0) for i in range(S)]
    assert host["status"][S - 1] == 0 and (host["phi_a"][S - 1] != SENTINEL).all() and (host["scalars"][S - 1] != SENTINEL).all()
    for k, v in dev.items():
        assert _bits(host[k], v.cpu().numpy()), k


def test_null_outputs_are_skipped_and_nothing_is_written_past_an_output(pkg, Q):
    L, lib = pkg._lib, pkg.lib()
    name, n_a, S, n = "thawing", 65, 2, 65
    theta = fs.theta_of(name, fs.physical(name, S, 3))
    m = _model(Q, name, n_a)
    a_q, phi_q, t_q = _given_queries(name, theta, n_a, (n, n, n), 6)
    full = _np(Q.reconstruct(m, torch.from_numpy(theta).to(DEV), a=a_q, phi=phi_q, t=t_q))
    x = torch.from_numpy(theta).to(DEV)
    dq = {k: torch.from_numpy(v).to(DEV) for k, v in (("a_q", a_q), ("phi_q", phi_q), ("t_q", t_q))}
    stream = torch.cuda.current_stream(DEV).cuda_stream
    for only in ("phi_a", "V_a", "a_phi", "V_phi", "a_t", "phi_t", "scalars"):
        width = L.CF_FIELD_NSCALAR if only == "scalars" else n
        buf = torch.full((S * width + 64,), SENTINEL, dtype=torch.float64, device=DEV)
        q, o = L.cf_field_queries(), L.cf_field_out()
        q.a_q, q.phi_q, q.t_q, q.n_aq, q.n_phi, q.n_t = dq["a_q"].data_ptr(), dq["phi_q"].data_ptr(), dq["t_q"].data_ptr(), n, n, n
        setattr(o, only, buf.data_ptr())
        L.check(lib.cf_field_device(C.byref(m._desc), x.data_ptr(), S, C.byref(q), C.byref(o), stream))
        got = buf.cpu().numpy()
        assert (got[S * width:] == SENTINEL).all(), only
        want = np.stack([full[k] for k in L.FIELD_SCALARS], axis=1) if only == "scalars" else full[only]
        assert _bits(got[:S * width].reshape(S, width), np.ascontiguousarray(want)), only


def test_the_script_s_own_rows_at_its_own_sizes(Q):
    """The eight rows of the fixture (field.py run as it is) at 5000 nodes, 2000 field values and 1000 times, on the device."""
    g = golden("field")
    nodes = g["nodes"]
    a_nodes = np.linspace(1e-8, 5, 5000)[nodes]
    m = Q.Model(columns={"H0": 0, "Om": 1, "w0": 2})
    got = _np(Q.reconstruct(m, torch.from_numpy(np.ascontiguousarray(g["theta"])).to(DEV), a=a_nodes, phi=2000, t=1000))
    assert (got["status"] == 0).all()
    refs = [fr.row("thawing", *p, a_q=a_nodes, phi_q=2000, t_q=1000) for p in g["theta"]]
    _report("device vs restatement, the script's sizes", fs.compare(got, refs))
    thin = {k: got[k][:, ::10] for k in ("phi_grid", "V_phi", "t_grid", "a_t", "phi_t")}
    script = dict(phi_a=g["phi"], t_a=g["t"], K_a=g["K"], V_a=g["V"], phi_grid=g["phi_plot"], V_phi=g["V_of_phi"], t_grid=g["t_plot"],
                  a_t=g["a_of_t"], phi_t=g["phi_of_t"], phi_today=g["scalars"][:, 0], t_today=g["scalars"][:, 1], hubble_time=g["scalars"][:, 2])
    worst = {}
    for k, want in script.items():  # the script's float64 numbers in the role of the reference, same bars
        ref_rows = [dict(r, **{k: want[i].astype(np.longdouble) if want.ndim > 1 else np.longdouble(want[i])}) for i, r in enumerate(refs)]
        worst.update(fs.compare({k: thin.get(k, got[k])}, ref_rows))
    _report("device vs the script itself", worst)
    assert set(worst) == set(script)


def test_more_rows_than_one_grid_takes(pkg, Q):
    """One row above CF_FIELD_LAUNCH_ROWS and 65: the call runs as two grids, and the rows of the second (outputs offset per
    grid) carry the bits they have alone.  16 nodes, scalars, status and one query per set, so that the size is in the rows."""
    cap = pkg._lib.CF_FIELD_LAUNCH_ROWS
    S = cap + 66
    tail = fs.theta_of("thawing", fs.physical("thawing", 67, 91))  # rows cap - 1 .. cap + 65: the planted rows 7, 8, 9 among them
    x = torch.from_numpy(tail[:1]).to(DEV).repeat(S, 1)
    x[cap - 1:] = torch.from_numpy(tail).to(DEV)
    m = _model(Q, "thawing", 16)
    kw = dict(a=[0.5], phi=1, t=[3.0])
    big = Q.reconstruct(m, x, **kw)
    alone = Q.reconstruct(m, x[cap - 1:].contiguous(), **kw)
    for k, v in alone.items():
        if v.dim() >= 1 and v.shape[0] == 67:
            assert _bits(v.cpu().numpy(), big[k][cap - 1:].cpu().numpy()), k
    st = big["status"]
    assert st[cap - 1:].cpu().tolist() == [fs.planted("thawing", 67).get(i, 0) for i in range(67)]
    assert int(st[:cap - 1].sum()) == 0 and bool((big["t_today"][:cap - 1] == big["t_today"][0]).all())
