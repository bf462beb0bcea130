"""GPU (-m gpu): the three kernels of the template scan (csrc/cosmofit_scan.hip) through the handle-free
``cf_scan_apply_device`` on planted rows, at the shapes they accept (tests/scan_shapes.py: n around the k step, the 16-wide tile,
the 32-wide staged tile and the 64-wide block; K around the MFMA tile and the 64-wide column tile; S around a row block; every
sign; one shape of Pantheon+ size with 4096 candidates) -- against the long-double restatement (tests/scan_reference.py, which
never forms V); best against the device's own map to the bit; the bits of a row wherever it is computed; what lies in the
padding of the rows and beyond row S; non-finite rows; the column accumulators.

The accumulators are sums of the device's own scores, so they are judged against long-double sums of the device's map (1e-10 of
sum w |s| and of sum w s^2); the scores themselves are judged against the restatement."""
import ctypes as C

import numpy as np
import pytest
import torch

import scan_reference as SR
import scan_shapes as SS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LD = SR.LD
F64 = lambda x: np.asarray(x, dtype=np.float64)
ALL = ("best", "best_k", "s_best", "map")


@pytest.fixture(scope="module")
def SC(pkg):
    if pkg.lib().cf_device_count() < 1:
        pytest.fail("GPU tests need an MI355X; no HIP device visible (there is no fallback path)")
    return pkg.scan


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _same(a, b, keys=("best", "s_best", "map")):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in keys if k in a and k in b) and \
        ("best_k" not in a or "best_k" not in b or np.array_equal(a["best_k"], b["best_k"]))


class Apply:
    """One kernel shape: the scan on the device, the residual rows in a padded buffer, weights, and the device's results for all
    rows in one call (every output, the accumulators included) -- computed once and shared."""

    def __init__(self, pkg, SC, shape):
        self.c = c = SS.kernel_case(pkg, shape)
        self.n, self.K, self.sign, self.S = c.n, c.K, c.sign, c.S
        self.dec = SC.Scan(c.prep["V"], c.prep["live"], device=0)
        self.pitch = (c.n + 64) // 64 * 64  # at least one column of padding, as the residual rows of an engine have
        self.buf = torch.zeros((c.S + 3, self.pitch), dtype=torch.float64, device=DEV)
        self.buf[:c.S, :c.n] = _dev(c.rows)
        self.w = np.random.default_rng(c.n + c.K).uniform(0.0, 2.0, c.S)
        self.wd = _dev(self.w)
        self.acc = torch.zeros(2 * c.K + 1, dtype=torch.float64, device=DEV)
        self.res = _np(self.dec.apply(self.buf, S=c.S, sign=c.sign, weights=self.wd, want=ALL, colacc=self.acc))
        self.acc = self.acc.cpu().numpy()

    def call(self, buf, S=None, sign=None, want=ALL, **kw):
        return _np(self.dec.apply(buf, S=S, sign=self.sign if sign is None else sign, want=want, **kw))


_APPLY = {}
_ids = lambda s: "%d-%d-%d-%d" % s


@pytest.fixture(scope="module", params=SS.KERNEL + (SS.LARGE,), ids=_ids)
def ap(request, pkg, SC):
    if request.param not in _APPLY:
        _APPLY[request.param] = Apply(pkg, SC, request.param)
    return _APPLY[request.param]


def _own_best(m, live, sign):
    """(best, best_k, s_best) of a device map by numpy: the statistics of its own scores, the first maximum over the live ones."""
    stat = np.where(live[None, :], SR.statistic(m, sign), -1.0)
    k = stat.argmax(axis=1)
    r = np.arange(m.shape[0])
    return stat[r, k], k, m[r, k]


def test_apply_agrees_with_the_restatement_and_with_its_own_map(ap):
    c, r = ap.c, ap.res
    live = c.prep["live"]
    assert r["map"].shape == (ap.S, ap.K) and r["best"].shape == r["s_best"].shape == r["best_k"].shape == (ap.S,)
    assert np.isfinite(r["map"]).all() and not r["map"][:, ~live].any()                   # a dead candidate scores exactly 0.0
    e_map = np.abs(F64(r["map"][:, c.cols] - c.ref["s"]))
    e_s = np.abs(F64(r["s_best"] - c.s_best_ref))
    e_b = np.abs(F64(r["best"] - c.best_ref))
    some = c.tol > 0
    agree = r["best_k"] == c.best_k_ref
    print("n = %d K = %d m0 = %d sign = %d: map %.2e, s_best %.2e of the terms summed; best %.2e of 2 |s| x that; %d rows excused"
          % (c.shape + (float(np.max(e_map[some] / c.tol[some, None])) * SR.BAR if some.any() else 0.0,
                        float(np.max(e_s[some & agree] / c.tol[some & agree])) * SR.BAR if (some & agree).any() else 0.0,
                        float(np.max(e_b[c.best_tol > 0] / c.best_tol[c.best_tol > 0])) * SR.BAR if (c.best_tol > 0).any() else 0.0,
                        int(c.excused.sum()))))
    assert not e_map[~some].any() and (e_map <= c.tol[:, None]).all()
    assert (e_b <= c.best_tol).all()
    # the index: equal to the restatement's, rows with two leading statistics within twice the tolerance excused (at most 1 %;
    # tests/test_scan_cpu.py asserts that the restatement has none at these seeds)
    assert c.excused.mean() <= SS.EXCUSED_MAX and (agree | c.excused).all(), np.nonzero(~agree)[0]
    assert (e_s[agree] <= c.tol[agree]).all()
    # best is the maximum of the statistics of the device's own scores, to the bit, and best_k its first index
    best, k, s = _own_best(r["map"], live, ap.sign)
    assert np.array_equal(_bits(r["best"]), _bits(best)) and np.array_equal(r["best_k"], k) and np.array_equal(_bits(r["s_best"]), _bits(s))
    assert not c.rows[2].any() and r["best"][2] == 0.0 and r["best_k"][2] == int(np.argmax(live))  # a zero row: the first live one
    # a row does not depend on S
    for S in (SS.S_KERNEL if ap.S == SS.S_MAX else (1, 63)):
        got = ap.call(ap.buf, S=S)
        assert got["map"].shape == (S, ap.K) and _same(got, {k_: v[:S] for k_, v in r.items()}), (c.shape, S)


def test_bits_do_not_depend_on_position_company_outputs_sign_stream_or_repetition(ap, SC):
    c, r = ap.c, ap.res
    live = c.prep["live"]
    for p in (SS.POSITIONS if ap.S == SS.S_MAX else (0, 63)):
        got = ap.call(ap.buf[p:p + 1])
        assert _same(got, {k: v[p:p + 1] for k, v in r.items()}), (c.shape, "row", p)
    perm = np.random.default_rng(c.n + c.K).permutation(ap.S)
    got = ap.call(ap.buf[:ap.S][_dev(perm)].contiguous())
    assert _same(got, {k: v[perm] for k, v in r.items()}), "permuted rows"
    # a candidate alone, and among a few others
    for ks in ([0], [ap.K - 1], sorted({0, ap.K // 2, ap.K - 1})):
        few = SC.Scan(c.prep["V"][:, ks], live[ks], device=0)
        m = few.apply(ap.buf, S=ap.S, sign=ap.sign, want=("map",))["map"].cpu().numpy()
        assert np.array_equal(_bits(m), _bits(r["map"][:, ks])), (c.shape, ks)
        few.close()
    # with and without the optional outputs; the map under every sign; best under every sign from that map
    for want in (("best",), ("best_k",), ("s_best",), ("map",), ("best", "best_k", "s_best")):
        assert _same(ap.call(ap.buf, S=ap.S, want=want), r), want
    assert _same(ap.call(ap.buf, S=ap.S, want=("best",), colacc=torch.zeros(2 * ap.K + 1, dtype=torch.float64, device=DEV)), r)
    for sign in (0, 1, -1):
        got = ap.call(ap.buf, S=ap.S, sign=sign)
        best, k, s = _own_best(r["map"], live, sign)
        assert np.array_equal(_bits(got["map"]), _bits(r["map"])), sign
        assert np.array_equal(_bits(got["best"]), _bits(best)) and np.array_equal(got["best_k"], k) and np.array_equal(_bits(got["s_best"]), _bits(s))
    assert _same(ap.call(ap.buf, S=ap.S), r), "repeated"
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        got = ap.dec.apply(ap.buf, S=ap.S, sign=ap.sign, want=ALL)
    side.synchronize()
    assert _same(_np(got), r), "second stream"
    torch.cuda.synchronize()


def test_padding_rows_beyond_s_and_non_finite_rows(pkg, ap):
    c, r = ap.c, ap.res
    n, K, S = ap.n, ap.K, min(200, ap.S - 4)
    # NaN in the pad columns and in every row >= S (the weights included); the outputs padded too, their further rows untouched
    buf = ap.buf.clone()
    buf[:, n:] = float("nan")
    buf[S:, :] = float("nan")
    w = torch.cat([ap.wd, torch.zeros(3, dtype=torch.float64, device=DEV)])
    w[S:] = float("nan")
    best = torch.full((S + 2,), -7.0, dtype=torch.float64, device=DEV)
    s_best, k = best.clone(), torch.full((S + 2,), -7, dtype=torch.int32, device=DEV)
    m = torch.full((S + 2, K + 3), -7.0, dtype=torch.float64, device=DEV)
    acc = torch.zeros(2 * K + 1, dtype=torch.float64, device=DEV)
    pkg._lib.check(pkg.lib().cf_scan_apply_device(ap.dec._p, buf.data_ptr(), ap.pitch, S, ap.sign, w.data_ptr(), best.data_ptr(),
                                                  k.data_ptr(), s_best.data_ptr(), m.data_ptr(), K + 3, acc.data_ptr(),
                                                  torch.cuda.current_stream(DEV).cuda_stream))
    best, s_best, k, m, acc = (x.cpu().numpy() for x in (best, s_best, k, m, acc))
    assert np.array_equal(_bits(best[:S]), _bits(r["best"][:S])) and np.array_equal(_bits(s_best[:S]), _bits(r["s_best"][:S]))
    assert np.array_equal(k[:S], r["best_k"][:S]) and np.array_equal(_bits(m[:S, :K]), _bits(r["map"][:S]))
    assert (best[S:] == -7.0).all() and (k[S:] == -7).all() and (m[S:] == -7.0).all() and (m[:, K:] == -7.0).all()
    assert np.isfinite(acc).all()
    # NaN and inf inside a row: NaN / -1 in that row, no other row changes a bit
    buf = ap.buf.clone()
    bad_rows = [S // 3, S // 2, S // 2 + 1]
    buf[bad_rows[0], 0] = float("nan")
    buf[bad_rows[1], n - 1] = float("inf")
    buf[bad_rows[2], n // 2] = float("-inf")
    got = ap.call(buf, S=S)
    bad = np.zeros(S, dtype=bool)
    bad[bad_rows] = True
    assert np.isnan(got["best"][bad]).all() and np.isnan(got["s_best"][bad]).all() and (got["best_k"][bad] == -1).all()
    assert not np.isfinite(got["map"][bad]).all(axis=1).any()
    assert _same({k_: v[~bad] for k_, v in got.items()}, {k_: v[:S][~bad] for k_, v in r.items()})


def test_column_accumulators(pkg, ap):
    c, r = ap.c, ap.res
    K, S = ap.K, ap.S
    m, w = np.asarray(r["map"], dtype=LD), np.asarray(ap.w, dtype=LD)
    want1, want2, want_w = (w[:, None] * m).sum(axis=0), (w[:, None] * m * m).sum(axis=0), w.sum()
    tol1, tol2 = 1e-10 * F64((w[:, None] * np.abs(m)).sum(axis=0)), 1e-10 * F64(want2)
    acc = ap.acc
    print("n = %d K = %d: sum w s %.2e of sum w |s|, sum w s^2 %.2e relative" % (
        ap.n, K, float(np.max(np.abs(F64(acc[0:-1:2] - want1)) / np.maximum(tol1, 1e-300))) * 1e-10,
        float(np.max(np.abs(F64(acc[1:-1:2] - want2)) / np.maximum(tol2, 1e-300))) * 1e-10))
    assert (np.abs(F64(acc[0:-1:2] - want1)) <= tol1).all() and (np.abs(F64(acc[1:-1:2] - want2)) <= tol2).all()
    assert abs(float(acc[-1] - want_w)) <= 1e-10 * float(want_w)
    # the same cut again: the same bits, with or without the row outputs
    again = torch.zeros(2 * K + 1, dtype=torch.float64, device=DEV)
    ap.dec.apply(ap.buf, S=S, sign=ap.sign, weights=ap.wd, want=(), colacc=again)
    assert np.array_equal(_bits(again.cpu().numpy()), _bits(acc))
    # the host twin of the two reductions on the device's map: the same bits
    host = np.zeros(2 * K + 1)
    hb, hk, hs = np.empty(S), np.empty(S, dtype=np.int32), np.empty(S)
    lv = np.ascontiguousarray(c.prep["live"].astype(np.uint8))
    mm = np.ascontiguousarray(r["map"])
    assert pkg.lib().cf_selftest_scan_host(mm.ctypes.data, S, K, K, lv.ctypes.data, ap.sign, ap.w.ctypes.data, hb.ctypes.data,
                                     hk.ctypes.data, hs.ctypes.data, host.ctypes.data) == 0
    assert np.array_equal(_bits(host), _bits(acc)) and np.array_equal(_bits(hb), _bits(r["best"])) and np.array_equal(hk, r["best_k"])
    # another cut of the rows into calls: within the tolerance; repeated: the same bits
    if S > 100:
        cuts = []
        for _ in range(2):
            a = torch.zeros(2 * K + 1, dtype=torch.float64, device=DEV)
            ap.dec.apply(ap.buf[:100], sign=ap.sign, weights=ap.wd[:100].contiguous(), want=(), colacc=a)
            ap.dec.apply(ap.buf[100:S], sign=ap.sign, weights=ap.wd[100:S].contiguous(), want=(), colacc=a)
            cuts.append(a.cpu().numpy())
        assert np.array_equal(_bits(cuts[0]), _bits(cuts[1]))
        assert (np.abs(cuts[0][0:-1:2] - acc[0:-1:2]) <= tol1).all() and (np.abs(cuts[0][1:-1:2] - acc[1:-1:2]) <= tol2).all()
    # no weights: ones
    ones = torch.zeros(2 * K + 1, dtype=torch.float64, device=DEV)
    ap.dec.apply(ap.buf, S=S, sign=ap.sign, want=(), colacc=ones)
    ones = ones.cpu().numpy()
    assert ones[-1] == float(S) and (np.abs(F64(ones[1:-1:2] - (m * m).sum(axis=0))) <= 1e-10 * F64((m * m).sum(axis=0))).all()
    torch.cuda.synchronize()


def test_apply_refuses_bad_arguments(pkg, SC):
    ap = _APPLY.get((65, 65, 3, 1)) or Apply(pkg, SC, (65, 65, 3, 1))
    lib, p = pkg.lib(), ap.dec._p
    b = torch.empty((4,), dtype=torch.float64, device=DEV)
    m = torch.empty((4, 65), dtype=torch.float64, device=DEV)
    names = (("p", p), ("rows", ap.buf.data_ptr()), ("pitch", ap.pitch), ("S", 4), ("sign", 0), ("w", None), ("best", b.data_ptr()),
             ("k", None), ("s", None), ("map", None), ("mp", 0), ("acc", None), ("st", None))
    args = lambda **kw: [kw.get(k, d) for k, d in names]
    assert lib.cf_scan_apply_device(*args()) == 0
    assert lib.cf_scan_apply_device(*args(pitch=ap.n - 1)) == -1 and b"pitch below n" in lib.cf_last_error()
    assert lib.cf_scan_apply_device(*args(S=-1)) == -1 and lib.cf_scan_apply_device(*args(S=2**31)) == -1
    assert lib.cf_scan_apply_device(*args(sign=2)) == -1 and b"sign must be" in lib.cf_last_error()
    assert lib.cf_scan_apply_device(*args(best=None)) == -1 and b"no output" in lib.cf_last_error()
    assert lib.cf_scan_apply_device(*args(map=m.data_ptr(), mp=64)) == -1 and b"map pitch below K" in lib.cf_last_error()
    assert lib.cf_scan_apply_device(*args(map=m.data_ptr(), mp=65)) == 0
    assert lib.cf_scan_apply_device(*args(rows=None)) == -1 and lib.cf_scan_apply_device(*args(S=0, rows=None)) == 0
    n, K, dev, nl = C.c_int64(), C.c_int64(), C.c_int32(-1), C.c_int64()
    assert lib.cf_scan_info(p, C.byref(n), C.byref(K), C.byref(dev), C.byref(nl)) == 0
    assert (n.value, K.value, dev.value, nl.value) == (ap.n, ap.K, 0, int(ap.c.prep["live"].sum()))
    with pytest.raises(ValueError):
        ap.dec.apply(ap.buf.cpu())
    with pytest.raises(ValueError):
        ap.dec.apply(ap.buf[:, :ap.n - 1])
    with pytest.raises(ValueError):
        ap.dec.apply(ap.buf, want=("t",))
    torch.cuda.synchronize()
