"""GPU (-m gpu): the kernels of the leave-group-out fits (csrc/cosmofit_group.hip) at the shapes they accept.
``group_quad_kernel`` through ``Groups.from_precision`` / ``cf_group_quad_device``: n and m around the k step, the 16-wide tile,
the 64-wide column block and the 64-row workgroup, overlapping and shuffled groups, against the long-double restatement applied
to the device's own g; the bits of a row wherever and with whatever other groups it is computed; non-finite entries.
``cf_reweight_device`` against the restatement around the 2048-row slice."""
import ctypes as C

import numpy as np
import pytest
import torch

import infl_reference as IR
import infl_shapes as IS
import leaveout_reference as LR
import leaveout_shapes as LS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def LO(pkg):
    if pkg.lib().cf_device_count() < 1:
        pytest.fail("GPU tests need an MI355X; no HIP device visible (there is no fallback path)")
    return pkg.leaveout


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- group_quad_kernel ------------------------------------------------------------------------------------------------------------
class Quad:
    """A covariance of n data, its precision matrix and the groups on the device, g of 257 residual rows in a padded buffer, the
    restatement's q for them and the device's q of all rows in one call -- computed once per n and shared."""

    def __init__(self, pkg, LO, n):
        self.n = n
        self.chol = np.linalg.cholesky(IS.covariance(pkg, n))
        self.prec = pkg.influence.Precision(self.chol, device=0)
        self.K = IS.host_precision(pkg._lib, pkg.lib(), self.chol)[0]
        self.rows = IS.residual_rows(self.chol, LS.S_MAX, seed=n)
        self.pitch = (n + 64) // 64 * 64  # at least one column of padding
        self.buf = torch.zeros((LS.S_MAX + 3, self.pitch), dtype=torch.float64, device=DEV)
        self.prec.apply(torch.from_numpy(self.rows).to(DEV), out=self.buf[:LS.S_MAX])
        self.g = self.buf[:LS.S_MAX, :n].cpu().numpy()
        self.groups, self.n_sized = LS.quad_groups(n)
        self.G = LO.Groups.from_precision(self.prec, self.groups)
        ref = [LR.group_q(self.K, self.g, idx) for idx in self.groups]
        self.q_ref = np.stack([r[0] for r in ref], axis=1)
        self.tol = LR.BAR * np.asarray(np.stack([r[1] for r in ref], axis=1), dtype=np.float64)
        self.q = self.G.quad(self.buf, S=LS.S_MAX).cpu().numpy()


_QUAD = {}


@pytest.fixture(scope="module", params=LS.N_QUAD)
def qd(request, pkg, LO):
    if request.param not in _QUAD:
        _QUAD[request.param] = Quad(pkg, LO, request.param)
    return _QUAD[request.param]


def test_quad_agrees_with_the_restatement_over_shapes(qd):
    worst = 0.0
    for S in LS.S_QUAD:
        got = qd.G.quad(qd.buf, S=S).cpu().numpy()
        assert got.shape == (S, len(qd.groups))
        err = np.abs(np.asarray(got - qd.q_ref[:S], dtype=np.float64))
        assert (err <= qd.tol[:S]).all(), (qd.n, S, float(np.max(err / np.where(qd.tol[:S] > 0, qd.tol[:S], 1))))
        live = qd.tol[:S] > 0
        if live.any():
            worst = max(worst, float(np.max(err[live] / qd.tol[:S][live])) * LR.BAR)
        assert np.array_equal(_bits(got), _bits(qd.q[:S])), (qd.n, S)  # a row does not depend on S
        assert (got >= 0).all()
    print("n = %d, %d groups: largest |q - q_ref| / sum_j (sum_k |X_jk| |g_k|)^2 = %.2e" % (qd.n, len(qd.groups), worst))
    assert not qd.rows[2].any() and not _bits(qd.q[2]).any()  # a zero row gives +0.0
    info = qd.G.info()
    assert info["n"] == qd.n and info["n_groups"] == len(qd.groups) and info["max_m"] == qd.n
    assert np.array_equal(info["m"], [len(g) for g in qd.groups]) and np.array_equal(info["pitch"], (info["m"] + 15) // 16 * 16)
    assert info["bytes"] >= int((info["pitch"]**2).sum()) * 8


def test_singletons_are_influences_deletion_drop_and_the_whole_block_is_chi2(qd):
    kd = qd.prec.diag()
    single = qd.q[:, qd.n_sized:]
    drop = (qd.g * qd.g) / kd[None, :]                       # infl_row_kernel's own arithmetic
    rel = np.abs(single - drop) / np.where(drop > 0, drop, 1.0)
    print("n = %d: singleton q against g_i^2 / K_ii, largest difference %.2f eps" % (qd.n, rel.max() / IR.EPS))
    assert rel.max() <= 4 * IR.EPS
    whole = [k for k in range(qd.n_sized) if len(qd.groups[k]) == qd.n]
    assert len(whole) == 1
    chi2 = np.asarray((np.asarray(qd.rows, dtype=IR.LD) * np.asarray(qd.g, dtype=IR.LD)).sum(axis=1), dtype=np.float64)
    live = chi2 > 0
    rel = np.abs(qd.q[live, whole[0]] / chi2[live] - 1)
    print("n = %d: the whole-block group against chi^2, largest relative difference %.2e" % (qd.n, rel.max()))
    assert rel.max() <= 1e-10


def test_row_bits_do_not_depend_on_position_groups_stream_or_repetition(qd, LO):
    want = _bits(qd.q)
    for p in (0, 15, 16, 63, 64, 200, LS.S_MAX - 1):
        alone = qd.G.quad(qd.buf[p:p + 1]).cpu().numpy()
        assert np.array_equal(_bits(alone), want[p:p + 1]), (qd.n, "row", p)
    perm = np.random.default_rng(qd.n).permutation(LS.S_MAX)
    moved = qd.G.quad(qd.buf[:LS.S_MAX][torch.from_numpy(perm).to(DEV)].contiguous()).cpu().numpy()
    assert np.array_equal(_bits(moved), want[perm]), (qd.n, "permuted")
    assert np.array_equal(_bits(qd.G.quad(qd.buf, S=LS.S_MAX).cpu().numpy()), want), (qd.n, "repeated")
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        other = qd.G.quad(qd.buf, S=LS.S_MAX)
    side.synchronize()
    assert np.array_equal(_bits(other.cpu().numpy()), want), (qd.n, "second stream")
    # other groups absent, and in another order: a group's column keeps its bits
    pick = [k for k in (qd.n_sized - 1, 0, len(qd.groups) - 1) if k >= 0]
    with LO.Groups.from_precision(qd.prec, [qd.groups[k] for k in pick]) as few:
        got = few.quad(qd.buf, S=LS.S_MAX).cpu().numpy()
    assert np.array_equal(_bits(got), want[:, pick]), (qd.n, "a subset of the groups")


def test_padding_rows_beyond_s_and_non_finite_entries(qd):
    n, S = qd.n, 200
    clean = qd.q[:S]
    buf = qd.buf.clone()
    buf[:, n:] = float("nan")
    buf[S:, :] = float("nan")
    out = torch.full((S + 2, len(qd.groups) + 3), -7.0, dtype=torch.float64, device=DEV)
    qd.G.quad(buf, S=S, out=out)
    got = out.cpu().numpy()
    assert np.array_equal(_bits(got[:S, :len(qd.groups)]), _bits(clean))
    assert (got[:S, len(qd.groups):] == -7.0).all() and (got[S:] == -7.0).all()
    # one NaN and one inf: NaN in exactly the groups that hold the datum, in that row only
    buf = qd.buf.clone()
    hit = {17: 0, 90: n - 1}
    buf[17, 0], buf[90, n - 1] = float("nan"), float("inf")
    got = qd.G.quad(buf, S=S).cpu().numpy()
    want_nan = np.zeros((S, len(qd.groups)), dtype=bool)
    for s, i in hit.items():
        want_nan[s] = [i in g.tolist() for g in qd.groups]
    assert want_nan.any() and np.array_equal(np.isnan(got), want_nan)
    assert np.array_equal(_bits(got[~want_nan]), _bits(clean[~want_nan]))


def test_group_creation_refuses_on_the_device_what_it_must(pkg, LO):
    P = pkg.influence.Precision
    K = np.eye(6)
    K[3, :] = K[:, 3] = 0.0  # a datum the likelihood ignores
    prec = P(K, device=0, from_factor=False)
    with pytest.raises(pkg.CosmofitError, match="group 1 holds datum 3, which the likelihood ignores"):
        LO.Groups.from_precision(prec, [[0, 1], [2, 3]])
    off, idx, p = np.array([0, 2], dtype=np.int64), np.array([2, 3], dtype=np.int32), C.c_void_p()
    assert pkg.lib().cf_group_create(prec._p, 1, off.ctypes.data, idx.ctypes.data, C.byref(p)) == -1 and not p.value
    with LO.Groups.from_precision(prec, [[0, 1], [5, 2]]) as ok:
        g = torch.tensor([[1.0, 2.0, 3.0, 9.0, 9.0, 4.0]], dtype=torch.float64, device=DEV)
        assert ok.quad(g).cpu().numpy().tolist() == [[5.0, 25.0]]
        with pytest.raises(ValueError):
            ok.quad(g[:, :5])
        assert pkg.lib().cf_group_quad_device(ok._p, g.data_ptr(), 5, 1, g.data_ptr(), 2, None) == -1
    K = np.eye(4)
    K[1, 2] = K[2, 1] = 2.0  # indefinite in the pair (1, 2)
    with pytest.raises(pkg.CosmofitError, match="group 1: non-positive pivot at column 1"):
        LO.Groups.from_precision(P(K, device=0, from_factor=False), [[0], [1, 2], [3]])


# ---- cf_reweight_device -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", LS.S_RW)
def test_reweight_record_agrees_with_the_restatement(LO, S):
    worst = 0.0
    for G in LS.G_RW:
        for ncol in LS.NCOL_RW:
            lw, w0, x, pivot = LS.reweight_inputs(S, G, ncol)
            ref, scale = LR.reweight_record(lw, w0, x, pivot)
            d = [torch.from_numpy(a).to(DEV) for a in (lw, x, w0)]
            rec = LO.reweight_record(d[0], d[1], d[2], pivot)
            got = rec.cpu().numpy()
            assert got.shape == ref.shape
            for k, name in enumerate(LR.RW_SLOTS):
                if name in ("lmax", "n_used", "n_skipped"):
                    assert np.array_equal(got[:, k], np.asarray(ref[:, k], dtype=np.float64)), (S, G, ncol, name)
            err = np.abs(np.asarray(got - ref, dtype=np.float64))
            tol = LR.BAR * np.asarray(scale, dtype=np.float64)
            tol[:, 3] = LR.BAR * np.asarray(ref[:, 3], dtype=np.float64)  # the largest weight: one exp
            summed = np.ones(got.shape[1], dtype=bool)
            summed[[0, 4, 5]] = False
            assert (err[:, summed] <= tol[:, summed]).all(), (S, G, ncol)
            live = tol > 0
            worst = max(worst, float(np.max(err[live] / tol[live])) * LR.BAR if live.any() else 0.0)
            assert (got[:, 1:4] >= 0).all() and (got[:, 3] <= 2.0).all()
            # the same bits repeated, on a second stream, and for a column evaluated alone (in place and as a copy)
            assert np.array_equal(_bits(LO.reweight_record(d[0], d[1], d[2], pivot).cpu().numpy()), _bits(got))
            side = torch.cuda.Stream(device=DEV)
            side.wait_stream(torch.cuda.current_stream(DEV))
            with torch.cuda.stream(side):
                other = LO.reweight_record(d[0], d[1], d[2], pivot)
            side.synchronize()
            assert np.array_equal(_bits(other.cpu().numpy()), _bits(got))
            b = G - 1
            for col in (d[0][:, b:b + 1], d[0][:, b:b + 1].contiguous()):
                alone = LO.reweight_record(col, d[1], d[2], pivot).cpu().numpy()
                assert np.array_equal(_bits(alone[0]), _bits(got[b])), (S, G, ncol, "a column alone")
            if G == 3 and ncol == 4:  # no base weights: ones
                ref1, scale1 = LR.reweight_record(lw, None, x, pivot)
                got1 = LO.reweight_record(d[0], d[1], None, pivot).cpu().numpy()
                assert (np.abs(np.asarray(got1 - ref1, dtype=np.float64)) <= LR.BAR * np.maximum(np.asarray(scale1, dtype=np.float64), np.abs(np.asarray(ref1, dtype=np.float64)))).all()
    print("S = %d: largest |record - restatement| on the scale of the terms summed = %.2e" % (S, worst))


def test_reweight_summary_of_a_column_without_used_rows_and_of_minus_infinity(LO):
    S = 40
    lw = torch.zeros((S, 3), dtype=torch.float64, device=DEV)
    lw[:, 0] = float("nan")
    lw[:, 1] = -float("inf")
    lw[5:, 2] = -float("inf")
    x = torch.arange(S, dtype=torch.float64, device=DEV)[:, None] * torch.ones((1, 2), dtype=torch.float64, device=DEV)
    rec = LO.reweight_record(lw, x, None, np.zeros(2)).cpu().numpy()
    assert rec[0, 0] == -np.inf and rec[0, 4] == 0 and rec[0, 5] == S and not rec[0, 1:4].any()
    assert rec[1, 0] == -np.inf and rec[1, 4] == S and rec[1, 5] == 0 and not rec[1, 1:4].any() and rec[1, 6] == S
    assert rec[2, 0] == 0.0 and rec[2, 1] == 5.0 and rec[2, 3] == 1.0 and rec[2, 8] == 10.0 and rec[2, 10] == 30.0
    out = LO.reweight(lw[:, 2], x)
    assert out["mean"][0].tolist() == [2.0, 2.0] and out["ess"][0] == 5.0 and out["n_used"][0] == S and out["khat"][0] == np.inf
    assert not out["reliable"][0]
