"""
What happens if you drop them: the chi^2 a GROUP of data carries given all the others, and the posterior without the group, from
one chain that lives on the device -- no new engine, no new covariance factor and no new sampling run per cut.

``influence`` holds the vector that answers it, g = K r with K = C^-1.  For a group B of m data (csrc/cosmofit_group.hip):

* ``q_B = g_B^T (K_BB)^-1 g_B >= 0`` is the chi^2 of the group's leave-group-out residual ``e_B = K_BB^-1 g_B = r_B - C_BA C_AA^-1
  r_A`` (covariance ``K_BB^-1``, m degrees of freedom under the model); ``influence``'s ``g_i^2 / K_ii`` is the case m = 1;
* chi^2 of the data without B is ``chi^2 - q_B`` exactly -- no refit of the covariance;
* the posterior without B is the chain reweighted by ``exp(+q_B / 2)``.

So one chain plus one pass gives, for every group of a partition (or of any list of groups: they may overlap, as nested redshift
cuts do), the group's consistency statistic, the shift of every parameter when the group is removed, and an honest reliability
flag for that answer (the effective sample size and the Pareto tail index of the weights).

* ``groups_from_labels(labels)`` / ``groups_from_edges(z, edges)``: index lists and names.
* ``Groups(engine, groups, block)``: the ``cf_group`` on the engine's device, built on ``engine.precision(block)``.
* ``group_chi2(engine, theta, groups, block)``: q [S, G] on the device and dof [G].
* ``reweight(log_w, x, base_weights, names)``: the importance summary of ANY log-weights (``cf_reweight_device``).
* ``leave_group_out(engine, chain, groups, ...)``: everything above per group.

block: "sn" or "bao".  The inputs are float64 tensors on the engine's MI355X; there is no CPU or tensor fallback.  Out of scope:
quasar engines, engines over several devices, the CC / growth-rate / CMB blocks, groups beyond 1024 data or 1024 groups.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from . import fit_report as F
from . import influence as I
from ._args import on_device, ptr, row_weights, sample_rows, stream_of

PIECE = 65536  # rows of g formed at a time by group_chi2
KHAT_RELIABLE = 0.7  # Vehtari, Simpson, Gelman, Yao & Gabry, "Pareto smoothed importance sampling": the published threshold
_LGO_KEYS = ("groups", "block", "weights", "columns", "theta_ref", "names")



# ---- groups ---------------------------------------------------------------------------------------------------------------------
def groups_from_labels(labels):
    """(groups, names): one group per distinct label (a survey, a tracer), in the order of first appearance; groups[k] holds the
    indices of the data that carry names[k], ascending."""
    labels = np.asarray(labels)
    if labels.ndim != 1 or labels.size < 1:
        raise ValueError("groups_from_labels takes one label per datum")
    names, groups = [], []
    for lab in labels.tolist():
        if lab not in names:
            names.append(lab)
    for lab in names:
        groups.append(np.nonzero(labels == lab)[0].astype(np.int32))
    return groups, [str(x) for x in names]


def groups_from_edges(z, edges):
    """(groups, names): one group per bin [edges[k], edges[k + 1]) of z that holds a datum (the last bin closed above), named by
    its edges.  Data outside the edges are in no group."""
    z, edges = np.asarray(z, dtype=np.float64), np.asarray(edges, dtype=np.float64)
    if z.ndim != 1 or edges.ndim != 1 or edges.size < 2 or not (np.diff(edges) > 0).all() or not np.isfinite(edges).all():
        raise ValueError("groups_from_edges takes z [n] and at least two finite ascending edges")
    groups, names = [], []
    for k in range(edges.size - 1):
        hi = z <= edges[k + 1] if k == edges.size - 2 else z < edges[k + 1]
        idx = np.nonzero((z >= edges[k]) & hi)[0].astype(np.int32)
        if idx.size:
            groups.append(idx)
            names.append("z[%g,%g%s" % (edges[k], edges[k + 1], "]" if k == edges.size - 2 else ")"))
    if not groups:
        raise ValueError("groups_from_edges: no datum lies inside the edges")
    return groups, names


def pack_groups(groups):
    """(offsets int64 [G + 1], idx int32) of a list of index lists, as cf_group_create takes them (shape rules only)."""
    if isinstance(groups, np.ndarray) and groups.ndim == 1:
        groups = [groups]
    try:
        lists = [np.asarray(g) for g in groups]
    except Exception:
        raise ValueError("groups must be a list of index lists") from None
    if not lists:
        raise ValueError("groups must hold at least one group")
    for k, g in enumerate(lists):
        if g.ndim != 1 or g.size < 1 or not np.issubdtype(g.dtype, np.integer):
            raise ValueError(f"group {k} must be a non-empty list of integer indices")
        if g.min() < -2**31 or g.max() >= 2**31:
            raise ValueError(f"group {k} has an index outside 0..n-1")
    offsets = np.zeros(len(lists) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([g.size for g in lists])
    return offsets, np.ascontiguousarray(np.concatenate(lists), dtype=np.int32)


def check_groups(groups, n: int, kdiag=None):
    """The argument rules of ``cf_group_create`` without a device (``cf_group_check_args``): returns (offsets, idx) or raises
    ``CosmofitError`` naming the group."""
    offsets, idx = pack_groups(groups)
    kd = None if kdiag is None else np.ascontiguousarray(kdiag, dtype=np.float64)
    L.check(L.lib().cf_group_check_args(int(n), None if kd is None else ptr(kd), len(offsets) - 1, ptr(offsets), ptr(idx)))
    return offsets, idx


class Groups:
    """The groups of one block of an engine on its device (``cf_group``): per group the inverse Cholesky factor of K_BB, formed on
    the host in extended precision from ``engine.precision(block)``.  ``close()`` releases it."""

    def __init__(self, engine, groups, block: str = "sn", names: Optional[Sequence[str]] = None):
        n = F._check_engine(engine, block, "leaveout.Groups")
        self._check(groups, n, names)
        self.engine, self.block = engine, block
        self._build(engine.precision(block))

    @classmethod
    def from_precision(cls, prec: "I.Precision", groups, names: Optional[Sequence[str]] = None) -> "Groups":
        """The groups over the data of a bare ``influence.Precision`` (no engine: ``quad`` takes g from ``prec.apply``)."""
        self = cls.__new__(cls)
        self._check(groups, prec.n, names)
        self.engine, self.block = None, None
        self._build(prec)
        return self

    def _check(self, groups, n: int, names):
        """Every argument rule that needs no device, before any device work."""
        self._p = C.c_void_p()
        self.n = int(n)
        self.offsets, self.idx = check_groups(groups, n)
        self.n_groups = len(self.offsets) - 1
        if names is not None and len(names) != self.n_groups:
            raise ValueError("names must be one per group")
        self.names = [str(x) for x in names] if names is not None else [f"group{k}" for k in range(self.n_groups)]
        self.dof = np.diff(self.offsets).astype(np.int64)

    def _build(self, prec):
        self.device = prec.device
        L.check(L.lib().cf_group_check_args(self.n, ptr(prec.diag()), self.n_groups, ptr(self.offsets), ptr(self.idx)))
        L.check(L.lib().cf_group_create(prec._p, self.n_groups, ptr(self.offsets), ptr(self.idx), C.byref(self._p)))

    def close(self):
        if getattr(self, "_p", None) is not None and self._p.value:
            L.lib().cf_group_destroy(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def group(self, k: int) -> np.ndarray:
        return self.idx[self.offsets[k]:self.offsets[k + 1]]

    def info(self) -> dict:
        """n, n_groups, device, max_m, n_idx, bytes (held on the device), m [G], pitch [G] (m rounded up to 16)."""
        out, m, pitch = np.zeros(6, dtype=np.int64), np.zeros(self.n_groups, dtype=np.int64), np.zeros(self.n_groups, dtype=np.int64)
        L.check(L.lib().cf_group_info(self._p, ptr(out), ptr(m), ptr(pitch)))
        return dict(zip(("n", "n_groups", "device", "max_m", "n_idx", "bytes"), out.tolist()), m=m, pitch=pitch)

    def quad(self, g: torch.Tensor, S: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """q [S, G] of the rows g[:S, :n] (``cf_group_quad_device``), asynchronous on torch's current stream.  g: float64
        [>= S, pitch >= n] with contiguous columns on the device of the groups; rows >= S and columns >= n are never read."""
        if not isinstance(g, torch.Tensor) or g.dtype != torch.float64 or g.dim() != 2 or g.stride(1) != 1:
            raise ValueError("Groups.quad takes a float64 tensor [S, >= n] with contiguous columns")
        if not g.is_cuda or g.device.index != self.device:
            raise ValueError("Groups.quad takes g on the device of the groups")
        S = g.shape[0] if S is None else int(S)
        if not 0 <= S <= g.shape[0] or g.shape[1] < self.n:
            raise ValueError("Groups.quad: S rows of at least n columns")
        q = torch.empty((S, self.n_groups), dtype=torch.float64, device=g.device) if out is None else out
        if S:
            with torch.cuda.device(g.device):
                L.check(L.lib().cf_group_quad_device(self._p, g.data_ptr(), g.stride(0), S, q.data_ptr(), q.stride(0),
                                                     stream_of(g.device)))
        return q


def group_chi2(engine, theta, groups, block: str = "sn", piece: int = PIECE):
    """(q [S, G] on the device, dof [G] numpy): for every row of theta [S, ndim] and every group B, q_B = the chi^2 the group
    carries given all the other data; ``chi^2 - q_B`` is the chi^2 of the data without the group.  groups: a ``Groups`` of this
    engine and block, or a list of index lists (a ``Groups`` is built and released).  g is formed in pieces of at most `piece`
    (<= 65536) rows, so its memory stays bounded; a row's q does not depend on the piece size."""
    n = F._check_engine(engine, block, "leaveout.group_chi2")
    if not 1 <= int(piece) <= PIECE:
        raise ValueError(f"piece must be in 1..{PIECE}")
    own = not isinstance(groups, Groups)
    if own:
        check_groups(groups, n)
    elif groups.engine is not engine or groups.block != block:
        raise ValueError("these Groups were built for another engine or block")
    x = I._theta_rows(engine, theta, "leaveout.group_chi2")
    G = Groups(engine, groups, block) if own else groups
    try:
        q = torch.empty((x.shape[0], G.n_groups), dtype=torch.float64, device=x.device)
        for s0 in range(0, x.shape[0], int(piece)):
            g = I.rows(engine, x[s0:s0 + int(piece)], block, want=("g",))["g"]
            G.quad(g, out=q[s0:s0 + int(piece)])
        if own:
            torch.cuda.synchronize(x.device)
        return q, G.dof.copy()
    finally:
        if own:
            G.close()


# ---- importance reweighting -----------------------------------------------------------------------------------------------------
def tail_length(n_used: int) -> int:
    """M = min(S / 5, 3 sqrt(S)): the number of largest weights the tail index is fitted to (PSIS)."""
    return int(min(n_used // 5, np.floor(3.0 * np.sqrt(n_used))))


def gpd_khat(exceed: np.ndarray) -> float:
    """The shape k of the generalized Pareto distribution fitted to the exceedances (> 0, any order) by the profile estimator
    of Zhang & Stephens (2009, Technometrics 51, 316) with the weakly informative prior of Vehtari et al.'s PSIS (ten
    pseudo-observations of k = 0.5).  inf for fewer than five exceedances, a non-positive or non-finite one, or no spread."""
    x = np.sort(np.asarray(exceed, dtype=np.float64))
    n = x.size
    if n < 5 or not np.isfinite(x).all() or not x[0] > 0.0 or not x[-1] > x[0]:
        return float("inf")
    m = 30 + int(np.sqrt(n))
    b = 1.0 - np.sqrt(m / (np.arange(1, m + 1, dtype=np.float64) - 0.5))
    b = b / (3.0 * x[int(n / 4 + 0.5) - 1]) + 1.0 / x[-1]
    k = np.log1p(-b[:, None] * x[None, :]).mean(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        ll = n * (np.log(-(b / k)) - k - 1.0)
    ll = np.where(np.isfinite(ll), ll, -np.inf)
    w = np.exp(ll - ll.max())
    w /= w.sum()
    b_post = float((b * w).sum())
    k_post = float(np.log1p(-b_post * x).mean())
    return (n * k_post + 10 * 0.5) / (n + 10)


def _as_columns(t, what: str, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what} takes {name} as a tensor on an MI355X (there is no CPU implementation to fall back to)")
    if t.dtype != torch.float64:
        raise ValueError(f"{what} takes {name} as float64")
    if t.dim() == 1:
        t = t[:, None]
    if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"{what} takes {name} [S] or [S, k] with S >= 1")
    return t


def _check_reweight(log_w, x, base_weights, names, what="leaveout.reweight"):
    """Every rule of ``reweight`` that needs no device; returns (lw [S, G], x [S, ncol], w0 or None, names)."""
    lw, x = _as_columns(log_w, what, "log_w"), _as_columns(x, what, "x")
    S, G, ncol = lw.shape[0], lw.shape[1], x.shape[1]
    if x.shape[0] != S:
        raise ValueError(f"{what}: log_w and x must have one row per sample")
    if S > 2**31:
        raise ValueError(f"{what} takes at most 2^31 rows")
    if G > L.CF_RW_MAX_G:
        raise ValueError(f"{what} takes at most {L.CF_RW_MAX_G} columns of log_w")
    if ncol > L.CF_RW_MAX_NCOL:
        raise ValueError(f"{what} takes at most {L.CF_RW_MAX_NCOL} columns of x")
    if names is not None and len(names) != G:
        raise ValueError("names must be one per column of log_w")
    if lw.device != x.device:
        raise ValueError(f"{what}: log_w and x must be on one device")
    w0 = None
    if base_weights is not None:
        if not isinstance(base_weights, torch.Tensor) or base_weights.dtype != torch.float64:
            raise ValueError(f"{what} takes base_weights as a float64 tensor")
        if base_weights.dim() != 1 or base_weights.shape[0] != S:
            raise ValueError("base_weights must be [S], one per sample")
        if base_weights.device != x.device:
            raise ValueError("base_weights must be on the device of the samples")
        w0 = base_weights
    names = [str(n) for n in names] if names is not None else [f"w{k}" for k in range(G)]
    return lw, x, w0, names


def reweight_record(lw: torch.Tensor, x: torch.Tensor, w0: Optional[torch.Tensor], pivot: np.ndarray) -> torch.Tensor:
    """The raw records [G, CF_RW_NCOL(ncol)] of ``cf_reweight_device`` on the device (inputs as ``_check_reweight`` returns them,
    on an MI355X), asynchronous on torch's current stream."""
    on_device(x, "leaveout.reweight")
    lw = lw if lw.stride(1) == 1 else lw.contiguous()
    x = x if x.stride(1) == 1 else x.contiguous()
    w0 = None if w0 is None else w0.contiguous()
    S, G, ncol = lw.shape[0], lw.shape[1], x.shape[1]
    pivot = np.ascontiguousarray(pivot, dtype=np.float64)
    out = torch.empty((G, L.rw_ncol(ncol)), dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        L.check(L.lib().cf_reweight_device(lw.data_ptr(), lw.stride(0), S, G, None if w0 is None else w0.data_ptr(), x.data_ptr(),
                                           x.stride(0), ncol, ptr(pivot), out.data_ptr(),
                                           stream_of(x.device)))
    return out


def summary_from_record(rec: np.ndarray, pivot: np.ndarray) -> dict:
    """The per-column summary of records [G, CF_RW_NCOL(ncol)] (host arithmetic; ``reweight`` documents the keys)."""
    rec, pivot = np.asarray(rec, dtype=np.float64), np.asarray(pivot, dtype=np.float64)
    G, ncol = rec.shape[0], pivot.size
    col = {name: rec[:, k] for k, name in enumerate(L.RW_SLOTS)}
    iu = np.triu_indices(ncol)
    with np.errstate(divide="ignore", invalid="ignore"):
        m1 = rec[:, L.CF_RW_MEAN:L.CF_RW_MEAN + ncol] / col["sum_w"][:, None]
        m2 = np.zeros((G, ncol, ncol))
        m2[:, iu[0], iu[1]] = rec[:, L.CF_RW_MEAN + ncol:] / col["sum_w"][:, None]
        m2[:, iu[1], iu[0]] = m2[:, iu[0], iu[1]]
        cov = m2 - m1[:, :, None] * m1[:, None, :]
        ess = col["sum_w"]**2 / col["sum_w2"]
        ess_base = col["sum_w0"]**2 / col["sum_w0_sq"]
        return dict(log_mean_weight=col["lmax"] + np.log(col["sum_w"] / col["sum_w0"]), ess=ess, ess_fraction=ess / ess_base,
                    max_weight_share=col["max_w"] / col["sum_w"], mean=pivot[None, :] + m1, cov=cov,
                    std=np.sqrt(np.maximum(np.diagonal(cov, axis1=1, axis2=2), 0.0)), n_used=col["n_used"].astype(np.int64),
                    n_skipped=col["n_skipped"].astype(np.int64), lmax=col["lmax"].copy())


def _khat_columns(lw: torch.Tensor, x: torch.Tensor, w0: Optional[torch.Tensor], lmax: np.ndarray, n_used: np.ndarray) -> np.ndarray:
    """khat per column from the M + 1 largest weights of its used rows (``torch.topk`` on the device, the fit on the host)."""
    S, G = lw.shape
    ok = torch.isfinite(x).all(dim=1)
    if w0 is not None:
        ok &= torch.isfinite(w0) & (w0 >= 0)
    out = np.full(G, np.inf)
    step = max(1, (1 << 24) // S)
    for b0 in range(0, G, step):
        cols = lw[:, b0:b0 + step]
        used = ok[:, None] & ~torch.isnan(cols) & (cols != float("inf"))
        lm = torch.from_numpy(np.where(np.isfinite(lmax[b0:b0 + step]), lmax[b0:b0 + step], 0.0)).to(lw.device)
        w = torch.exp(torch.where(used, cols, torch.full_like(cols, -float("inf"))) - lm[None, :])
        if w0 is not None:
            w = torch.where(used, w * w0[:, None], torch.zeros_like(w))
        for b in range(b0, min(G, b0 + step)):
            M = tail_length(int(n_used[b]))
            if M < 5:
                continue
            top = torch.topk(w[:, b - b0], M + 1).values.cpu().numpy()
            ex = top[:M] - top[M]
            out[b] = gpd_khat(ex[ex > 0.0])  # strictly above the cutoff, as PSIS: a chain's repeated rows tie with it
    return out


def reweight(log_w, x, base_weights=None, names=None) -> dict:
    """Importance-reweight a chain that lives on the device: the posterior whose density is the chain's times ``exp(log_w)``.

    log_w: [S] or [S, G], one column per reweighting; x: [S, ncol <= 16], the columns to summarise (the parameters, derived
    quantities); base_weights: [S] finite and >= 0 (a nested posterior's), default ones.  A row is skipped for a column, and
    counted, when its log_w is NaN or +inf, when any of its x is non-finite, or when its base weight is not a finite number
    >= 0; log_w = -inf is weight 0.  The weights are scaled by the largest log_w among the rows of positive base weight, so
    the early points of a nested run (base weight exp(-40000) = 0, log_w enormous) cannot underflow all the others.  Where the
    weights of a column still span more than the range of a double (a tiny positive base weight under an enormous log_w) its
    sums underflow: ess and the moments are NaN, khat is inf and reliable is False -- the reweighted answer does not exist.  Returns per column of log_w (numpy, leading axis G):

      log_mean_weight   ln of the mean weight: ln of the evidence ratio when log_w is a log-likelihood difference
      ess, ess_fraction (sum w)^2 / sum w^2, and its ratio to the same of the base weights
      max_weight_share  the largest single weight over the sum
      khat, reliable    the generalized-Pareto tail index of the M = min(S / 5, 3 sqrt(S)) largest weights (Zhang & Stephens
                        2009 with the weak prior of Vehtari et al.'s PSIS); reliable = khat < 0.7, their published threshold
      mean [G, ncol], cov [G, ncol, ncol], std [G, ncol]
      n_used, n_skipped, names

    Two uses.  Adding a Gaussian H0 prior to a chain sampled without it (the ``*_H0trgb`` scripts differ from their parents by
    this one term)::

        out = leaveout.reweight(-0.5 * ((chain[:, i_H0] - 69.96) / 1.53) ** 2, chain)

    Adding a second engine's likelihood (SN chain, BAO added afterwards)::

        out = leaveout.reweight(bao.engine.torch_log_likelihood()(chain), chain)

    The sums run on the device in a fixed order (``cf_reweight_device``); the same inputs give the same bits."""
    lw, x, w0, names = _check_reweight(log_w, x, base_weights, names)
    on_device(x, "leaveout.reweight")
    ok = torch.isfinite(x).all(dim=1)
    wb = torch.ones(x.shape[0], dtype=torch.float64, device=x.device) if w0 is None else torch.where(torch.isfinite(w0) & (w0 >= 0), w0, torch.zeros_like(w0))
    wb = torch.where(ok, wb, torch.zeros_like(wb))
    tot = float(wb.sum())
    pivot = ((wb[:, None] * torch.where(ok[:, None], x, torch.zeros_like(x))).sum(dim=0) / tot).cpu().numpy() if tot > 0 else np.zeros(x.shape[1])
    pivot = np.where(np.isfinite(pivot), pivot, 0.0)
    rec = reweight_record(lw, x, w0, pivot).cpu().numpy()
    out = summary_from_record(rec, pivot)
    out["khat"] = _khat_columns(lw, x, w0, out["lmax"], out["n_used"])
    out["reliable"] = out["khat"] < KHAT_RELIABLE
    out["names"] = names
    return out


# ---- leave-group-out ------------------------------------------------------------------------------------------------------------
def leave_group_out(engine, chain, groups, block: str = "sn", weights=None, columns=None, theta_ref=None, names=None) -> dict:
    """For every group B: what the chain says about the data without it.

    chain: [S, ndim] on the engine's device; groups: a ``Groups`` or a list of index lists (they may overlap); weights: base
    weights [S] (a nested posterior's); columns: derived columns [S, k] summarised beside theta (ndim + k <= 16); theta_ref:
    one theta [ndim] at which q is quoted.  Returns ``q`` [S, G] on the device and, per group (numpy, leading axis G):

      dof, q_mean, q_std     the size m of the group, the posterior mean and scatter of q_B
      q_ref, p_ref           with theta_ref: q_B there and chi2.sf(q_ref, dof).  With parameters fitted on ALL the data (B
                             included) the chi^2 law of q_B holds only asymptotically (Wilks); ``mocks`` calibrates it.
      mean, std, cov         of the posterior without the group: the chain reweighted by exp(+q_B / 2)
      shift_sigma            (mean_b - mean_full) / std_full, per column
      width_ratio            std_b / std_full
      ess, ess_fraction, max_weight_share, khat, reliable, log_mean_weight, n_used, n_skipped     as ``reweight``
      mean_full, std_full, names

    A group whose removal moves the posterior far has few effective samples and khat >= 0.7: then the reweighted numbers are
    not to be trusted and a direct run on the reduced data is the answer (examples/union3_leaveout.py shows both)."""
    n = F._check_engine(engine, block, "leaveout.leave_group_out")
    x = sample_rows(chain, engine.ndim, "leaveout.leave_group_out") if isinstance(chain, torch.Tensor) and chain.dim() == 2 else None
    if x is None:
        raise ValueError(f"leaveout.leave_group_out takes the chain as a float64 tensor [S, {engine.ndim}] on an MI355X")
    if x.shape[0] < 1:
        raise ValueError("leaveout.leave_group_out needs at least one row")
    w0 = row_weights(weights, x, "leaveout.leave_group_out")
    cols = x
    if columns is not None:
        extra = _as_columns(columns, "leaveout.leave_group_out", "columns")
        if extra.shape[0] != x.shape[0] or extra.device != x.device:
            raise ValueError("columns must be [S, k] on the device of the chain")
        cols = torch.cat([x, extra], dim=1)
    if cols.shape[1] > L.CF_RW_MAX_NCOL:
        raise ValueError(f"theta and the derived columns together must be at most {L.CF_RW_MAX_NCOL}")
    ref = None
    if theta_ref is not None:
        ref = np.asarray(theta_ref.cpu() if isinstance(theta_ref, torch.Tensor) else theta_ref, dtype=np.float64).reshape(-1)
        if ref.shape != (engine.ndim,):
            raise ValueError(f"theta_ref must be one theta [{engine.ndim}]")
    own = not isinstance(groups, Groups)
    if own:
        check_groups(groups, n)
    G = Groups(engine, groups, block, names) if own else groups
    try:
        q, dof = group_chi2(engine, x, G, block)
        out = reweight(0.5 * q, cols, w0, G.names)
        full = reweight(torch.zeros((x.shape[0], 1), dtype=torch.float64, device=x.device), cols, w0)
        wb = torch.ones(x.shape[0], dtype=torch.float64, device=x.device) if w0 is None else w0
        wb = torch.where(torch.isfinite(cols).all(dim=1), wb, torch.zeros_like(wb))
        wq = torch.where(torch.isfinite(q), wb[:, None], torch.zeros_like(q))
        qz = torch.where(torch.isfinite(q), q, torch.zeros_like(q))
        wsum = wq.sum(dim=0)
        q_mean = (wq * qz).sum(dim=0) / wsum
        q_var = (wq * (qz - q_mean[None, :])**2).sum(dim=0) / wsum
        out.update(q=q, dof=dof, q_mean=q_mean.cpu().numpy(), q_std=torch.sqrt(q_var).cpu().numpy(),
                   mean_full=full["mean"][0], std_full=full["std"][0])
        with np.errstate(divide="ignore", invalid="ignore"):
            out["shift_sigma"] = (out["mean"] - out["mean_full"][None, :]) / out["std_full"][None, :]
            out["width_ratio"] = out["std"] / out["std_full"][None, :]
        if ref is not None:
            from scipy.stats import chi2 as chi2_dist

            out["q_ref"] = group_chi2(engine, ref[None, :], G, block)[0][0].cpu().numpy()
            out["p_ref"] = chi2_dist.sf(out["q_ref"], dof)
        return out
    finally:
        if own:
            G.close()


def chain_leave_group_out(engine, chain, **kw) -> dict:
    """``leave_group_out`` with its keywords checked by name: what ``ShardedEnsemble.leave_group_out`` and
    ``DeviceNestedSampler.leave_group_out`` return.  Keywords: groups (required), block, weights, columns, theta_ref, names."""
    unknown = set(kw) - set(_LGO_KEYS)
    if unknown:
        raise TypeError(f"leave_group_out got unexpected keyword(s) {sorted(unknown)}; valid: {list(_LGO_KEYS)}")
    if "groups" not in kw:
        raise TypeError("leave_group_out needs groups=")
    return leave_group_out(engine, chain, kw.pop("groups"), **kw)
