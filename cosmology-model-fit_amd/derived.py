"""
Derived parameters and posterior-predictive bands of a chain that lives on the device.

The first thing every post-fit block of the reference does with its samples is to add columns: omega_m, Omega_m, z*, r_d
(bao/desi_cmb.py:196-199), S8, q0, j0 (bao/desi_cmb_union3_fs8.py:282-287), z_drag (bao/desi_*_theta_star.py), the blobs of
cmb/cmb.py:45-63 and its ``addDerived`` columns (:118-138); the prediction plots evaluate H(z), D_M(z), the BAO ratios or
mu(z) on a 200-point grid (bao/plot_predictions.py:23).  Here both run where the chain is (csrc/cosmofit_derived.hip):

* ``Spec(engine, names, **consts)``: a validated list of quantities of one engine.
* ``columns(spec, samples)``: [n, n_q] on the device, asynchronous on the current stream.
* ``augment(spec, samples)``: [n, k + n_q], ready for ``marginals.corner_data`` and ``chain_stats.percentile``.
* ``curves(spec_or_engine, samples, z, quantity)``: [n, nz], one distance table per sample.
* ``bands(engine, samples, z, quantity, q, weights)``: the 16 / 50 / 84 % envelopes of those curves, reduced column by column
  with the device quantile of ``chain_stats`` (unweighted: ``np.percentile``'s bits) or ``marginals`` (weighted:
  ``corner.quantile``'s definition).

Names: the scalar quantities of ``_lib.DERIVED_CODES`` ("H0", "h", "Om", "omh2", "obh2", "och2", "w0", "wa", "q0", "j0",
"S8", "rd", "z_star", "r_drag", "z_drag", "z_eq", "rs_star", "DM_star", "theta_star100", "R", "lA") and at-z scalars
"<curve>@<z>" with a curve of ``_lib.CURVE_CODES`` ("H@0.51", "DV_rd@0.51", "mu@1.2", ...).

The inputs are float64 tensors on an MI355X; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from . import chain_stats, marginals
from ._args import ptr, sample_rows, single_device_engine, stream_of

MAX_COLUMNS = marginals.MAX_NDIM  # marginals.corner_data takes at most this many columns
_GL_NAMES = ("rs_star", "DM_star", "theta_star100", "R", "lA")
_RD_CURVES = ("DV_rd", "DM_rd", "DH_rd")

# the reductions of ``bands`` (module attributes so that a test can put host stand-ins behind the chunking logic)
_percentile = chain_stats.percentile
_weighted_quantile = marginals._weighted_quantile


def _missing(info: dict, name: str, consts: dict) -> Optional[str]:
    """What `name` needs of the engine and does not find (None: nothing): the rules of cf_derived_device / cf_curves_device."""
    slots, physical = info["slots"], info["ez_model"] == L.CF_EZ_PHYSICAL

    def need(*names):
        for s in names:
            if s not in slots:
                return {"H0": "an H0 slot", "Om": "an Om slot", "obh2": "an obh2 slot", "och2": "an och2 slot",
                        "s8": "a sigma8 slot", "rd": "an r_d slot or the r_drag fit"}[s]
        return None

    om = need("H0", "obh2", "och2") if physical else (need("Om") or (need("H0") if info["om_mode"] else None))
    wm_drag = need("obh2", "H0", "Om") if info["rd_wm_late"] else need("obh2", "och2")
    rd = wm_drag if info["rd_fit"] else need("rd")
    if name in ("H0", "h"):
        return need("H0")
    if name in ("Om", "q0", "j0"):
        return om
    if name == "omh2":
        return need("obh2", "och2") if physical else (need("H0") or om)
    if name in ("obh2", "och2"):
        return need(name)
    if name in ("w0", "wa"):
        return None
    if name == "S8":
        return need("s8") or om
    if name == "rd":
        return rd
    if name == "z_star":
        return need("obh2", "och2") if info["cmb"] else "a compressed-CMB block (z_star coefficients)"
    if name == "r_drag":
        return wm_drag if (info["rd_fit"] or consts.get("rdrag_fit") is not None) else "r_drag coefficients (rd_fit or rdrag_fit=)"
    if name == "z_drag":
        return wm_drag if consts.get("zdrag_fit") is not None else "z_drag coefficients (zdrag_fit= or comp=)"
    if name == "z_eq":
        return need("obh2", "och2") or (None if consts.get("zeq_or_h2") else "Omega_r h^2 (zeq_or_h2= or comp=)")
    if name in _GL_NAMES:
        return need("H0", "obh2", "och2") if info["cmb"] else "Gauss-Legendre nodes (a compressed-CMB block)"
    if name in L.CURVE_CODES:
        base = need("H0") or (need("obh2", "och2") if physical else om)
        return base or (rd if name in _RD_CURVES else None)
    return "to be a known quantity"


_QUASAR = "no derived quantities or prediction curves"


class Spec:
    """A list of derived quantities of one engine, validated at construction.

    consts: ``comp`` = a compression of ``cmb_data`` (its ``zdrag_fit``, ``rd_fit`` and ``zeq_or_h2`` are the defaults), or
    explicitly ``zdrag_fit`` (s1, s2, b, m, c1, e1, e2, c2, e3, e4), ``rdrag_fit`` (b, m, a1..a9: only read by "r_drag" on an
    engine whose BAO block does not use the fit) and ``zeq_or_h2`` (Omega_r h^2 of "z_eq")."""

    def __init__(self, engine, names: Sequence[str], *, comp: Optional[dict] = None, zdrag_fit=None, rdrag_fit=None,
                 zeq_or_h2: Optional[float] = None):
        info = single_device_engine(engine, "Spec", _QUASAR)
        if isinstance(names, str) or len(names) < 1:
            raise ValueError("Spec takes a non-empty sequence of names")
        if comp is not None:
            zdrag_fit = comp.get("zdrag_fit") if zdrag_fit is None else zdrag_fit
            rdrag_fit = comp.get("rd_fit") if rdrag_fit is None else rdrag_fit
            zeq_or_h2 = comp.get("zeq_or_h2") if zeq_or_h2 is None else zeq_or_h2
        consts = dict(zdrag_fit=zdrag_fit, rdrag_fit=rdrag_fit, zeq_or_h2=zeq_or_h2)
        if zdrag_fit is not None and len(zdrag_fit) != 10:
            raise ValueError("zdrag_fit takes 10 numbers: s1, s2, b, m, c1, e1, e2, c2, e3, e4")
        if rdrag_fit is not None and len(rdrag_fit) != 11:
            raise ValueError("rdrag_fit takes 11 numbers: b, m, a1..a9")
        if zeq_or_h2 is not None and not (np.isfinite(zeq_or_h2) and zeq_or_h2 > 0):
            raise ValueError("zeq_or_h2 must be a finite Omega_r h^2 > 0")
        self.engine, self.names, self.ndim = engine, tuple(str(n) for n in names), int(info["ndim"])
        self.n_q = len(self.names)
        # scalar-kernel entries (column, code, arg) and curve-kernel entries grouped by quantity: {code: [(column, z)]}
        self._scalar, self._at = [], {}
        for col, name in enumerate(self.names):
            base, at, z = name.partition("@")
            if at:
                try:
                    z = float(z)
                except ValueError:
                    raise ValueError(f"{name!r}: the redshift of an at-z quantity must be a number") from None
                if not np.isfinite(z):
                    raise ValueError(f"{name!r}: the redshift of an at-z quantity must be finite")
                if base not in L.CURVE_CODES:
                    raise ValueError(f"unknown quantity {name!r}: an at-z quantity is one of {sorted(L.CURVE_CODES)} + '@z'")
            elif name not in L.DERIVED_CODES or name == "H@":
                raise ValueError(f"unknown quantity {name!r}; valid: {sorted(n for n in L.DERIVED_CODES if n != 'H@')} and "
                                 f"'<curve>@<z>' with a curve of {sorted(L.CURVE_CODES)}")
            miss = _missing(info, base, consts)
            if miss:
                raise ValueError(f"{name} needs {miss}, which this engine lacks")
            if not at:
                self._scalar.append((col, L.DERIVED_CODES[name], float(zeq_or_h2) if name == "z_eq" else 0.0))
            elif base == "H":
                self._scalar.append((col, L.DERIVED_CODES["H@"], z))
            else:
                self._at.setdefault(L.CURVE_CODES[base], []).append((col, z))
        if len(self._scalar) > L.CF_DQ_MAX:
            raise ValueError(f"at most {L.CF_DQ_MAX} scalar quantities per Spec")
        c = L.cf_derived_consts()
        c.struct_size = C.sizeof(L.cf_derived_consts)
        if zdrag_fit is not None:
            c.zdrag_fit[:] = [float(x) for x in zdrag_fit]
        if rdrag_fit is not None:
            c.has_rdrag_fit = 1
            c.rdrag_fit[:] = [float(x) for x in rdrag_fit]
        c.zeq_or_h2 = float(zeq_or_h2) if zeq_or_h2 is not None else 0.0
        self._consts = c
        self._codes = np.array([code for _, code, _ in self._scalar], dtype=np.int32)
        self._args = np.array([arg for _, _, arg in self._scalar], dtype=np.float64)
        self._scalar_cols = [col for col, _, _ in self._scalar]

    def host_columns(self, theta: np.ndarray) -> np.ndarray:
        """The same columns for host rows [n, ndim] -> [n, n_q] numpy (cf_derived / cf_curves, synchronous)."""
        th = np.ascontiguousarray(theta, dtype=np.float64)
        if th.ndim != 2 or th.shape[1] != self.ndim:
            raise ValueError(f"theta must be [n, {self.ndim}]")
        n, lib, h = th.shape[0], L.lib(), self.engine._h
        out = np.empty((n, self.n_q))
        if self._scalar:
            tmp = np.empty((n, len(self._scalar)))
            L.check(lib.cf_derived(h, ptr(th), n, ptr(self._codes), ptr(self._args), len(self._scalar),
                                   C.cast(C.pointer(self._consts), C.c_void_p), ptr(tmp)))
            out[:, self._scalar_cols] = tmp
        for code, items in self._at.items():
            z = np.array([zz for _, zz in items], dtype=np.float64)
            tmp = np.empty((n, len(items)))
            L.check(lib.cf_curves(h, ptr(th), n, code, ptr(z), len(items), ptr(tmp)))
            out[:, [col for col, _ in items]] = tmp
        return out


def _launch_curves(engine, x: torch.Tensor, code: int, z: torch.Tensor, out: torch.Tensor, stream: int):
    L.check(L.lib().cf_curves_device(engine._h, x.data_ptr(), x.shape[0], code, z.data_ptr(), z.shape[0], out.data_ptr(), stream))


def columns(spec: Spec, samples: torch.Tensor) -> torch.Tensor:
    """The quantities of `spec` for every row of samples [n, ndim]: [n, n_q] float64 on the samples' device, in the order of
    ``spec.names``.  Asynchronous on torch's current stream; nothing is copied to the host."""
    x = sample_rows(samples, spec.ndim, "columns")
    n, dev = x.shape[0], x.device
    out = torch.empty((n, spec.n_q), dtype=torch.float64, device=dev)
    if n == 0:
        return out
    lib = L.lib()
    with torch.cuda.device(dev):
        stream = stream_of(dev)
        if spec._scalar:
            direct = not spec._at  # every column comes from the scalar kernel, in order
            tmp = out if direct else torch.empty((n, len(spec._scalar)), dtype=torch.float64, device=dev)
            L.check(lib.cf_derived_device(spec.engine._h, x.data_ptr(), n, ptr(spec._codes), ptr(spec._args),
                                          len(spec._scalar), C.cast(C.pointer(spec._consts), C.c_void_p), tmp.data_ptr(),
                                          stream))
            if not direct:
                out[:, spec._scalar_cols] = tmp
        for code, items in spec._at.items():
            z = torch.tensor([zz for _, zz in items], dtype=torch.float64).to(dev, non_blocking=False)
            tmp = torch.empty((n, len(items)), dtype=torch.float64, device=dev)
            _launch_curves(spec.engine, x, code, z, tmp, stream)
            out[:, [col for col, _ in items]] = tmp
    return out


def augment(spec: Spec, samples: torch.Tensor) -> torch.Tensor:
    """[n, k + n_q]: the sampled columns, then the derived ones -- what ``marginals.corner_data`` and
    ``chain_stats.percentile`` take.  Raises when the width would exceed the 16 columns ``marginals`` accepts."""
    if isinstance(samples, torch.Tensor) and samples.dim() == 2 and samples.shape[1] + spec.n_q > MAX_COLUMNS:
        raise ValueError(f"{samples.shape[1]} sampled + {spec.n_q} derived columns exceed the {MAX_COLUMNS} columns marginals takes; "
                         f"pass fewer names, or select columns of `columns(spec, samples)`")
    x = sample_rows(samples, spec.ndim, "augment")
    return torch.cat([x, columns(spec, x)], dim=1)


def _curve_code(quantity: str) -> int:
    if quantity not in L.CURVE_CODES:
        raise ValueError(f"unknown curve quantity {quantity!r}; valid: {sorted(L.CURVE_CODES)}")
    return L.CURVE_CODES[quantity]


def _z_array(z) -> np.ndarray:
    z = np.atleast_1d(np.asarray(z.detach().cpu().numpy() if isinstance(z, torch.Tensor) else z, dtype=np.float64))
    if z.ndim != 1 or z.size < 1:
        raise ValueError("z must be a non-empty 1-d sequence of redshifts")
    if not np.isfinite(z).all():
        raise ValueError("z must be finite")
    return np.ascontiguousarray(z)


def curves(spec_or_engine, samples: torch.Tensor, z, quantity: str) -> torch.Tensor:
    """`quantity` ("H", "DM", "DV_rd", "DM_rd", "DH_rd", "F_AP", "mu") at the redshifts z [nz] for every row of samples:
    [n, nz] float64 on the samples' device.  Each sample builds its own distance table once (the engine's n_grid nodes) and
    serves all redshifts from it; any order of z, beyond the grid by linear extrapolation as the scripts' ``DM_z``."""
    engine = spec_or_engine.engine if isinstance(spec_or_engine, Spec) else spec_or_engine
    info = single_device_engine(engine, "curves", _QUASAR)
    code = _curve_code(quantity)
    miss = _missing(info, quantity, {})
    if miss:
        raise ValueError(f"{quantity} needs {miss}, which this engine lacks")
    zs = _z_array(z)
    x = sample_rows(samples, info["ndim"], "curves")
    n, dev = x.shape[0], x.device
    out = torch.empty((n, zs.size), dtype=torch.float64, device=dev)
    if n == 0:
        return out
    with torch.cuda.device(dev):
        stream = stream_of(dev)
        zd = torch.from_numpy(zs).to(dev)
        if zs.size <= L.CF_CURVE_MAX_NZ:
            _launch_curves(engine, x, code, zd, out, stream)
        else:  # more redshifts than one launch takes: pieces of CF_CURVE_MAX_NZ columns
            for k0 in range(0, zs.size, L.CF_CURVE_MAX_NZ):
                piece = torch.empty((n, min(L.CF_CURVE_MAX_NZ, zs.size - k0)), dtype=torch.float64, device=dev)
                _launch_curves(engine, x, code, zd[k0:k0 + piece.shape[1]].contiguous(), piece, stream)
                out[:, k0:k0 + piece.shape[1]] = piece
    return out


_BAND_BUFFERS = 4  # per redshift column of a chunk: the curve values, their sorted copy, the sort's indices, one temporary


def band_chunk(n: int, nz: int, max_bytes: int) -> int:
    """Redshifts per chunk of ``bands``: the most whose workspace (``_BAND_BUFFERS`` arrays of n doubles per redshift) stays
    under max_bytes, at least 1, at most what one launch takes."""
    if max_bytes < 1:
        raise ValueError("max_bytes must be >= 1")
    return int(max(1, min(nz, L.CF_CURVE_MAX_NZ, max_bytes // (_BAND_BUFFERS * 8 * max(n, 1)))))


def reduce_columns(block: torch.Tensor, qs: np.ndarray, w: Optional[torch.Tensor] = None, own_buffers: bool = False):
    """(quantiles [len(qs), m], mean [m], std [m]) as numpy, of the columns of block [n, m], every column on its own: the
    reduction of ``bands`` (and of ``quintessence.bands``).  own_buffers: every column is summed from an allocation of its
    own.  torch's sum reads an unaligned head of its input apart, so the bits of a column's mean can depend on where the
    column starts: in the transposed copy that is a multiple of n doubles, which for odd n depends on the column's place in the
    chunk; in a buffer of its own it does not."""
    n, m = block.shape
    w_tot = None if w is None else w.sum()
    if w is None:
        out_b = _percentile(block, list(100.0 * qs)).cpu().numpy()
    else:
        out_b = _weighted_quantile(block, w, qs)
    # mean and std column by column on contiguous copies: the order of each sum depends on n alone, not on the chunk's width
    cols = block.t().contiguous()
    means, stds = [], []
    for j in range(m):
        c = cols[j].clone() if own_buffers else cols[j]
        mu = c.sum() / n if w is None else (w * c).sum() / w_tot
        var = ((c - mu) ** 2).sum() / n if w is None else (w * (c - mu) ** 2).sum() / w_tot
        means.append(mu)
        stds.append(torch.sqrt(var))
    return out_b, torch.stack(means).cpu().numpy(), torch.stack(stds).cpu().numpy()


def bands(engine, samples: torch.Tensor, z, quantity: str, q=(0.159, 0.5, 0.841), weights: Optional[torch.Tensor] = None,
          max_bytes: int = 2**31) -> dict:
    """Posterior-predictive band of `quantity` over z: dict(z [nz], q [len(q)], bands [len(q), nz], mean [nz], std [nz]) as
    numpy arrays.  The curves are evaluated in chunks of redshifts whose workspace stays under max_bytes (``band_chunk``) and
    every column is reduced on its own, so the result does not depend on the chunking: without weights
    ``np.percentile(curve[:, j], 100 q)`` (its bits, ``chain_stats.percentile``), mean and std (ddof 0); with weights
    ``corner.quantile(curve[:, j], q, weights)`` (``marginals``' definition) and the weighted mean and std."""
    if isinstance(engine, Spec):
        engine = engine.engine
    zs = _z_array(z)
    qs = np.atleast_1d(np.asarray(q, dtype=np.float64))
    if qs.ndim != 1 or qs.size < 1 or np.isnan(qs).any() or (qs < 0).any() or (qs > 1).any():
        raise ValueError("q must be quantile levels in [0, 1]")
    if not isinstance(samples, torch.Tensor) or samples.dim() != 2 or samples.shape[0] < 1:
        raise ValueError("bands takes samples [n, ndim] with n >= 1")
    n = samples.shape[0]
    w = None
    if weights is not None:
        w = marginals._weights(weights, n, "bands")[0]
    step = band_chunk(n, zs.size, int(max_bytes))
    out_b, out_m, out_s = np.empty((qs.size, zs.size)), np.empty(zs.size), np.empty(zs.size)
    for k0 in range(0, zs.size, step):
        block = curves(engine, samples, zs[k0:k0 + step], quantity)  # [n, m]
        m = block.shape[1]
        out_b[:, k0:k0 + m], out_m[k0:k0 + m], out_s[k0:k0 + m] = reduce_columns(block, qs, w)
        del block
    return dict(z=zs, q=qs, bands=out_b, mean=out_m, std=out_s)
