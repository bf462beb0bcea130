"""
The scalar field behind a dark-energy fit, for every sample of a chain that lives on the device.

``field.py`` of the reference reconstructs, for one parameter triple typed in from a fit, the quintessence field of a thawing
model: phi(a), the potential V(phi), the kinetic and potential terms, cosmic time t(a), a(t), phi(t) and the age of the
universe.  Here the same runs for every row of a posterior (csrc/cosmofit_field.hip: one workgroup per sample, the sample's
{phi, t} table in LDS) and is reduced to bands as ``derived.bands`` does for the distance curves:

* ``Model(fde, columns, scale, fixed, ...)``: which columns of the samples are H0, Om, w0 (and wa), and the a grid.
* ``Model.from_recipe(name)``: the same from ``scripts.RECIPES``.
* ``reconstruct(model, samples, a=, phi=, t=)``: a dict of float64 tensors on the samples' device.
* ``bands(model, samples, quantity, x, q, weights)``: quantile envelopes, mean and std over the samples.

The three dark-energy forms with a canonical field: "thawing" (the reference's), "wcdm" and "cpl".  1 + w is formed directly
(the script forms 1 + (-1 + x)), so below a ~ 0.01 these values are the more accurate ones: the script's own phi differs from
an extended-precision evaluation by up to 1.6e-6 relative at its first nodes (4e-15 of the row's largest phi).

Row status: 0 ok; 1 phantom (1 + w < 0 at a node; the phi-dependent outputs are NaN); 2 invalid (non-finite parameter,
H0 <= 0, E^2 <= 0 at a node; everything is NaN).  The inputs are float64 tensors on an MI355X; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib as L
from . import derived, marginals
from ._args import ptr, sample_rows, stream_of

FDE = {"wcdm": L.CF_FDE_WCDM, "thawing": L.CF_FDE_THAWING, "cpl": L.CF_FDE_CPL}
MAX_NQ = L.CF_FIELD_MAX_NQ
# bands: quantity -> (the query set it is evaluated at, the output of the kernel)
QUANTITIES = {"phi_a": "a", "t_a": "a", "w_a": "a", "K_a": "a", "V_a": "a", "V_phi": "phi", "a_phi": "phi", "a_t": "t",
              "phi_t": "t", "t_today": None, "phi_today": None}
_SETS = {"a": ("phi_a", "t_a", "w_a", "K_a", "V_a"), "phi": ("phi_grid", "a_phi", "V_phi"), "t": ("t_grid", "a_t", "phi_t")}


class Model:
    """Where the parameters of the field are in a row of samples, and the a grid of the reconstruction.

    ``columns``: name -> column of the samples; ``scale``: name -> factor (a sampled h: {"H0": 100}); ``fixed``: name -> a
    constant instead of a column.  Names: "H0", "Om", "w0", and "wa" exactly when fde = "cpl".  ``ndim`` is the width of the
    samples (default: the largest column + 1)."""

    def __init__(self, fde: str = "thawing", columns: Optional[dict] = None, scale: Optional[dict] = None,
                 fixed: Optional[dict] = None, orh2: float = 4.1835e-05, n_a: int = 5000, a_min: float = 1e-8, a_max: float = 5.0,
                 ndim: Optional[int] = None):
        columns, scale, fixed = dict(columns or {}), dict(scale or {}), dict(fixed or {})
        if fde == "lcdm":
            raise ValueError("LambdaCDM has no scalar field to reconstruct (fde is one of 'thawing', 'wcdm', 'cpl')")
        if fde not in FDE:
            raise ValueError(f"unknown fde {fde!r}; valid: {sorted(FDE)}")
        names = L.FIELD_PARS if fde == "cpl" else L.FIELD_PARS[:3]
        for n in list(columns) + list(scale) + list(fixed):
            if n not in L.FIELD_PARS:
                raise ValueError(f"unknown parameter {n!r}; valid: {list(L.FIELD_PARS)}")
        if fde != "cpl" and ("wa" in columns or "wa" in fixed):
            raise ValueError("wa is a parameter of fde='cpl' only")
        for n in names:
            if (n in columns) == (n in fixed):
                raise ValueError(f"{n} must be given once: a column or a fixed value")
        for n in scale:
            if n not in columns:
                raise ValueError(f"scale[{n!r}] has no column to scale")
        for n, i in columns.items():
            if isinstance(i, bool) or not isinstance(i, (int, np.integer)) or i < 0:
                raise ValueError(f"column of {n} must be an index >= 0")
        for n, v in list(scale.items()) + list(fixed.items()):
            if not np.isfinite(v):
                raise ValueError(f"value of {n} must be finite")
        if isinstance(n_a, bool) or not isinstance(n_a, (int, np.integer)) or not 16 <= n_a <= 8192:
            raise ValueError("n_a must be an integer in 16..8192")
        if not (np.isfinite(a_min) and np.isfinite(a_max) and 0 < a_min < 1 < a_max):
            raise ValueError("the grid needs finite 0 < a_min < 1 < a_max")
        if not (np.isfinite(orh2) and orh2 >= 0):
            raise ValueError("orh2 must be finite and >= 0")
        width = max(columns.values(), default=-1) + 1
        self.ndim = int(ndim) if ndim is not None else max(width, 1)
        if self.ndim < max(width, 1) or self.ndim > L.CF_FIELD_MAX_NDIM:
            raise ValueError(f"ndim must cover the columns and be at most {L.CF_FIELD_MAX_NDIM}")
        self.fde, self.columns, self.scale, self.fixed = fde, columns, scale, fixed
        self.orh2, self.n_a, self.a_min, self.a_max = float(orh2), int(n_a), float(a_min), float(a_max)
        d = L.cf_field_desc()
        d.struct_size, d.fde, d.n_a, d.ndim, d.n_par = C.sizeof(L.cf_field_desc), FDE[fde], self.n_a, self.ndim, len(names)
        d.a_min, d.a_max, d.orh2 = self.a_min, self.a_max, self.orh2
        for s, n in enumerate(L.FIELD_PARS):
            d.par[s].idx, d.par[s].scale, d.par[s].fixed = -1, 1.0, 0.0
            if n in columns:
                d.par[s].idx, d.par[s].scale = int(columns[n]), float(scale.get(n, 1.0))
            elif n in fixed:
                d.par[s].fixed = float(fixed[n])
        self._desc = d

    @classmethod
    def from_recipe(cls, recipe, **grid) -> "Model":
        """The slot map of a reference script: a ``scripts.Recipe`` or its name in ``scripts.RECIPES``.  Raises for a recipe
        whose E(z) this reconstruction cannot express (physical densities, an omega_m slot) or that has no field (LambdaCDM)."""
        from . import scripts

        if isinstance(recipe, str):
            if recipe not in scripts.RECIPES:
                raise KeyError(f"no recipe for {recipe!r}; known: {sorted(scripts.RECIPES)}")
            name, recipe = recipe, scripts.RECIPES[recipe]
        else:
            name = "the recipe"
        if recipe.physical:
            raise ValueError(f"{name}: E(z) from physical densities (omega_b, omega_c, neutrinos) is not the field reconstruction's")
        if recipe.omh2:
            raise ValueError(f"{name}: its Om slot holds Omega_m h^2, which the field reconstruction does not take")
        if recipe.fde == "lcdm":
            raise ValueError(f"{name}: LambdaCDM has no scalar field to reconstruct")
        names = L.FIELD_PARS if recipe.fde == "cpl" else L.FIELD_PARS[:3]
        theta = list(recipe.theta)
        columns = {n: theta.index(n) for n in names if n in theta}
        fixed = {n: recipe.fixed[n] for n in names if n in recipe.fixed and n not in columns}
        scale = {n: recipe.scale[n] for n in columns if n in recipe.scale}
        return cls(fde=recipe.fde, columns=columns, scale=scale, fixed=fixed, ndim=len(theta), **grid)


def _queries(x, what: str, own_ok: bool):
    """None, an int (the rows' own grids) or a 1-d float64 numpy array."""
    if x is None:
        return None
    if own_ok and isinstance(x, (int, np.integer)) and not isinstance(x, bool):
        if not 1 <= x <= MAX_NQ:
            raise ValueError(f"{what}: an own grid has 1..{MAX_NQ} points")
        return int(x)
    x = np.atleast_1d(np.asarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x, dtype=np.float64))
    if x.ndim != 1 or x.size < 1:
        raise ValueError(f"{what} must be a non-empty 1-d sequence" + (" or a number of points" if own_ok else ""))
    return np.ascontiguousarray(x)


def pieces(n: int):
    """(start, stop) of the launches that serve n given query points: at most ``MAX_NQ`` each."""
    return [(k0, min(n, k0 + MAX_NQ)) for k0 in range(0, max(n, 1), MAX_NQ)]


def _call(model: Model, theta_ptr, n: int, qa, qphi, qt, alloc, upload, ptr, stream, want):
    """One or more launches; `alloc(shape, dtype)`, `upload(np array)` and `ptr(buffer)` make it the same for device tensors
    and host arrays.  Returns the dict of buffers."""
    lib, out = L.lib(), {}
    sets = {"a": qa, "phi": qphi, "t": qt}
    n_of = {k: (0 if v is None else (v if isinstance(v, int) else v.size)) for k, v in sets.items()}
    for k, names in _SETS.items():
        for name in names:
            if n_of[k] and (want is None or name in want) and not (name.endswith("_grid") and not isinstance(sets[k], int)):
                out[name] = alloc((n, n_of[k]), np.float64)
    if want is None or "scalars" in want:
        out["scalars"] = alloc((n, L.CF_FIELD_NSCALAR), np.float64)
    if want is None or "status" in want:
        out["status"] = alloc((n,), np.int32)
    if n == 0:
        return out
    n_pieces = max(len(pieces(n_of[k])) for k in sets)
    for i in range(n_pieces):
        q, o, keep, copies = L.cf_field_queries(), L.cf_field_out(), [], []
        for k, names in _SETS.items():
            v = sets[k]
            if v is None:
                continue
            if isinstance(v, int):
                lo, hi = (0, v) if i == 0 else (0, 0)
            else:
                lo, hi = pieces(v.size)[i] if i < len(pieces(v.size)) else (0, 0)
            if hi <= lo or not any(name in out for name in names):
                continue
            setattr(q, {"a": "n_aq", "phi": "n_phi", "t": "n_t"}[k], hi - lo)
            if not isinstance(v, int):
                buf = upload(v[lo:hi])
                keep.append(buf)
                setattr(q, {"a": "a_q", "phi": "phi_q", "t": "t_q"}[k], ptr(buf))
            for name in names:
                if name not in out:
                    continue
                if lo == 0 and hi == n_of[k]:
                    setattr(o, name, ptr(out[name]))
                else:  # a piece of the columns: a contiguous buffer of its own, copied into place
                    piece = alloc((n, hi - lo), np.float64)
                    copies.append((name, lo, hi, piece))
                    setattr(o, name, ptr(piece))
        if i == 0:
            if "scalars" in out:
                o.scalars = ptr(out["scalars"])
            if "status" in out:
                o.status = ptr(out["status"])
        if stream is None:
            L.check(lib.cf_field(C.byref(model._desc), theta_ptr, n, C.byref(q), C.byref(o)))
        else:
            L.check(lib.cf_field_device(C.byref(model._desc), theta_ptr, n, C.byref(q), C.byref(o), stream))
        for name, lo, hi, piece in copies:
            out[name][:, lo:hi] = piece
    return out


def _unpack(out: dict, qa, qphi, qt, wrap) -> dict:
    res = {k: v for k, v in out.items() if k != "scalars"}
    if "scalars" in out:
        for j, name in enumerate(L.FIELD_SCALARS):
            res[name] = out["scalars"][:, j]
    if qa is not None:
        res["a"] = wrap(qa)
    if qphi is not None and not isinstance(qphi, int):
        res["phi_grid"] = wrap(qphi)
    if qt is not None and not isinstance(qt, int):
        res["t_grid"] = wrap(qt)
    return res


def _rows(model: Model, samples, what: str) -> torch.Tensor:
    if not isinstance(model, Model):
        raise ValueError(f"{what} takes a quintessence.Model")
    return sample_rows(samples, model.ndim, what)


def reconstruct(model: Model, samples: torch.Tensor, a=None, phi=None, t=None, _want=None) -> dict:
    """The field of every row of samples [n, ndim], as float64 tensors on the samples' device (status: int32):

    * always: ``status`` [n], ``phi_today``, ``t_today`` [Gyr], ``hubble_time`` [Gyr], ``phi_max``, ``t_max`` [Gyr], each [n];
    * ``a`` = scale factors [n_a]: ``phi_a``, ``t_a`` [Gyr], ``w_a``, ``K_a``, ``V_a``, each [n, n_a] (``np.interp``'s rule on the
      a grid for phi and t, the closed forms for w, K, V);
    * ``phi`` = field values [n_phi], or an int for every row's own ``linspace(phi[0], phi[-1], phi)`` (the reference: 2000):
      ``a_phi``, ``V_phi`` [n, n_phi] by ``interp1d``'s rule with linear extrapolation, and ``phi_grid`` ([n_phi], or
      [n, n_phi] for own grids);
    * ``t`` = times in Gyr [n_t], or an int for every row's own ``linspace(t[10], min(1.5 t_today, 0.95 t[-1]), t)`` (the
      reference: 1000): ``a_t`` (``interp1d``), ``phi_t`` (``np.interp``) and ``t_grid``.

    More than 4096 given points run in pieces.  Asynchronous on torch's current stream; nothing is copied to the host."""
    qa, qphi, qt = _queries(a, "a", False), _queries(phi, "phi", True), _queries(t, "t", True)
    x = _rows(model, samples, "reconstruct")
    dev = x.device
    tdt = {np.float64: torch.float64, np.int32: torch.int32}
    with torch.cuda.device(dev):
        out = _call(model, x.data_ptr(), x.shape[0], qa, qphi, qt,
                    alloc=lambda shape, dt: torch.empty(shape, dtype=tdt[dt], device=dev),
                    upload=lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev),
                    ptr=lambda b: b.data_ptr(), stream=stream_of(dev), want=_want)
    return _unpack(out, qa, qphi, qt, lambda v: torch.from_numpy(v).to(dev))


def reconstruct_host(model: Model, theta, a=None, phi=None, t=None) -> dict:
    """``reconstruct`` for host rows [n, ndim] -> numpy arrays (cf_field: synchronous, through temporary device buffers)."""
    qa, qphi, qt = _queries(a, "a", False), _queries(phi, "phi", True), _queries(t, "t", True)
    if not isinstance(model, Model):
        raise ValueError("reconstruct_host takes a quintessence.Model")
    th = np.ascontiguousarray(theta, dtype=np.float64)
    if th.ndim != 2 or th.shape[1] != model.ndim:
        raise ValueError(f"theta must be [n, {model.ndim}]")
    out = _call(model, ptr(th), th.shape[0], qa, qphi, qt, alloc=lambda shape, dt: np.empty(shape, dtype=dt),
                upload=lambda v: np.ascontiguousarray(v), ptr=ptr, stream=None, want=None)
    return _unpack(out, qa, qphi, qt, lambda v: v)


def bands(model: Model, samples: torch.Tensor, quantity: str, x=None, q=(0.159, 0.5, 0.841),
          weights: Optional[torch.Tensor] = None, max_bytes: int = 2**31) -> dict:
    """The band of `quantity` over the samples: dict(x [nx], q [len(q)], bands [len(q), nx], mean [nx], std [nx], n_used,
    n_phantom, n_invalid), numpy arrays and ints.

    `quantity`: "phi_a", "t_a", "w_a", "K_a", "V_a" at scale factors x; "V_phi", "a_phi" at field values x; "a_t", "phi_t" at
    times x [Gyr]; the scalars "t_today" and "phi_today" (x is not taken) as one-column bands.  Rows whose status is not 0
    are left out of the reduction (with their weights) and counted.  The columns are evaluated in chunks whose workspace
    stays under max_bytes (``derived.band_chunk``) and reduced one by one by ``derived.reduce_columns``, so the result does
    not depend on the chunking: ``np.percentile``'s bits without weights, ``corner.quantile``'s definition with them."""
    if quantity not in QUANTITIES:
        raise ValueError(f"unknown quantity {quantity!r}; valid: {sorted(QUANTITIES)}")
    kind = QUANTITIES[quantity]
    if kind is None:
        if x is not None:
            raise ValueError(f"{quantity} is a scalar of the row: it takes no x")
        xs = np.empty(0)
    else:
        if x is None:
            raise ValueError(f"{quantity} needs the points x it is evaluated at")
        xs = _queries(x, "x", False)
        if not np.isfinite(xs).all():
            raise ValueError("x must be finite")
    qs = np.atleast_1d(np.asarray(q, dtype=np.float64))
    if qs.ndim != 1 or qs.size < 1 or np.isnan(qs).any() or (qs < 0).any() or (qs > 1).any():
        raise ValueError("q must be quantile levels in [0, 1]")
    if not isinstance(samples, torch.Tensor) or samples.dim() != 2 or samples.shape[0] < 1:
        raise ValueError("bands takes samples [n, ndim] with n >= 1")
    if int(max_bytes) < 1:
        raise ValueError("max_bytes must be >= 1")
    if not isinstance(model, Model):
        raise ValueError("bands takes a quintessence.Model")
    n = samples.shape[0]
    w = None
    if weights is not None:
        w = marginals._weights(weights, n, "bands")[0]
    rows = _rows(model, samples, "bands")
    if w is not None and w.device != rows.device:
        raise ValueError("weights must be on the device of the samples")
    first = reconstruct(model, rows, _want=("status", "scalars"))
    status = first["status"]
    n_phantom, n_invalid = int((status == L.CF_FIELD_PHANTOM).sum()), int((status == L.CF_FIELD_BAD).sum())
    good = status == L.CF_FIELD_OK
    n_used = n - n_phantom - n_invalid
    if n_used < 1:
        raise ValueError("no row of the samples has a field (status 0)")
    if n_used < n:
        rows = rows[good].contiguous()
        w = None if w is None else w[good].contiguous()
        if w is not None and not float(w.max()) > 0:
            raise ValueError("at least one weight of the rows that have a field must be > 0")
    counts = dict(n_used=n_used, n_phantom=n_phantom, n_invalid=n_invalid)
    if kind is None:
        col = first[quantity][good].contiguous()[:, None]
        b, m, s = derived.reduce_columns(col, qs, w, own_buffers=True)
        return dict(x=xs, q=qs, bands=b, mean=m, std=s, **counts)
    step = derived.band_chunk(n_used, xs.size, int(max_bytes))
    out_b, out_m, out_s = np.empty((qs.size, xs.size)), np.empty(xs.size), np.empty(xs.size)
    for k0 in range(0, xs.size, step):
        block = reconstruct(model, rows, **{kind: xs[k0:k0 + step]}, _want=(quantity,))[quantity]
        m = block.shape[1]
        out_b[:, k0:k0 + m], out_m[k0:k0 + m], out_s[k0:k0 + m] = derived.reduce_columns(block, qs, w, own_buffers=True)
        del block
    return dict(x=xs, q=qs, bands=out_b, mean=out_m, std=out_s, **counts)
