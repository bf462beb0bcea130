"""CPU: the long-double restatement of the derived quantities against the fixture the reference computed, ``derived.Spec``'s
validation, emcee's blob slicing of the ensemble, and the chunking of ``derived.bands`` -- everything of ``derived`` that needs
no device."""
import importlib
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import chain_gloo_worker as cw
import derived_reference as R
import derived_shapes as DS
from conftest import golden, load_pkg

amd = load_pkg()
D = importlib.import_module("cosmology-model-fit_amd.derived")

REL, ABS0 = 1e-10, 1e-12  # the project's parity bar; q0 and j0 cross zero: an absolute bar instead


def _engine(case, **over):
    kw = DS.engine_kwargs(amd, case)
    kw.update(over)
    return SimpleNamespace(model_info=amd.engine.model_info(**kw))


@pytest.mark.parametrize("case", DS.CASES)
def test_restatement_reproduces_the_fixture(case):
    names, want = DS.COLUMNS[case], DS.expected(case)
    got = R.scalars(DS.model(amd, case), DS.thetas(case), names)
    assert got.shape == want.shape and want.shape[0] >= 300
    for j, name in enumerate(names):
        err = np.abs(got[:, j] - want[:, j])
        if name in DS.ZERO_CROSSING:
            assert float(err.max()) <= ABS0, (case, name, float(err.max()))
        else:
            rel = float((err / np.abs(want[:, j])).max())
            assert rel <= REL, (case, name, rel)


@pytest.mark.parametrize("case", ["desi_cmb_thawing", "desi_cmb_lcdm"])
@pytest.mark.parametrize("quantity", ["H", "DM", "DV_rd", "DM_rd", "DH_rd"])
def test_restatement_curves_reproduce_the_fixture(case, quantity):
    g = golden("derived")
    z, want = g[case + "/curve_z"], g[case + "/" + quantity]
    got = R.curves(DS.model(amd, case), DS.thetas(case)[: want.shape[0]], z, quantity).astype(np.float64)
    assert np.allclose(got, want, rtol=REL, atol=0.0), float(np.nanmax(np.abs(got / want - 1)))


def test_restatement_mu_and_fap_follow_from_the_distances():
    """mu and F_AP have no column in the fixture: they are the scripts' expressions of the two checked distances."""
    m, th = DS.model(amd, "desi_cmb_thawing"), DS.thetas("desi_cmb_thawing")[:2]
    z = np.array([0.3, 1.1, 2.0])
    dm, dh_rd, dm_rd = (R.curves(m, th, z, q) for q in ("DM", "DH_rd", "DM_rd"))
    assert np.allclose((R.curves(m, th, z, "mu")).astype(float), (25 + 5 * np.log10((1 + z) * dm)).astype(float), rtol=1e-15)
    assert np.allclose(R.curves(m, th, z, "F_AP").astype(float), (dm_rd / dh_rd).astype(float), rtol=1e-15)


# ---- Spec ---------------------------------------------------------------------------------------------------------------------
def test_spec_accepts_every_applicable_name_and_keeps_the_order():
    for case in DS.CASES:
        names = DS.applicable_scalars(amd, case) + ["DM@0.51", "mu@1.0"]
        spec = D.Spec(_engine(case), names, **DS.consts(amd, case))
        assert spec.names == tuple(names) and spec.n_q == len(names)
        assert sorted(spec._scalar_cols + [c for items in spec._at.values() for c, _ in items]) == list(range(len(names)))
    assert set(DS.COLUMNS["cmb_cmb"]) <= set(DS.applicable_scalars(amd, "cmb_cmb"))


def test_spec_refuses_an_unknown_name():
    eng = _engine("desi_cmb_thawing")
    for bad in ("omega_m", "H@", "H@x", "H@nan", "sigma8@0.5", ""):
        with pytest.raises(ValueError, match="unknown quantity|must be a number|must be finite"):
            D.Spec(eng, ["H0", bad])
    with pytest.raises(ValueError, match="non-empty"):
        D.Spec(eng, [])


@pytest.mark.parametrize("case,name,what", [
    ("desi_cmb_thawing", "S8", "sigma8"),                      # no sigma8 slot
    ("desi_union3_bbn", "rs_star", "Gauss-Legendre"),          # no compressed-CMB block, hence no nodes
    ("desi_union3_bbn", "z_star", "compressed-CMB"),
    ("desi_union3_bbn", "och2", "och2"),                       # a late-time flat engine without that slot
    ("cmb_cmb", "rd", "r_d slot"),                             # no BAO block: neither the slot nor the fit
    ("cmb_cmb", "DV_rd@0.5", "r_d slot"),
])
def test_spec_names_the_quantity_whose_slot_or_block_is_missing(case, name, what):
    with pytest.raises(ValueError, match=f"^{name.split('@')[0]}.* needs .*{what}"):
        D.Spec(_engine(case), ["H0", name], **DS.consts(amd, case))


def test_spec_needs_its_constants():
    eng = _engine("cmb_cmb")
    for name in ("z_drag", "r_drag", "z_eq"):
        with pytest.raises(ValueError, match=f"^{name} needs"):
            D.Spec(eng, [name])
        D.Spec(eng, [name], comp=amd.cmb_data.PLANCK_ACT)
    with pytest.raises(ValueError, match="10 numbers"):
        D.Spec(eng, ["z_drag"], zdrag_fit=(1.0, 2.0))
    late = SimpleNamespace(model_info=amd.engine.model_info(ndim=3, params=dict(H0=amd.Param(0, scale=100.0), Om=amd.Param(1), w0=amd.Param(2)),
                                                            fde=amd.CF_FDE_THAWING))
    with pytest.raises(ValueError, match="^obh2 needs an obh2 slot"):
        D.Spec(late, ["obh2"])
    assert D.Spec(late, ["Om", "wa", "q0", "j0", "omh2", "h"]).n_q == 6


def test_augment_refuses_more_columns_than_marginals_takes():
    spec = D.Spec(_engine("desi_cmb_union3_fs8"), ["H0", "h", "Om", "omh2", "obh2", "och2", "w0", "wa", "q0", "j0", "S8"])
    with pytest.raises(ValueError, match="exceed the 16 columns"):
        D.augment(spec, torch.zeros((5, 6), dtype=torch.float64))  # 6 + 11 = 17
    with pytest.raises(ValueError, match="MI355X"):                # 6 + 10 fits: the next check is the device
        D.augment(D.Spec(_engine("desi_cmb_union3_fs8"), spec.names[:10]), torch.zeros((5, 6), dtype=torch.float64))


def test_device_entry_points_refuse_cpu_tensors_and_wrong_shapes():
    spec = D.Spec(_engine("cmb_cmb"), ["Om"])
    x = torch.zeros((4, 3), dtype=torch.float64)
    for call in (lambda: D.columns(spec, x), lambda: D.curves(spec, x, [0.1], "H")):
        with pytest.raises(ValueError, match="MI355X"):
            call()
    with pytest.raises(ValueError, match=r"samples \[n, 3\]"):
        D.columns(spec, torch.zeros((4, 5), dtype=torch.float64))
    with pytest.raises(ValueError, match="float64"):
        D.columns(spec, x.float())
    with pytest.raises(ValueError, match="unknown curve"):
        D.curves(spec, x, [0.1], "w")
    with pytest.raises(ValueError, match="finite"):
        D.curves(spec, x, [0.1, np.inf], "H")
    with pytest.raises(ValueError, match="^DV_rd needs"):
        D.curves(spec, x, [0.1], "DV_rd")


# ---- get_blobs ----------------------------------------------------------------------------------------------------------------
def _fake_columns(spec, samples):
    """A blob that is a function of the stored position: (sum, product of the first two)."""
    return torch.stack([samples.sum(dim=1), samples[:, 0] * samples[:, 1]], dim=1)


def test_get_blobs_needs_a_spec_and_a_run(monkeypatch):
    monkeypatch.setattr(D, "columns", _fake_columns)
    ens = cw.make_ensemble(24, (("stretch", 1.0),))
    ens.run_mcmc(2)
    with pytest.raises(AttributeError, match="blobs="):
        ens.get_blobs()
    ens = _ensemble_with_blobs(24)
    with pytest.raises(AttributeError, match="run_mcmc"):
        ens.get_blobs()


def _ensemble_with_blobs(W):
    from oracle import moves_torch

    g = torch.Generator().manual_seed(7)
    start = cw.MU + cw.SIG * torch.randn(W, 3, generator=g, dtype=torch.float64)
    return amd.ensemble.ShardedEnsemble(cw.gauss_logp, start, seed=11, moves=(("stretch", 1.0),), blobs=object(),
                                        moves_impl=moves_torch.TensorMoves(amd.ensemble.stream_key))


@pytest.mark.parametrize("discard,thin", [(0, 1), (3, 2), (1, 3), (0, 20), (19, 1)])
def test_get_blobs_slices_and_shapes_as_emcee(monkeypatch, discard, thin):
    """emcee's rule: stored[discard + thin - 1 : iteration : thin], [n, W, n_q]; flat = step-major, walker-minor."""
    monkeypatch.setattr(D, "columns", _fake_columns)
    W, steps = 12, 20
    ens = _ensemble_with_blobs(W)
    ens.run_mcmc(steps)
    full = ens.get_chain()
    want = torch.stack([full.sum(dim=2), full[..., 0] * full[..., 1]], dim=2)[discard + thin - 1: steps: thin]
    got = ens.get_blobs(discard=discard, thin=thin)
    assert got.shape == (len(range(discard + thin - 1, steps, thin)), W, 2) and torch.equal(got, want)
    flat = ens.get_blobs(discard=discard, thin=thin, flat=True)
    assert flat.shape == (got.shape[0] * W, 2) and torch.equal(flat, want.reshape(-1, 2))
    assert torch.equal(flat, _fake_columns(None, ens.get_chain(discard=discard, thin=thin, flat=True)))


# ---- bands --------------------------------------------------------------------------------------------------------------------
def _host_percentile(samples, q):
    return torch.from_numpy(np.percentile(samples.numpy(), q, axis=0))


def _host_weighted_quantile(x, w, q):
    """corner.quantile per column (marginals._weighted_quantile's definition) on host tensors."""
    out = np.empty((len(q), x.shape[1]))
    for c in range(x.shape[1]):
        idx = np.argsort(x[:, c].numpy(), kind="stable")
        sw = w.numpy()[idx]
        cdf = np.cumsum(sw)[:-1]
        cdf /= cdf[-1]
        out[:, c] = np.interp(q, np.append(0, cdf), x[:, c].numpy()[idx])
    return out


def _fake_curves(engine, samples, z, quantity):
    z = torch.as_tensor(np.asarray(z, dtype=np.float64))
    return samples[:, :1] * torch.sqrt(samples[:, 1:2] * (1 + z[None, :]) ** 3 + 1 - samples[:, 1:2])


@pytest.mark.parametrize("weighted", [False, True])
def test_bands_do_not_depend_on_the_chunking(monkeypatch, weighted):
    monkeypatch.setattr(D, "curves", _fake_curves)
    monkeypatch.setattr(D, "_percentile", _host_percentile)
    monkeypatch.setattr(D, "_weighted_quantile", _host_weighted_quantile)
    rng = np.random.default_rng(3)
    n, nz = 1000, 37
    x = torch.from_numpy(np.stack([rng.uniform(60, 80, n), rng.uniform(0.2, 0.4, n)], axis=1))
    w = torch.from_numpy(rng.uniform(0.0, 1.0, n)) if weighted else None
    z = np.linspace(0, 2.5, nz)
    whole = D.bands(None, x, z, "H", weights=w)
    assert whole["bands"].shape == (3, nz) and whole["mean"].shape == whole["std"].shape == (nz,)
    per_col = D._BAND_BUFFERS * 8 * n
    for max_bytes, chunk in ((per_col, 1), (5 * per_col + 7, 5), (36 * per_col, 36), (2**31, nz)):
        assert D.band_chunk(n, nz, max_bytes) == chunk
        part = D.bands(None, x, z, "H", weights=w, max_bytes=max_bytes)
        for key in ("z", "q", "bands", "mean", "std"):
            assert np.array_equal(part[key], whole[key]), (key, chunk)
    # and the unchunked band is numpy's percentile of each column / corner's weighted quantile
    curve = _fake_curves(None, x, z, "H")
    want = np.percentile(curve.numpy(), [15.9, 50, 84.1], axis=0) if not weighted else \
        _host_weighted_quantile(curve, w, np.array([0.159, 0.5, 0.841]))
    assert np.array_equal(whole["bands"], want)


def test_band_chunk_never_exceeds_one_launch():
    assert D.band_chunk(10, 10000, 2**40) == amd._lib.CF_CURVE_MAX_NZ
    assert D.band_chunk(10**9, 200, 2**31) == 1
    with pytest.raises(ValueError):
        D.band_chunk(10, 10, 0)
