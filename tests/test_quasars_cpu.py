"""CPU: the quasar Hubble-diagram likelihoods (quasars.py, include/cosmofit.h: cf_create_quasar) without a GPU.

* The numpy restatement (tests/quasar_reference.py) reproduces every fixture of tests/golden/generate_quasars.py -- the
  reference's own log_posterior, log_likelihood, per-block chi^2 and theory vectors -- at rtol 1e-12, -inf rows exactly,
  with the recipe of quasars.RECIPES translated into the restatement's terms.
* At the docstring medians the reference's chi^2 match the printed "Flat wzCDM" numbers within 0.02 (real-data scripts).
* The ctypes mirror of cf_qsr_ext has gcc's layout, and cf_desc keeps its size.
"""
import os
import subprocess

import numpy as np
import pytest

import quasar_reference as ref
from conftest import ROOT, golden, synthetic_cov


def _recipe(pkg, name):
    r = pkg.quasars.RECIPES[ref.SCRIPTS[name]]
    return dict(theta=r.theta, nkp=r.nkp, bounds=r.bounds, sn_grid=r.sn_grid, sn_zhel=r.sn_zhel), r


def _run(pkg, name):
    g = dict(golden(name))
    rec, r = _recipe(pkg, name)
    qsr, sn, bao = ref.fixture_data(g, synthetic_cov)
    assert (sn is not None) == r.sn and (bao is not None) == r.bao
    b = None if bao is None else (bao[0]["z"], bao[0]["value"], bao[0]["quantity"], bao[1])
    return g, ref.evaluate(rec, g["thetas"], qsr, sn, b)


def _close(a, b, rtol):
    a, b = np.asarray(a), np.asarray(b)
    fin = np.isfinite(b)
    assert np.array_equal(np.isfinite(a), fin) or not fin.all()
    np.testing.assert_allclose(a[fin], b[fin], rtol=rtol, atol=0)


@pytest.mark.parametrize("name", ref.CASES)
def test_restatement_reproduces_the_reference(pkg, name):
    g, out = _run(pkg, name)
    fin = np.isfinite(g["logp"])
    assert np.array_equal(out["logp"] == -np.inf, ~fin), "the -inf rows are the out-of-box rows"
    np.testing.assert_allclose(out["logp"][fin], g["logp"][fin], rtol=1e-12, atol=0)
    _close(out["logl"], g["logl"], 1e-12)
    _close(out["chi2_parts"], g["chi2_parts"], 1e-12)
    rows = g["theory_rows"]
    np.testing.assert_allclose(out["mu_qsr"][rows], g["mu_qsr"], rtol=1e-12, atol=0)
    if "mu_sn" in g:
        np.testing.assert_allclose(out["mu_sn"][rows], g["mu_sn"], rtol=1e-12, atol=0)
    if "bao_theory" in g:
        np.testing.assert_allclose(out["bao_theory"][rows], g["bao_theory"], rtol=1e-12, atol=0)


@pytest.mark.parametrize("name", ["qsr_union3", "qsr_desi"])
def test_docstring_medians_give_the_printed_chi2(name):
    g = golden(name)
    sn, qsr, bao = g["chi2_parts"][-1]
    assert abs(qsr - g["printed_qsr"]) < 0.02
    if name == "qsr_union3":
        assert abs(sn - g["printed_sn"]) < 0.02
    else:
        assert abs(bao - g["printed_bao"]) < 0.02


@pytest.mark.parametrize("name", ref.CASES)
def test_recipe_box_is_the_scripts(pkg, name):
    g = golden(name)
    np.testing.assert_array_equal(np.asarray(pkg.quasars.RECIPES[ref.SCRIPTS[name]].bounds, float), g["bounds"])


def test_unbinned_catalogue_has_repeated_redshifts_and_reaches_the_grid_top():
    g = golden("qsr_union3_unbinned")
    z = g["qsr_z"]
    assert z.size > 2000 and np.unique(z).size < z.size
    assert np.max(z) == np.linspace(0, np.max(z), ref.N_GRID)[-1]


def test_scripts_build_delegates_quasar_names(pkg):
    with pytest.raises(KeyError, match="quasar recipe"):
        pkg.scripts.build("quasars/qsr_nope.py", qsr=([1.0], [40.0], [0.1]))
    assert set(pkg.quasars.RECIPES).isdisjoint(pkg.scripts.RECIPES)


def test_qsr_ext_layout_matches_c(pkg, tmp_path):
    import ctypes as C

    L = pkg._lib
    fields = [f for f, _ in L.cf_qsr_ext._fields_]
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "cosmofit.h"\nint main(){printf("%zu %zu", sizeof(cf_qsr_ext), '
            'sizeof(cf_desc));' + "".join(f'printf(" %zu", offsetof(cf_qsr_ext, {f}));' for f in fields) + "return 0;}")
    src = tmp_path / "q.c"
    src.write_text(prog)
    exe = tmp_path / "q"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    vals = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert vals[0] == C.sizeof(L.cf_qsr_ext)
    assert vals[1] == 1152 == C.sizeof(L.cf_desc)
    for f, off in zip(fields, vals[2:]):
        assert getattr(L.cf_qsr_ext, f).offset == off, f


def test_quasar_entry_points_are_exported(pkg):
    lib = pkg.lib()
    for name in ("cf_create_quasar", "cf_qsr_eval_parts"):
        assert hasattr(lib, name)
