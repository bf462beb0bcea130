"""The descriptor refusals cf_create makes from the descriptor alone (validate_desc: bounds, the two Gaussian-term index
ranges and their sigmas, the factor's pivots), as ``LikelihoodEngine`` keywords: one list for tests/test_abi_cpu.py (no device) and
tests/test_gpu_create_refusals.py (between two working engines).  The engine pre-checks none of them."""
import re

import numpy as np
import pytest

PIVOT = "CF_ERR_NOT_POSDEF: cf_create: the Cholesky factor has a non-positive or non-finite pivot"


def _sn2(pivot):
    """Two SNe whose 2 x 2 factor has `pivot` as its second diagonal entry."""
    return dict(z_cmb=np.array([0.1, 0.5]), z_hel=np.array([0.1, 0.5]), obs=np.array([19.0, 23.0]),
                chol=np.array([[0.2, 0.0], [0.01, pivot]]))


def cases(Param):
    """(name, extra LikelihoodEngine keywords, the whole CosmofitError text)."""
    return [
        ("bounds lo == hi", dict(bounds=[[60.0, 80.0], [0.3, 0.3]]), "CF_ERR_INVALID: cf_create: bounds must satisfy lo < hi"),
        ("gauss idx == ndim", dict(gauss=[(2, 0.0, 1.0)]), "CF_ERR_INVALID: cf_create: gauss idx"),
        ("chi2_gauss idx == ndim", dict(chi2_gauss=[(2, 0.0, 1.0)]), "CF_ERR_INVALID: cf_create: chi2_gauss idx"),
        ("gauss sigma == 0", dict(gauss=[(1, 0.3, 0.0)]), "CF_ERR_INVALID: cf_create: gauss sigma must be finite and non-zero"),
        ("gauss sigma inf", dict(gauss=[(0, 70.0, 1.0), (1, 0.3, np.inf)]), "CF_ERR_INVALID: cf_create: gauss sigma must be finite and non-zero"),
        ("chi2_gauss sigma == 0", dict(chi2_gauss=[(0, 70.0, 1.0), (1, 0.3, -0.0)]),
         "CF_ERR_INVALID: cf_create: chi2_gauss sigma must be finite and non-zero"),
        ("chi2_gauss sigma NaN", dict(chi2_gauss=[(1, 0.3, np.nan)]), "CF_ERR_INVALID: cf_create: chi2_gauss sigma must be finite and non-zero"),
        ("zero pivot", dict(sn=_sn2(0.0)), PIVOT),
        ("NaN pivot", dict(sn=_sn2(np.nan)), PIVOT),
    ]


def check(pkg):
    """Every case is refused with its own code and its full message."""
    for name, extra, text in cases(pkg.Param):
        with pytest.raises(pkg.CosmofitError, match="^" + re.escape(text) + "$") as err:
            pkg.LikelihoodEngine(ndim=2, z_max=1.0, n_grid=64, params=dict(H0=pkg.Param(0), Om=pkg.Param(1)), **extra)
        assert err.value.code == (-4 if text is PIVOT else -1), name
