"""Long-double restatement of the prior / output epilogue for the epilogue sweep (tests/epilogue_shapes.py,
tests/test_epilogue_cpu.py, tests/test_gpu_epilogue.py), written from the text of the Python reference -- sn/pantheon.py:80-97 as
oracle/oracle_np.py restates it in chi_squared / log_likelihood / log_prior / log_probability -- not from the kernel's.

A case (tests/epilogue_shapes.py) is read through these keys only: ndim, bounds ([ndim, 2] or None), prior_normalised, gauss and
chi2_gauss (sequences of (idx, mean, sigma)), cpl_wall, slots (name -> (idx, scale) or ("fixed", value); w0 defaults to -1, wa to 0,
fcc and fs8err to 1), logl_const, n_fs8, n_cc, cc_logdet, cc_f_inverse.

``finalize(case, theta_row, chi2, kind)`` takes the sum of the likelihood blocks WITHOUT the chi^2 Gaussian terms and gives what the
sampler sees, with whether the row is counted as non-finite.  Two places where the product defines more than the reference does
(DESIGN.md): a non-finite chi^2 is -inf and counted (the reference returns NaN and emcee aborts), and the CPL wall is looked at
before chi^2 is, so a row on the wall is lp - 1e8 whatever its chi^2.

Order of decisions: (1) chi^2 Gaussian terms; (2) CHI2 returns, NaN passed through, never counted; (3) LOGP with bounds: strict box,
-inf outside (NaN in any coordinate is outside), not counted; log_norm inside; (4) Gaussian priors; (5) wall; (6) non-finite chi^2:
-inf, counted once; (7) -0.5 chi^2 + logl_const + n_fs8 ln f_err - 0.5 (n_cc ln 2 pi + logdet +- 2 n_cc ln f_cc)."""
import numpy as np

LD = np.longdouble
CHI2, LOGL, LOGP = "chi2", "logl", "logp"
KINDS = (CHI2, LOGL, LOGP)
EPS = LD(2.0) ** -52
_DEFAULT = dict(w0=-1.0, wa=0.0, fcc=1.0, fs8err=1.0)
LN_2PI = np.log(LD(2) * LD("3.14159265358979323846264338327950288"))


def slot(case, name, row):
    """The slots' idx / scale / fixed rule: theta[idx] * scale for a free slot, the constant otherwise."""
    a, b = case["slots"].get(name, ("fixed", _DEFAULT[name]))
    return LD(b) if a == "fixed" else LD(row[a]) * LD(b)


def in_box(case, row):
    """lo < t < hi in every coordinate; a NaN coordinate fails both comparisons."""
    b = case["bounds"]
    return bool(np.all((b[:, 0] < row) & (row < b[:, 1])))


def on_wall(case, row):
    return bool(case["cpl_wall"]) and bool(slot(case, "w0", row) + slot(case, "wa", row) >= 0)


def walk(case, row, chi2, kind):
    """dict(value, counted, reason, terms, logs): reason is one of "chi2", "outside", "wall", "nonfinite", "value"; terms are the
    long-double addends of the value in the order the reference adds them; logs are (n, ln f) of the logarithms of theta taken."""
    row = np.asarray(row, dtype=np.float64)
    terms, logs = [LD(chi2)], []
    for idx, mean, sigma in case["chi2_gauss"]:                      # oracle_np.chi_squared: (theta[idx] - mean) ** 2 / sigma ** 2
        terms.append((LD(row[idx]) - LD(mean)) ** 2 / LD(sigma) ** 2)
    total = sum(terms[1:], terms[0])
    if kind == CHI2:
        return dict(value=total, counted=False, reason="chi2", terms=terms, logs=logs)
    chi_terms, terms, lp = terms, [], LD(0)
    if kind == LOGP:                                                 # oracle_np.log_prior
        if case["bounds"] is not None:
            if not in_box(case, row):
                return dict(value=LD(-np.inf), counted=False, reason="outside", terms=[], logs=[])
            if case["prior_normalised"]:
                terms += [-np.log(LD(hi) - LD(lo)) for lo, hi in case["bounds"]]
        for idx, mean, sigma in case["gauss"]:
            terms.append(-LD(0.5) * (LD(row[idx]) - LD(mean)) ** 2 / LD(sigma) ** 2)
        lp = sum(terms, LD(0))
    if on_wall(case, row):                                           # oracle_np.log_likelihood: before chi^2 is looked at
        terms.append(LD(-1e8))
        return dict(value=lp + LD(-1e8), counted=False, reason="wall", terms=terms, logs=logs)
    if not np.isfinite(total):
        return dict(value=LD(-np.inf), counted=True, reason="nonfinite", terms=[], logs=[])
    terms += [-LD(0.5) * t for t in chi_terms] + [LD(case["logl_const"])]
    with np.errstate(all="ignore"):
        if case["n_fs8"]:
            ln_f = np.log(slot(case, "fs8err", row))
            terms.append(case["n_fs8"] * ln_f)
            logs.append((case["n_fs8"], ln_f))
        if case["n_cc"]:
            n, ln_f = case["n_cc"], np.log(slot(case, "fcc", row))
            terms += [-LD(0.5) * n * LN_2PI, -LD(0.5) * LD(case["cc_logdet"]), -LD(0.5) * (2 if case["cc_f_inverse"] else -2) * n * ln_f]
            logs.append((n, ln_f))
    return dict(value=sum(terms, LD(0)), counted=False, reason="value", terms=terms, logs=logs)


def finalize(case, theta_row, chi2, kind):
    """(value, counted) in np.longdouble / bool."""
    w = walk(case, theta_row, chi2, kind)
    return w["value"], w["counted"]


def bound(w):
    """What float64 may lose adding the T terms of walk()'s result, whatever the order and with each term formed by at most four
    rounded operations: 2^-52 (T + 4) sum |term|, plus n 2 2^-52 max(1, |ln f|) per logarithm (two ulp of a library log, n times)."""
    if not w["terms"]:
        return LD(0)
    b = EPS * (len(w["terms"]) + 4) * sum((abs(t) for t in w["terms"]), LD(0))
    for n, ln_f in w["logs"]:
        b += n * 2 * EPS * max(LD(1), abs(ln_f))
    return b
