"""A long-double restatement of the fit report (include/cosmofit.h: cf_resid_device): the per-sample residual statistics as the
scripts' post-fit lines define them (sn/pantheon.py:157-164, sn/plotting.py:52, scipy.stats.skew / kurtosis), and the
sequential weighted per-datum accumulators.  No engine code involved; numpy only."""
import numpy as np

LD = np.longdouble
COLUMNS = ("mean", "std", "ss_res", "rmsd", "ss_tot", "r2", "skew", "kurtosis", "max_pull", "max_pull_index")
RELATIVE = ("std", "ss_res", "rmsd", "ss_tot", "r2", "max_pull")  # the project's 1e-10 bar, relative ...
ABSOLUTE = ("mean", "skew", "kurtosis")                           # ... and absolute for the columns that cross zero


def sample_stats(r, y, sigma=None):
    """The columns of one row from its residuals r [n] and its (corrected) data y [n]: dict of long doubles (max_pull and its
    index only with sigma).  Two passes; plain IEEE (n = 1 or m2 = 0 give NaN where numpy does)."""
    r, y = np.asarray(r, dtype=LD), np.asarray(y, dtype=LD)
    n = LD(r.size)
    with np.errstate(all="ignore"):
        mean = r.sum() / n
        d = r - mean
        m2, m3, m4 = (d**2).sum() / n, (d**3).sum() / n, (d**4).sum() / n
        ss_res, ss_tot = (r**2).sum(), ((y - y.sum() / n) ** 2).sum()
        out = dict(mean=mean, std=np.sqrt(m2), ss_res=ss_res, rmsd=np.sqrt(ss_res / n), ss_tot=ss_tot, r2=1 - ss_res / ss_tot,
                   skew=m3 / m2 ** LD(1.5), kurtosis=m4 / m2**2 - 3)
        if sigma is not None:
            pull = np.abs(r) / np.asarray(sigma, dtype=LD)
            k = int(np.argmax(pull))  # the first NaN, else the first maximum
            out.update(max_pull=pull[k], max_pull_index=LD(k))
    return out


def stats_matrix(rows, ys, sigma):
    """[S, len(COLUMNS)] long double of rows [S, n], ys [S, n]."""
    return np.array([[sample_stats(r, y, sigma)[c] for c in COLUMNS] for r, y in zip(rows, ys)], dtype=LD)


def new_state(n, n_thr):
    return dict(w_sum=np.zeros(n, LD), mean=np.zeros(n, LD), m2=np.zeros(n, LD), exceed=np.zeros((n_thr, n), LD),
                n_used=np.zeros(n, np.int64), n_skipped=np.zeros(n, np.int64))


def accumulate(state, rows, sigma, thresholds=(), w=None):
    """Continue the per-datum state over rows [m, n] in order: West's weighted update (Welford's for unit weights); a row whose
    weight is <= 0 or not finite, or whose residual for the datum is not finite, is skipped and counted for that datum."""
    rows = np.asarray(rows, dtype=LD)
    sigma = np.asarray(sigma, dtype=LD)
    for s in range(rows.shape[0]):
        wt = LD(1) if w is None else LD(w[s])
        r = rows[s]
        ok = np.isfinite(r) & bool(wt > 0 and np.isfinite(wt))
        state["n_skipped"] += ~ok
        state["n_used"] += ok
        with np.errstate(all="ignore"):
            w2 = state["w_sum"] + wt
            d = r - state["mean"]
            mean = state["mean"] + (wt * d) / w2
            m2 = state["m2"] + (wt * d) * (r - mean)
        state["w_sum"] = np.where(ok, w2, state["w_sum"])
        state["mean"] = np.where(ok, mean, state["mean"])
        state["m2"] = np.where(ok, m2, state["m2"])
        for k, t in enumerate(thresholds):
            with np.errstate(invalid="ignore"):
                state["exceed"][k] += np.where(ok & (np.abs(r) > LD(t) * sigma), wt, LD(0))
    return state


def finish(state, sigma):
    with np.errstate(all="ignore"):
        mean = np.where(state["w_sum"] > 0, state["mean"], np.nan)
        return dict(mean=mean, std=np.sqrt(state["m2"] / state["w_sum"]), pull_mean=mean / np.asarray(sigma, dtype=LD),
                    exceed=state["exceed"] / state["w_sum"][None, :], n_used=state["n_used"], n_skipped=state["n_skipped"])


def two_pass(rows, w=None):
    """(mean [n], std [n]) of the finite entries of every column by the defining sums, in long double."""
    rows = np.asarray(rows, dtype=LD)
    wt = np.ones(rows.shape[0], LD) if w is None else np.asarray(w, dtype=LD)
    use = np.isfinite(rows) & ((wt > 0) & np.isfinite(wt))[:, None]
    ww = np.where(use, wt[:, None], LD(0))
    x = np.where(use, rows, LD(0))
    with np.errstate(all="ignore"):
        tot = ww.sum(axis=0)
        mean = (ww * x).sum(axis=0) / tot
        var = (ww * np.where(use, x - mean[None, :], LD(0)) ** 2).sum(axis=0) / tot
    return mean, np.sqrt(var)


def errors(got, want, columns=COLUMNS):
    """{column: largest error} of got [S, ncol] against want [S, ncol]: relative for RELATIVE, absolute for ABSOLUTE columns,
    NaN positions must coincide (asserted), max_pull_index must be equal (error 0 / inf)."""
    got, want = np.asarray(got, dtype=LD), np.asarray(want, dtype=LD)
    out = {}
    for j, c in enumerate(columns):
        g, w = got[:, j], want[:, j]
        assert np.array_equal(np.isnan(g), np.isnan(w)), (c, "NaN positions differ")
        fin = ~np.isnan(w)
        if not fin.any():
            out[c] = 0.0
            continue
        with np.errstate(all="ignore"):
            if c == "max_pull_index":
                out[c] = 0.0 if np.array_equal(g[fin], w[fin]) else np.inf
            elif c in ABSOLUTE:
                out[c] = float(np.max(np.where(g[fin] == w[fin], 0, np.abs(g[fin] - w[fin]))))
            else:  # equal values (0, +-inf) are no error
                out[c] = float(np.max(np.where(g[fin] == w[fin], 0, np.abs(g[fin] - w[fin]) / np.abs(w[fin]))))
    return out
