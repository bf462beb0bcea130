"""The per-walker SN stage sweep of tests/test_gpu_walker_shapes.py under whatever CF_TUNE this process was started with (the string
is read once per process, so the tests start one process per string):
    python tests/walker_forms_worker.py <out.npz> stream | wg_default | wg_rows | generic
        under walker_shapes.FORMS' string of that name: asserts through walker_form, solve_form and the residual accessor's layout
        that the form asked for is the one a 33-walker batch takes, then saves per case "<case>:chi2", "<case>:logp", "<case>:rows"
        (the residual buffer as walker rows [33, n_ld], un-permuted where the layout is the fragment order) and "<case>:layout";
        "<case>:logl" for the growth case
    python tests/walker_forms_worker.py <out.npz> auto
        without any of the sweep's keys: the automatic switch of every model family at 4096 walkers; the 33 rows of
        walker_shapes.AUTO_CASES alone and scattered through a 4096-walker batch ("auto:<case>:rows33" / ":rows4096", chi2 alike);
        and batches of walker_shapes.W_BACK_TO_BACK walkers and of 176 again, back to back on one handle
        ("b2b:<k>:rows", ":chi2", ":layout")
Everything is float64 (int32 for a layout), compared as bits and against the references by the parent."""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
amd = importlib.import_module("cosmology-model-fit_amd")
import walker_shapes as S  # noqa: E402

OUT, MODE = sys.argv[1], sys.argv[2]
TUNE = os.environ.get("CF_TUNE", "")
results = {}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def evaluate(eng, theta, n_sn, want_layout):
    """chi^2 and log P of a batch, and the residual rows behind each (they must be the same bits: the stage does not depend on
    the output kind)."""
    W = theta.shape[0]
    chi2 = eng.chi_squared(theta)
    buf, layout = eng.last_residuals(W)
    assert layout == want_layout, f"layout {layout}, expected {want_layout} for {W} walkers under CF_TUNE={TUNE!r}"
    rows = S.rows_of_buffer(buf, layout, W, n_sn)
    logp = eng.log_probability(theta)
    buf2, layout2 = eng.last_residuals(W)
    assert layout2 == layout and np.array_equal(bits(buf2), bits(buf)), "the residual buffer differs between two evaluations"
    return chi2, logp, rows, layout


if MODE in S.FORMS:
    tune = [kv for kv in TUNE.split(",") if kv.startswith(S.OWN_KEYS)]
    assert ",".join(tune) == S.FORMS[MODE][0], f"CF_TUNE={TUNE!r} does not carry {S.FORMS[MODE][0]!r}"
    for name, case in S.CASES.items():
        with S.engine(amd, name) as eng:
            form, frag = S.expected_form(name, MODE)
            got = (eng.walker_form(S.N_ROWS), eng.solve_form(S.N_ROWS)["frag_order"])
            assert got == (form, frag), f"{name}: (walker_form, frag_order) = {got}, expected {(form, frag)} under CF_TUNE={TUNE!r}"
            th = np.array(S.rows(name))
            chi2, logp, rows, layout = evaluate(eng, th, case["n_sn"], frag)
            results[f"{name}:chi2"], results[f"{name}:logp"], results[f"{name}:rows"] = chi2, logp, rows
            results[f"{name}:layout"] = np.int32(layout)
            if case["growth"]:
                results[f"{name}:logl"] = eng.log_likelihood(th)
            with np.errstate(invalid="ignore"):
                print(f"{name}: walker_form {form}, layout {layout}, instantiation <{case['ez_model']}, {case['fde']}>")
elif MODE == "auto":
    assert not any(kv.startswith(S.OWN_KEYS) for kv in TUNE.split(",")), TUNE
    in_budget = {}
    for name, case in S.CASES.items():
        if case["group"] != "model":
            continue
        with S.engine(amd, name) as eng:
            in_budget[name] = eng.walker_form(S.W_AUTO)
            assert eng.walker_form(S.N_ROWS) == 0 and eng.walker_form(176) == 0, name
            if name in S.AUTO_CASES:
                assert in_budget[name] == 1, f"{name}: walker_form({S.W_AUTO}) = {in_budget[name]}"
                base, where = np.array(S.rows(name)), S.scatter(S.W_AUTO)
                big = base[np.arange(S.W_AUTO) % S.N_ROWS].copy()
                big[where] = base
                chi2, logp, rows, _ = evaluate(eng, big, case["n_sn"], 0)
                results[f"auto:{name}:chi2_4096"], results[f"auto:{name}:logp_4096"] = chi2[where], logp[where]
                results[f"auto:{name}:rows4096"] = rows[where]
                chi2, logp, rows, _ = evaluate(eng, base, case["n_sn"], 1)
                results[f"auto:{name}:chi2_33"], results[f"auto:{name}:logp_33"], results[f"auto:{name}:rows33"] = chi2, logp, rows
    results["auto:walker_form_4096"] = np.array([in_budget[n] for n in sorted(in_budget)], dtype=np.int32)
    print("walker_form(4096):", {n: in_budget[n] for n in sorted(in_budget)})
    # layouts back to back on ONE handle (one workspace): walker rows, the fragment order with two and with four workgroups per
    # walker, and walker rows again over what the fragment order left
    name = S.B2B_CASE
    base = np.array(S.rows(name))
    with S.engine(amd, name) as eng:
        for k, W in enumerate(S.W_BACK_TO_BACK + (S.W_BACK_TO_BACK[0],)):
            th = base[S.b2b_rows(W)]
            want = 1 if W <= 160 else 0
            assert eng.walker_form(W) == 0 and eng.solve_form(W)["frag_order"] == want, (W, eng.walker_form(W))
            chi2, _, rows, layout = evaluate(eng, th, S.CASES[name]["n_sn"], want)
            results[f"b2b:{k}:chi2"], results[f"b2b:{k}:rows"], results[f"b2b:{k}:layout"] = chi2, rows, np.int32(layout)
            print(f"back to back: {W} walkers, layout {layout}")
else:
    raise SystemExit(f"unknown mode {MODE!r}")
np.savez(OUT, **results)
