"""The solve sweep of tests/test_gpu_solve_shapes.py under whatever CF_TUNE this process was started with (the string is read
once per process, so the tests start one process per string):
    python tests/solve_forms_worker.py <out.npz>                 chi^2, log P and the solve form of every (N <= 449, W in W_WORKER)
    python tests/solve_forms_worker.py <out.npz> forms           the solve forms of those alone: cf_solve_form needs no GPU
    python tests/solve_forms_worker.py <out.npz> forms-default   the solve forms of the whole table x its in-process batch sizes
Keys of <out.npz>: "<N>:<W>:chi2", "<N>:<W>:logp" (float64 [W], compared as bits by the parent) and "<N>:<W>:form" (int32: the ten
values of cf_solve_form, then frag_order of the handle, -1 in the `forms` modes)."""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
amd = importlib.import_module("cosmology-model-fit_amd")
import solve_shapes as S  # noqa: E402

OUT = sys.argv[1]
MODE = sys.argv[2] if len(sys.argv) > 2 else "eval"
fields = amd.engine.SOLVE_FORM_FIELDS
assert fields == S.FORM_FIELDS
results = {}
if MODE in ("forms", "forms-default"):
    for n in (S.N_SMALL if MODE == "forms" else [s[0] for s in S.SIZES]):
        for W in (S.W_WORKER if MODE == "forms" else S.w_list(n)):
            f = amd.engine.solve_form(n, W)
            results[f"{n}:{W}:form"] = np.array([f[k] for k in fields] + [-1], dtype=np.int32)
else:
    for n in S.N_SMALL:
        base = S.base_rows(n)
        with S.engine(amd, n) as eng:
            assert eng.info()["solve_mode"] == amd.engine.solve_mode_of("inverse")
            for W in S.W_WORKER:
                theta = base[S.batch_rows(W, base.shape[0])]
                f = eng.solve_form(W)
                results[f"{n}:{W}:form"] = np.array([f[k] for k in fields] + [f["frag_order"]], dtype=np.int32)
                results[f"{n}:{W}:chi2"] = eng.chi_squared(theta)
                results[f"{n}:{W}:logp"] = eng.log_probability(theta)
np.savez(OUT, **results)
