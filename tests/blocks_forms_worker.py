"""The small-blocks sweep of tests/test_gpu_blocks_shapes.py under whatever CF_TUNE this process was started with (the string is
read once per process, so the tests start one process per string):
    python tests/blocks_forms_worker.py <out.npz> forced    under one of blocks_shapes.FORMS' strings: asserts that the form asked
                                                             for is the one a 33-walker batch takes, then every case's outputs
                                                             for its 33 rows ("<case>:<output>") and for blocks_shapes.bad_rows
                                                             ("<case>:bad:<output>")
    python tests/blocks_forms_worker.py <out.npz> auto      without CF_TUNE: asserts 64 x 2 for 33 walkers and 16 x 1 for 2049, and
                                                             that the 33 rows have the same bits alone and inside a 2049-row batch
                                                             (SWITCH_CASES; saved as "<case>:<output>" and "<case>:big:<output>")
    python tests/blocks_forms_worker.py <out.npz> generic   under walker_generic=1: asserts the generic per-walker kernel, then the
                                                             grid-edge cases' outputs
    python tests/blocks_forms_worker.py <out.npz> typo      under mistyped keys: asserts the default forms, one case's outputs
Outputs: blocks_shapes.OUTPUTS, float64, compared as bits and against the reference by the parent."""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
amd = importlib.import_module("cosmology-model-fit_amd")
import blocks_shapes as S  # noqa: E402

OUT, MODE = sys.argv[1], sys.argv[2]
TUNE = os.environ.get("CF_TUNE", "")
results = {}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def save(prefix, got):
    for key, v in got.items():
        results[f"{prefix}:{key}"] = v


if MODE == "forced":
    want = {tune: form for form, tune in S.FORMS.items()}[TUNE]
    for name in S.CASES:
        with S.engine(amd, name) as eng:
            for W in (1, S.N_ROWS, S.W_LARGE):
                assert eng.small_blocks_form(W) == want, f"{name}: small_blocks_form({W}) = {eng.small_blocks_form(W)} under CF_TUNE={TUNE!r}"
            assert eng.walker_form(S.N_ROWS) == 0, eng.walker_form(S.N_ROWS)
            save(name, S.evaluate(eng, S.rows(name)))
            save(name + ":bad", S.evaluate(eng, S.bad_rows(name)))
elif MODE == "auto":
    assert TUNE == "", TUNE
    for name in S.SWITCH_CASES:
        with S.engine(amd, name) as eng:
            assert eng.small_blocks_form(S.N_ROWS) == (64, 2) and eng.small_blocks_form(2048) == (64, 2), eng.small_blocks_form(S.N_ROWS)
            assert eng.small_blocks_form(S.W_LARGE) == (16, 1), eng.small_blocks_form(S.W_LARGE)
            base = S.rows(name)
            # the 33 rows spread over the large batch: at its start, across workgroup boundaries, and at its ragged end
            where = np.concatenate([np.arange(11), 1000 + 17 * np.arange(11), S.W_LARGE - 11 + np.arange(11)])
            big = base[np.arange(S.W_LARGE) % S.N_ROWS].copy()
            big[where] = base
            small, large = S.evaluate(eng, base), S.evaluate(eng, big)
            for key in small:
                bad = np.flatnonzero(np.any((bits(small[key]) != bits(large[key][where])).reshape(S.N_ROWS, -1), axis=1))
                assert bad.size == 0, f"{name}: {key} of rows {bad} differs between 64 x 2 (33 walkers) and 16 x 1 (inside {S.W_LARGE})"
            save(name, small)
            save(name + ":big", {k: v[where] for k, v in large.items()})
elif MODE == "generic":
    for name in S.EDGE_CASES:
        with S.engine(amd, name) as eng:
            assert eng.walker_form(S.N_ROWS) == 2, f"{name}: walker_form = {eng.walker_form(S.N_ROWS)} under CF_TUNE={TUNE!r}"
            save(name, S.evaluate(eng, S.rows(name)))
elif MODE == "typo":  # mistyped keys are silently ignored: the defaults must be reported (and run)
    assert "sb_wide_max=" not in TUNE and "sb_roles_max=" not in TUNE and TUNE, TUNE
    name = S.SWITCH_CASES[1]
    with S.engine(amd, name) as eng:
        forms = [eng.small_blocks_form(W) for W in (1, S.N_ROWS, 2048, S.W_LARGE)]
        assert forms == [(64, 2), (64, 2), (64, 2), (16, 1)], f"{forms} under CF_TUNE={TUNE!r}"
        save(name, S.evaluate(eng, S.rows(name)))
else:
    raise SystemExit(f"unknown mode {MODE!r}")
np.savez(OUT, **results)
