"""
The streaming form of the per-walker kernel (walker_stream_kernel: one wave per walker, the distance table in segments of 512
nodes) gives the bits of the workgroup form (walker_fast_kernel).  tests/walker_stream_worker.py evaluates every case in a fresh
process under CF_TUNE walker_stream=0 and =1 (CF_TUNE is read once per process) and asserts through cf_walker_form that the
form asked for is the one that ran; a third process under the automatic switch evaluates the same 32 rows inside a batch of 176
(workgroup form) and of 4096 (streaming form).  Equality is of the bit patterns: NaN positions and -inf included.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "walker_stream_worker.py")

CASES = (["pm1_n70_g4000"] + [f"pm1_n200_g{g}" for g in (4000, 1000, 4096, 520)] + [f"boundary_g{g}" for g in (4000, 4096, 520)] +
         ["weights_n200", "lin_n200", "pm1_n1701_g4000"])


def _worker(mode, out):
    tune = [kv for kv in os.environ.get("CF_TUNE", "").split(",") if kv and not kv.startswith("walker_stream=")]
    if mode != "auto":
        tune.append(f"walker_stream={mode}")
    env = dict(os.environ, CF_TUNE=",".join(tune))
    r = subprocess.run([sys.executable, WORKER, mode, out], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return dict(np.load(out))


@pytest.fixture(scope="module")
def forms(tmp_path_factory):
    d = tmp_path_factory.mktemp("walker_stream")
    return {m: _worker(m, str(d / f"form_{m}.npz")) for m in ("0", "1")}


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_streaming_form_gives_the_workgroup_forms_bits(forms, case):
    for kind in ("chi2", "logp"):
        a, b = forms["0"][f"{case}:{kind}"], forms["1"][f"{case}:{kind}"]
        diff = np.flatnonzero(a.view(np.uint64) != b.view(np.uint64))
        print(f"{case}:{kind}: {a.size} walkers, {diff.size} differ, {np.isnan(a).sum()} NaN, {np.isneginf(a).sum()} -inf")
        assert _same_bits(a, b), f"{case}:{kind}: rows {diff[:10]} differ: {a[diff[:4]]} vs {b[diff[:4]]}"
    # the special rows did what they are there for: the NaN-velocity walker's chi^2 is NaN, the out-of-box rows are -inf
    assert np.isnan(forms["0"][f"{case}:chi2"]).any() or case == "lin_n200"
    assert np.isneginf(forms["0"][f"{case}:logp"]).any()


@pytest.mark.gpu
def test_streaming_form_joint_likelihood_with_bao_nodes(forms):
    a, b = forms["0"]["joint_cpl:logl"], forms["1"]["joint_cpl:logl"]
    print(f"joint_cpl:logl: {a.size} walkers, {(a.view(np.uint64) != b.view(np.uint64)).sum()} differ, finite {np.isfinite(a).sum()}")
    assert np.isfinite(a).sum() > a.size // 2
    assert _same_bits(a, b)


@pytest.mark.gpu
def test_batch_invariance_across_the_automatic_switch(tmp_path):
    r = _worker("auto", str(tmp_path / "auto.npz"))
    for kind in ("chi2", "logp"):
        a, b = r[f"invariance_176:{kind}"], r[f"invariance_4096:{kind}"]
        print(f"invariance:{kind}: {(a.view(np.uint64) != b.view(np.uint64)).sum()} of {a.size} differ")
        assert a.size == 32 and _same_bits(a, b)
        # 5201 walkers, streaming form: the rows in the first round and at the end of the partly filled last one
        for part in ("head", "tail"):
            c = r[f"invariance_split_{part}:{kind}"]
            print(f"invariance split {part}:{kind}: {(a.view(np.uint64) != c.view(np.uint64)).sum()} of {c.size} differ")
            assert _same_bits(a, c)
