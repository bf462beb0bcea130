"""
The progress-keyed wave priority of the streaming per-walker kernel (walker_stream_kernel takes s_setprio 3 .. 0 at the top of
each grid segment, from a table cf_create works out of the SNe per segment: csrc/cf_stream_pack.h) changes no bit.
tests/walker_level_worker.py evaluates every case in a fresh process (CF_TUNE is read once per process) in three modes: the
streaming form with CF_TUNE walker_level=0 (every wave at priority 0) and =1 (the table), and the workgroup form; the streaming
form is forced (walker_stream=1, with small_frag=0,sn_parts=1 so that batches of 1 and 5 walkers take it).  Each worker asserts
through cf_walker_form and cf_walker_levels that the form and the table in effect are the ones its mode stands for -- all zeros
under walker_level=0, the table worked out in Python from the data otherwise.  Equality is of the bit patterns: NaN positions
and -inf included.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "walker_level_worker.py")
OWN_KEYS = ("walker_stream=", "walker_level=", "small_frag=", "sn_parts=")
TUNE = {"level0": "walker_stream=1,small_frag=0,sn_parts=1,walker_level=0", "level1": "walker_stream=1,small_frag=0,sn_parts=1,walker_level=1",
        "wg": "walker_stream=0,small_frag=0,sn_parts=1"}

GRID_CASES = [f"g{g}_{w}" for g in (520, 1000, 4000, 4096) for w in ("w1", "w1slow", "w5", "w4096")]
EDGE_CASES = [f"edge_n{n}" for n in (1, 63, 64, 65, 127, 128, 129, 191, 192, 193)] + ["empty_middle"]


@pytest.fixture(scope="module")
def modes(tmp_path_factory):
    d = tmp_path_factory.mktemp("walker_level")
    out = {}
    for mode, tune in TUNE.items():
        keep = [kv for kv in os.environ.get("CF_TUNE", "").split(",") if kv and not kv.startswith(OWN_KEYS)]
        env = dict(os.environ, CF_TUNE=",".join(keep + [tune]))
        path = str(d / f"{mode}.npz")
        r = subprocess.run([sys.executable, WORKER, mode, path], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        out[mode] = dict(np.load(path))
    return out


def _assert_same_bits(modes, key):
    a = modes["level0"][key]
    for other in ("level1", "wg"):
        b = modes[other][key]
        diff = np.flatnonzero(a.view(np.uint64) != b.view(np.uint64)) if a.shape == b.shape else None
        print(f"{key}: level0 vs {other}: {a.size} walkers, {'shape' if diff is None else diff.size} differ, {np.isnan(a).sum()} NaN, "
              f"{np.isneginf(a).sum()} -inf")
        assert diff is not None and diff.size == 0, f"{key}: level0 vs {other}: rows {diff[:10]} differ: {a[diff[:4]]} vs {b[diff[:4]]}"


@pytest.mark.gpu
@pytest.mark.parametrize("case", GRID_CASES)
def test_levelling_changes_no_bit(modes, case):
    for kind in ("chi2", "logp"):
        _assert_same_bits(modes, f"{case}:{kind}")
    chi2, logp = modes["level0"][f"{case}:chi2"], modes["level0"][f"{case}:logp"]
    if chi2.size >= 5:  # the special rows did what they are there for (walker_level_worker.thetas)
        assert np.isnan(chi2[1]) and np.isneginf(logp[2]) and np.isfinite(chi2[2]) and np.isfinite(chi2[3]) and np.isneginf(logp[3])
        assert np.isfinite(logp[[0, 4]]).all()
    # the knob took: zeros under walker_level=0; with several segments the table starts at 3 and never rises
    lv0, lv1 = modes["level0"][f"{case}:levels"], modes["level1"][f"{case}:levels"]
    assert not lv0.any() and lv1[0] == 3 and (np.diff(lv1) <= 0).all() and lv1.min() >= 0, (lv0, lv1)


@pytest.mark.gpu
@pytest.mark.parametrize("case", EDGE_CASES)
def test_segment_populations_at_trip_edges(modes, case):
    for kind in ("chi2", "logp"):
        _assert_same_bits(modes, f"{case}:{kind}")
    chi2, logp = modes["level0"][f"{case}:chi2"], modes["level0"][f"{case}:logp"]
    assert np.isnan(chi2[1]) and np.isneginf(logp[2]) and np.isfinite(chi2[3]) and np.isfinite(logp[[0, 4]]).all()
    lv0, lv1 = modes["level0"][f"{case}:levels"], modes["level1"][f"{case}:levels"]
    assert not lv0.any() and lv1[0] == 3 and (np.diff(lv1) <= 0).all(), (lv0, lv1)


@pytest.mark.gpu
def test_empty_middle_segments_against_the_c_oracle(modes, pkg):
    """log-probability of the in-box rows of the empty-middle case within 1e-10 (relative) of the C oracle."""
    from oracle import oracle_c, oracle_np as onp

    m = modes["level1"]
    theta, rows = m["empty_middle:theta"], [0, 4]
    ref = oracle_c.COracle(onp.Likelihood(
        ndim=4, z_max=2.36, n_grid=4000, offset=onp.Slot(0), H0=onp.Slot(1), Om=onp.Slot(2), v=onp.Slot(3),
        z_cmb=m["empty_middle:z_cmb"], z_hel=m["empty_middle:z_hel"], obs=m["empty_middle:obs"], chol=m["empty_middle:chol"],
        bounds=pkg.sn_pantheon.bounds, gauss=[pkg.sn_pantheon.H0_PRIOR])).logp(theta[rows])
    got = m["empty_middle:logp"][rows]
    err = np.max(np.abs(got - ref) / np.abs(ref))
    print(f"empty_middle: logp {got} against the C oracle {ref}: relative error {err:.3e}")
    assert err < 1e-10


@pytest.mark.gpu
def test_joint_likelihood_under_both_knob_values(modes):
    a = modes["level0"]["joint_cpl:logl"]
    print(f"joint_cpl:logl: {a.size} walkers, finite {np.isfinite(a).sum()}, levels {modes['level1']['joint_cpl:levels']}")
    assert np.isfinite(a).sum() > a.size // 2
    _assert_same_bits(modes, "joint_cpl:logl")
    assert not modes["level0"]["joint_cpl:levels"].any() and modes["level1"]["joint_cpl:levels"][0] == 3
