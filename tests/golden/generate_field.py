#!/usr/bin/env python3
"""
Generate tests/golden/field.npz by RUNNING THE REFERENCE's field.py, once per parameter row.

Run from the repo root, in the build container only (needs the reference checkout):

    python tests/golden/generate_field.py

field.py is a script with its parameters typed in (field.py:8,9,11) and a plot after every block.  Each row runs in its own
subprocess: the text of the script is read from the reference at that moment, the three literals are replaced, and it is
executed with a stand-in for matplotlib whose every call returns at once.  Nothing of the script is written anywhere: the
fixture holds numbers only -- the parameters, and thinned copies of the arrays the script leaves in its namespace.

Rows: the script's own (66.53, 0.312, -0.763) and seven drawn with default_rng(5) from H0 55..85, Om 0.1..0.6, w0 -0.999..-0.34.
Thinning (the file stays under 256 KB): phi_vals, t_vals_Gyr, kinetic_term, potential_term at NODES = the first 32 nodes and
every 10th; phi_plot, V_of_phi(phi_plot), t_plot_range, a_of_t, phi_of_t at every 10th point.
"""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

REF = os.environ.get("COSMOFIT_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "field.npz")
N_A = 5000
NODES = np.unique(np.concatenate([np.arange(32), np.arange(0, N_A, 10)]))


def rows():
    rng = np.random.default_rng(5)
    drawn = np.column_stack([rng.uniform(55, 85, 7), rng.uniform(0.1, 0.6, 7), rng.uniform(-0.999, -0.34, 7)])
    return np.vstack([[66.53, 0.312, -0.763], drawn])


class _Stub:
    """matplotlib.pyplot for a script that only draws: every attribute is a callable that returns another stub."""

    def __getattr__(self, name):
        return _Stub()

    def __call__(self, *a, **k):
        return _Stub()


def run_row(H0, Om, w0, out_path):
    import types

    text = open(os.path.join(REF, "field.py")).read()
    for name, val in (("H0", H0), ("Om", Om), ("w0", w0)):
        text, n = re.subn(rf"^{name} = [-0-9.eE]+", f"{name} = {float(val)!r}", text, count=1, flags=re.M)
        assert n == 1, name
    mpl = types.ModuleType("matplotlib")
    mpl.pyplot = _Stub()
    sys.modules["matplotlib"], sys.modules["matplotlib.pyplot"] = mpl, mpl.pyplot
    ns = {"__name__": "__main__"}
    exec(compile(text, "field.py", "exec"), ns)
    assert ns["H0"] == float(H0) and ns["Om"] == float(Om) and ns["w0"] == float(w0) and ns["N_a"] == N_A
    tp = ns["t_plot_range"]
    np.savez(out_path,
             phi=ns["phi_vals"][NODES], t=ns["t_vals_Gyr"][NODES], K=ns["kinetic_term"][NODES], V=ns["potential_term"][NODES],
             phi_plot=ns["phi_plot"][::10], V_of_phi=ns["V_of_phi"](ns["phi_plot"])[::10],
             t_plot=tp[::10], a_of_t=ns["a_of_t"](tp)[::10], phi_of_t=ns["phi_of_t"](tp)[::10],
             scalars=np.array([ns["phi_today"], ns["t_today_Gyr"], ns["Hubble_time_Gyr"]]),
             sizes=np.array([ns["phi_plot"].size, tp.size]))


def main():
    theta = rows()
    per_row = []
    with tempfile.TemporaryDirectory() as tmp:
        for i, (H0, Om, w0) in enumerate(theta):
            path = os.path.join(tmp, f"row{i}.npz")
            subprocess.run([sys.executable, os.path.abspath(__file__), "--run", repr(float(H0)), repr(float(Om)), repr(float(w0)), path],
                           check=True, stdout=subprocess.DEVNULL, env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"))
            per_row.append(dict(np.load(path)))
    out = {k: np.stack([r[k] for r in per_row]) for k in per_row[0]}
    np.savez_compressed(OUT, theta=theta, nodes=NODES, **out)
    print(OUT, os.path.getsize(OUT), "bytes")
    assert os.path.getsize(OUT) < 256 * 1024


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--run":
        run_row(float(sys.argv[2]), float(sys.argv[3]), float(sys.argv[4]), sys.argv[5])
    else:
        main()
