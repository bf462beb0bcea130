"""
The create-time packing of the streaming per-walker kernel (csrc/cf_stream_pack.h: the SNe sorted by the grid node of z_cmb and
assigned to the 512-node segment whose LDS window holds that node well inside) under AddressSanitizer + UBSan on the CPU, through
the stand-alone driver tools/stream_pack_check.cpp: every SN exactly once, its interval at least HALO / 2 - 1 nodes inside the
window, monotone offsets that end at n_sn, and a guard bound that admits the prior box's |v| = 300 km/s for the Pantheon+ shape.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "stream_pack_check.cpp")


def test_stream_packing_is_right_and_clean_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "stream_pack_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe],
                   check=True, cwd=ROOT)
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout and "Sanitizer" not in r.stderr
