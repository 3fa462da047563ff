"""Runs the C++ test of LinearSolvers::overwriting_solve_bunch_kaufman_multi
(tests/cpp/test_cxx_bk_multi.cpp): the multi-right-hand-side Bunch-Kaufman
solve through the reference-shaped C++ interface, each row against the
single-vector function."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cxx_bk_multi():
    exe = os.path.join(REPO, "ipm-zoo_amd", "build", "test_cxx_bk_multi")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(REPO, "ipm-zoo_amd"), "cxxtest"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cxx bk multi ok" in r.stdout
