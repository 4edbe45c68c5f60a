"""Runs tests/cpp/test_duals_gpu.cpp: Solver::duals of MIN canonical problems equals the solution of their
Canonical::GetDual() (y = u - v, d = the dual's slacks)."""
import subprocess

import pytest

from tests.test_host_cpp import _exe


@pytest.mark.gpu
def test_solver_duals_gpu():
    r = subprocess.run([_exe("test_duals_gpu")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout
