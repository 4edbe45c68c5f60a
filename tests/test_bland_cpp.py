"""Runs tests/cpp/test_bland_gpu.cpp: Solver::setPivotRule(Bland) solves Beale's cycling LP, the default
Solver still throws the iteration-limit error."""
import subprocess

import pytest

from tests.test_host_cpp import _exe


@pytest.mark.gpu
def test_solver_bland_gpu():
    r = subprocess.run([_exe("test_bland_gpu")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout
