"""Runs tests/cpp/test_bounded_rules_gpu.cpp: the Solver::boundedSimplex / boundedResolve overloads with a pivot rule
on Beale's LP with boxed columns."""
import subprocess

import pytest

from tests.test_host_cpp import _exe


@pytest.mark.gpu
def test_solver_bounded_rules_gpu():
    r = subprocess.run([_exe("test_bounded_rules_gpu")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout
