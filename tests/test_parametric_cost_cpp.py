"""Runs tests/cpp/test_parametric_cost_gpu.cpp: Solver::parametricCost after Solver::twoPhaseSimplex_ex equals
tests/ref/parametric_cost_ref.c bit for bit, and the path it returns is concave."""
import os
import subprocess

import pytest

from simplexmethod_amd import build
from tests.test_host_cpp import _exe


@pytest.mark.gpu
def test_solver_parametric_cost_gpu():
    env = dict(os.environ, LP_PARAMETRIC_COST_REF=build.build_parametric_cost_ref())
    r = subprocess.run([_exe("test_parametric_cost_gpu")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout
