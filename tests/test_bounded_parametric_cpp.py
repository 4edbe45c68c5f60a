"""Runs tests/cpp/test_bounded_parametric_gpu.cpp: Solver::boundedParametricRhs and Solver::boundedParametricCost after
Solver::boundedSimplex, and the batched C calls, equal tests/ref/bounded_parametric_ref.c bit for bit at two shapes;
statuses and exceptions."""
import os
import subprocess

import pytest

from simplexmethod_amd import build
from tests.test_host_cpp import _exe


@pytest.mark.gpu
def test_solver_bounded_parametric_gpu():
    env = dict(os.environ, LP_BOUNDED_PARAMETRIC_REF=build.build_bounded_parametric_ref())
    r = subprocess.run([_exe("test_bounded_parametric_gpu")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout
