"""Runs the C++ programs of Solver::boundedParametricRhsLarge and Solver::boundedParametricCostLarge
(tests/cpp/bounded_parametric_large_*.cpp): the size checks that need no device, and on the GPU both paths after
Solver::boundedSimplexLarge at 160 x 320 against the C entries and tests/ref/bounded_parametric_ref.c, and against the LDS
methods at a shape that fits."""
import os
import subprocess

import pytest

from simplexmethod_amd import build
from tests.test_host_cpp import _exe


def test_size_checks_cpu():
    r = subprocess.run([_exe("bounded_parametric_large_sizes")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout


@pytest.mark.gpu
def test_solver_program_gpu():
    env = dict(os.environ, LP_BOUNDED_PARAMETRIC_REF=build.build_ref("bounded_parametric"))
    r = subprocess.run([_exe("bounded_parametric_large_gpu")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout
