"""Runs tests/cpp/test_mip_bounded_gpu.cpp: Solver::boundedBranchAndBound from a Solver::boundedSimplex result, and
from a relaxation it solves itself, equals tests/ref/mip_bounded_ref.c."""
import os
import subprocess

import pytest

from simplexmethod_amd import build
from tests.test_host_cpp import _exe


@pytest.mark.gpu
def test_solver_bounded_branch_and_bound_gpu():
    env = dict(os.environ, LP_MIP_BOUNDED_REF=build.build_mip_bounded_ref())
    r = subprocess.run([_exe("test_mip_bounded_gpu")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout
