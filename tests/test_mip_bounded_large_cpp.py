"""Runs the C++ programs of Solver::boundedBranchAndBoundLarge (tests/cpp/mip_bounded_large_*.cpp): the size and argument
checks that need no device, and on the GPU the search after Solver::boundedSimplexLarge at 160 x 320 against
tests/ref/mip_bounded_ref.c."""
import os
import subprocess

import pytest

from simplexmethod_amd import build
from tests.test_host_cpp import _exe


def test_size_checks_cpu():
    r = subprocess.run([_exe("mip_bounded_large_sizes")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout


@pytest.mark.gpu
def test_solver_program_gpu():
    env = dict(os.environ, LP_MIP_BOUNDED_REF=build.build_ref("mip_bounded"))
    r = subprocess.run([_exe("mip_bounded_large_gpu")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout
