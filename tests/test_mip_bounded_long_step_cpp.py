"""Runs the C++ program of Solver::boundedBranchAndBound / boundedBranchAndBoundLarge under a dual ratio test
(tests/cpp/mip_bounded_long_step_gpu.cpp): on the GPU, the searches under DualRatio::LongStep at 8 x 20 and at 67 x 201
against tests/ref/mip_bounded_long_step_ref.c, in a child process."""
import os
import subprocess

import pytest

from simplexmethod_amd import build
from tests.test_host_cpp import _exe


@pytest.mark.gpu
def test_solver_program_gpu():
    env = dict(os.environ, LP_MIP_BOUNDED_LONG_STEP_REF=build.build_ref("mip_bounded_long_step"))
    r = subprocess.run([_exe("mip_bounded_long_step_gpu")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout
