"""Runs the C++ program of Solver::boundedBranchAndBoundLarge with snapshots (tests/cpp/mip_bounded_snapshots_gpu.cpp):
on the GPU, the searches at 4 x 14 and 160 x 320 against tests/ref/mip_bounded_snapshots_ref.c, in a child process."""
import os
import subprocess

import pytest

from simplexmethod_amd import build
from tests.test_host_cpp import _exe


@pytest.mark.gpu
def test_solver_program_gpu():
    env = dict(os.environ, LP_MIP_BOUNDED_SNAPSHOTS_REF=build.build_ref("mip_bounded_snapshots"))
    r = subprocess.run([_exe("mip_bounded_snapshots_gpu")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout
