"""Runs tests/cpp/test_ranging_gpu.cpp: Solver::ranging after Solver::twoPhaseSimplex_ex equals
tests/ref/ranging_ref.c bit for bit, and the basis stays optimal just inside every finite end."""
import os
import subprocess

import pytest

from simplexmethod_amd import build
from tests.test_host_cpp import _exe


@pytest.mark.gpu
def test_solver_ranging_gpu():
    env = dict(os.environ, LP_RANGING_REF=build.build_ranging_ref())
    r = subprocess.run([_exe("test_ranging_gpu")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout
