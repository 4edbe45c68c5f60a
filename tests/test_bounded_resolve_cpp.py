"""Runs tests/cpp/test_bounded_resolve_gpu.cpp: Solver::boundedResolve equals tests/ref/bounded_resolve_ref.c."""
import os
import subprocess

import pytest

from simplexmethod_amd import build
from tests.test_host_cpp import _exe


@pytest.mark.gpu
def test_solver_bounded_resolve_gpu():
    env = dict(os.environ, LP_BOUNDED_RESOLVE_REF=build.build_bounded_resolve_ref())
    r = subprocess.run([_exe("test_bounded_resolve_gpu")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout
