"""Runs tests/cpp/test_bounded_large_gpu.cpp: Solver::boundedSimplexLarge equals the result vector that
tests/ref/bounded_ref.c recorded in tests/golden/bounded_large_case.json, and maps the failures to exceptions."""
import os
import subprocess

import pytest

from tests.test_host_cpp import _exe

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bounded_large_case.json")


@pytest.mark.gpu
def test_solver_bounded_simplex_large_gpu():
    env = dict(os.environ, LP_BOUNDED_LARGE_GOLDEN=GOLDEN)
    r = subprocess.run([_exe("test_bounded_large_gpu")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout
