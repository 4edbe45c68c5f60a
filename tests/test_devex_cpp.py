"""Runs tests/cpp/test_devex_gpu.cpp: Solver::setPivotRule(PivotRule::Devex) on solve() and twoPhaseSimplex()
against tests/golden/devex_cases.json (written by tests/golden/make_devex_golden.py from tests/ref/devex_ref.c)."""
import os
import subprocess

import pytest

from tests.test_host_cpp import _exe

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "devex_cases.json")


@pytest.mark.gpu
def test_solver_devex_gpu():
    env = dict(os.environ, LP_DEVEX_GOLDEN=GOLDEN)
    r = subprocess.run([_exe("test_devex_gpu")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout
