"""Runs the C++ programs of the Solver::boundedSimplexLarge / boundedResolveLarge overloads that take a pivot rule
(tests/cpp/bounded_large_rules_*.cpp): the size checks that need no device, and on the GPU Bland's rule on the cycling
boxed LP and Devex pricing at 160 x 320 against tests/golden/bounded_large_rules_cases.json."""
import os
import subprocess

import pytest

from tests.test_host_cpp import ROOT, _exe


def test_size_checks_cpu():
    r = subprocess.run([_exe("bounded_large_rules_sizes")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout


@pytest.mark.gpu
def test_solver_program_gpu():
    golden = os.path.join(ROOT, "tests", "golden", "bounded_large_rules_cases.json")
    env = dict(os.environ, LP_BOUNDED_LARGE_RULES_GOLDEN=golden)
    r = subprocess.run([_exe("bounded_large_rules_gpu")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout
