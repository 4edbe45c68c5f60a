"""Runs the C++ program of Solver::boundedResolve / boundedResolveLarge under a dual pricing rule
(tests/cpp/bounded_resolve_dual_rules_gpu.cpp): on the GPU, the re-solves under DualRule::Devex at 32 x 96 and at
160 x 320 against tests/ref/bounded_resolve_dual_rules_ref.c."""
import os
import subprocess

import pytest

from simplexmethod_amd import build
from tests.test_host_cpp import _exe


@pytest.mark.gpu
def test_solver_program_gpu():
    env = dict(os.environ, LP_BOUNDED_RESOLVE_DUAL_RULES_REF=build.build_ref("bounded_resolve_dual_rules"))
    r = subprocess.run([_exe("bounded_resolve_dual_rules_gpu")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout
