"""Runs the C++ programs of Solver::boundedCertificateLarge (tests/cpp/bounded_certificate_large_*.cpp): the size checks
that need no device, and on the GPU the certificate after Solver::boundedSimplexLarge and Solver::boundedResolveLarge
at 160 x 320 against its own inequalities and tests/ref/bounded_certificate_ref.c."""
import os
import subprocess

import pytest

from simplexmethod_amd import build
from tests.test_host_cpp import _exe


def test_size_checks_cpu():
    r = subprocess.run([_exe("bounded_certificate_large_sizes")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout


@pytest.mark.gpu
def test_solver_program_gpu():
    env = dict(os.environ, LP_BOUNDED_CERTIFICATE_REF=build.build_ref("bounded_certificate"))
    r = subprocess.run([_exe("bounded_certificate_large_gpu")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout
