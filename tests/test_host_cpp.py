"""Runs the C++ tests of the host classes (tests/cpp/*.cpp): the CPU-only one mirrors the
reference's gtest cases for Canonical / Symmetrical / SymmetricalParser and pins what Solver does
before it reaches the device; the GPU ones drive the drop-in Solver / EnumerationSolver classes on
the device, one program per feature of Solver (SOLVER_PROGRAMS)."""
import functools
import glob
import os
import subprocess

import pytest

from simplexmethod_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _exe(name):
    """The prebuilt test executable (built by __graft_entry__.build()); built here only if missing —
    on the GPU box the snapshot's file times say nothing about staleness."""
    path = os.path.join(build.TESTS_OUT, name)
    if not os.path.exists(path):
        exes = {os.path.basename(e): e for e in build.build_cpp_tests()}
        assert name in exes, f"{name} was not built"
        path = exes[name]
    return path


def test_host_classes_cpu():
    r = subprocess.run([_exe("test_host")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout


@pytest.mark.gpu
def test_solver_classes_gpu():
    r = subprocess.run([_exe("test_solvers_gpu")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout


def _ref(name):
    """The C restatement tests/ref/<name>_ref.c as a shared library, built when the test runs."""
    return functools.partial(build.build_ref, name)


def _golden(name):
    return functools.partial(os.path.join, ROOT, "tests", "golden", name)


# The programs that test one feature of Solver on the device: executable -> the environment variables it reads and
# what each names (a restatement it loads at run time and compares against bit for bit, or a file of recorded results).
SOLVER_PROGRAMS = {
    "test_bland_gpu": {},
    "test_bounded_certificate_gpu": {"LP_BOUNDED_CERTIFICATE_REF": _ref("bounded_certificate")},
    "test_bounded_gpu": {"LP_BOUNDED_REF": _ref("bounded")},
    "test_bounded_large_gpu": {"LP_BOUNDED_LARGE_GOLDEN": _golden("bounded_large_case.json")},
    "test_bounded_parametric_gpu": {"LP_BOUNDED_PARAMETRIC_REF": _ref("bounded_parametric")},
    "test_bounded_resolve_gpu": {"LP_BOUNDED_RESOLVE_REF": _ref("bounded_resolve")},
    "test_bounded_rules_gpu": {},
    "test_bounded_sens_gpu": {"LP_BOUNDED_SENS_REF": _ref("bounded_sens")},
    "test_certificate_gpu": {"LP_CERTIFICATE_REF": _ref("certificate")},
    "test_devex_gpu": {"LP_DEVEX_GOLDEN": _golden("devex_cases.json")},
    "test_duals_gpu": {},
    "test_mip_bounded_gpu": {"LP_MIP_BOUNDED_REF": _ref("mip_bounded")},
    "test_mip_gpu": {"LP_MIP_REF": _ref("mip")},
    "test_parametric_cost_gpu": {"LP_PARAMETRIC_COST_REF": _ref("parametric_cost")},
    "test_parametric_gpu": {"LP_PARAMETRIC_REF": _ref("parametric")},
    "test_ranging_gpu": {"LP_RANGING_REF": _ref("ranging")},
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SOLVER_PROGRAMS))
def test_solver_program_gpu(name):
    env = dict(os.environ, **{var: value() for var, value in SOLVER_PROGRAMS[name].items()})
    r = subprocess.run([_exe(name)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout


def test_every_cpp_program_has_a_runner():
    sources = glob.glob(os.path.join(build.TESTS_CPP, "test_*.cpp"))
    programs = {os.path.splitext(os.path.basename(p))[0] for p in sources}
    assert programs == set(SOLVER_PROGRAMS) | {"test_host", "test_solvers_gpu"}
