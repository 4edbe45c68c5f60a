"""simplexmethod_amd.build.REFS, the table build_ref works from, against tests/ref/: every source once, each
entry's includes as the source states them, and every entry builds into a library that loads."""
import ctypes as C
import os
import re

import pytest

from simplexmethod_amd import build


def _included(name, seen=None):
    """The names whose <name>_ref.c tests/ref/<name>_ref.c #includes, directly or through another."""
    seen = set() if seen is None else seen
    with open(os.path.join(build.TESTS_REF, name + "_ref.c")) as f:
        for inc in re.findall(r'^\s*#\s*include\s+"(\w+)_ref\.c"', f.read(), re.M):
            if inc not in seen:
                seen.add(inc)
                _included(inc, seen)
    return seen


def test_table_names_every_source_once():
    sources = sorted(f for f in os.listdir(build.TESTS_REF) if f.endswith(".c"))
    assert sources == sorted(name + "_ref.c" for name in build.REFS)


@pytest.mark.parametrize("name", sorted(build.REFS))
def test_includes_are_the_sources(name):
    incs = build.REFS[name]
    assert len(set(incs)) == len(incs)
    assert set(incs) == _included(name)
    assert name not in incs


@pytest.mark.parametrize("name", sorted(build.REFS))
def test_build_ref_gives_a_loadable_library(name):
    lib = build.build_ref(name)
    assert lib == os.path.join(build.TESTS_REF, "_build", "lib" + name + "_ref.so")
    assert os.path.getmtime(lib) >= max(os.path.getmtime(os.path.join(build.TESTS_REF, d + "_ref.c"))
                                        for d in (name,) + tuple(build.REFS[name]))
    C.CDLL(lib)


def test_build_ref_without_the_source_is_none():
    assert build.build_ref("no_such") is None
