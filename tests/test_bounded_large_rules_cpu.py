"""lp_simplex_bounded_large_ex and lp_simplex_bounded_resolve_large_ex without a GPU: the entries are declared, bound
and exported, they refuse before touching a device, and the inputs of tests/test_gpu_bounded_large_rules.py reach what
that file claims for them, on the rules reference (tests/ref/bounded_rules_ref.c, bounded_resolve_rules_ref.c) alone: the
pinned counts show that each rule takes its own path on every input, so the GPU comparisons cannot pass vacuously."""
import ctypes as C
import inspect

import numpy as np
import pytest

from simplexmethod_amd import build, capi
from tests import bounded_large_cases as K
from tests import bounded_large_rules_cases as X
from tests import bounded_resolve_large_cases as Q
from tests import bounded_rules_ref as RR
from tests.test_gpu_bounded import _same

DANTZIG, BLAND, DEVEX = RR.RULES


def test_entries_are_declared_bound_and_exported():
    S = capi.SIGNATURES
    for plain in ("lp_simplex_bounded_large", "lp_simplex_bounded_resolve_large"):
        assert plain + "_ex" in S
        assert S[plain + "_ex"] == (S[plain][0], S[plain][1] + [C.c_int])   # the plain arity plus the rule
    assert len(S["lp_simplex_bounded_large_ex"][1]) == 18
    assert len(S["lp_simplex_bounded_resolve_large_ex"][1]) == 20
    assert S["lp_simplex_bounded_large_ex"] == S["lp_simplex_bounded_ex"]
    assert S["lp_simplex_bounded_resolve_large_ex"] == S["lp_simplex_bounded_resolve_ex"]
    build.build_hip()
    lib = C.CDLL(build.HIP_LIB)
    assert hasattr(lib, "lp_simplex_bounded_large_ex") and hasattr(lib, "lp_simplex_bounded_resolve_large_ex")
    for method in ("bounded_large", "bounded_resolve_large"):
        assert inspect.signature(getattr(capi.Context, method)).parameters["pivot_rule"].default is None


def test_refuse_without_a_context_and_an_unknown_rule_writes_nothing():
    lib = capi.load()
    d = np.zeros(16).ctypes.data_as(C.POINTER(C.c_double))
    i = np.zeros(16, np.int32).ctypes.data_as(C.POINTER(C.c_int))
    for rule in RR.RULES:
        assert lib.lp_simplex_bounded_large_ex(None, d, 2, 4, d, d, d, d, 1, 4, 1e-9, 10, d, i, i, d, i,
                                               rule) == RR.BAD_ARG
        assert lib.lp_simplex_bounded_resolve_large_ex(None, d, 2, 4, d, d, d, d, i, i, 1, 4, 1e-9, 10, d, i, i, d, i,
                                                       rule) == RR.BAD_ARG
    # the reference refuses an unknown rule before it writes an output, like the library (the GPU test shows that)
    A, b, c, lo, hi, mx = K.boxed(6, 16, "mixed", 1)
    for rule in (3, -1):
        r = RR.bounded(A, b, c, lo, hi, mx, rule=rule)
        assert r["status"] == RR.BAD_ARG and np.all(r["basis"] == -1) and r["iters"] == [0, 0, 0, 0]


def test_rule_zero_is_the_plain_reference_on_every_input():
    for key in X.BOXED:
        m, n = key[:2]
        A, b, c, lo, hi, mx = K.boxed(*key)
        _same(X.boxed_ref(key, DANTZIG), K.ref(("rules-plain",) + key, A, b, c, lo, hi, mx, n - m))
    m, n = X.TALL_SHAPE
    A, b, c, lo, hi, mx = K.boxed(m, n, "mixed", 1)
    _same(X.tall_ref(DANTZIG), K.ref(("tall", "mixed", 1), A, b, c, lo, hi, mx, n - m, max_iter=K.TALL_MAX_ITER))
    from tests import bounded_ref as R
    _same(X.cycling_ref(DANTZIG), R.bounded(*RR.cycling_boxed(), True, max_iter=X.CYCLING_MAX_ITER))
    _same(X.beale_ref(DANTZIG), R.bounded(*RR.beale_boxed(), True, max_iter=X.BEALE_MAX_ITER))
    for key in X.DRIVEOUT_FLIP:
        _same(X.driveout_flip_ref(key, DANTZIG), K.ref(("driveout_flip",) + key, *K.driveout_with_flip(*key)))
    for seed in X.DRIVEOUT_SEEDS:
        _same(X.driveout_ref(seed, DANTZIG), K.ref(("driveout", seed), *K.driveout(seed)))
    for name in X.RESOLVE:
        start, mx = X.resolve_start(name)
        _same(X.resolve_ref(name, DANTZIG, start, mx), Q.ref(("rules-plain", name), start, mx))


@pytest.mark.parametrize("key", sorted(X.BOXED))
def test_boxed_counts(key):
    assert capi.load().lp_simplex_bounded_fits(*key[:2]) == int(key[:2] == (67, 201))
    for rule, (status, iters) in X.BOXED[key].items():
        r = X.boxed_ref(key, rule)
        assert (r["status"], r["iters"]) == (status, iters)
        assert iters[0] > 0 and iters[2] > 0 and iters[3] > 0   # pivots in both phases, and flips
    counts = [tuple(v[1]) for v in X.BOXED[key].values()]
    assert len(set(counts)) == len(counts)   # every rule takes its own path


def test_tall_counts():
    m, n = X.TALL_SHAPE
    assert m > 1024 and n + m > 64 * 16   # (phase I prices n + m columns: beyond one tile of Bland's scan)
    for rule, (status, iters) in X.TALL.items():
        r = X.tall_ref(rule)
        assert (r["status"], r["iters"]) == (status, iters) and sum(iters) == X.TALL_MAX_ITER
    assert X.tall_ref(DANTZIG)["iters"] == K.TALL[("mixed", 1)]


def test_wide_counts():
    m, n = X.WIDE_KEY[:2]
    assert n > 4 * 1024   # beyond one step of Devex's pricing and staging loops, in phase II too
    for rule, (status, iters) in X.WIDE.items():
        r = X.wide_ref(rule)
        assert (r["status"], r["iters"]) == (status, iters)
        assert r["basis"].max() >= 4 * 1024 and iters[0] > 0 and iters[2] > 0 and iters[3] > 0
    A, b, c, lo, hi, mx = K.boxed(*X.WIDE_KEY)
    _same(X.wide_ref(DANTZIG), K.ref(("rules-plain-wide",), A, b, c, lo, hi, mx, n - m))


def test_cycling_counts():
    for rule, (status, iters) in X.CYCLING.items():
        r = X.cycling_ref(rule)
        assert (r["status"], r["iters"]) == (status, iters)
    for rule, (status, iters) in X.BEALE.items():
        r = X.beale_ref(rule)
        assert r["status"] == status and (iters is None or r["iters"] == iters)
    A = RR.cycling_boxed()[0]
    assert capi.load().lp_simplex_bounded_fits(*A.shape) == 1   # 64 x 128: the one cycling LP at hand fits LDS too


@pytest.mark.parametrize("key", sorted(X.DRIVEOUT_FLIP))
def test_driveout_with_flip_counts(key):
    for rule, iters in X.DRIVEOUT_FLIP[key].items():
        r = X.driveout_flip_ref(key, rule)
        assert (r["status"], r["iters"]) == (RR.OPTIMAL, iters)


@pytest.mark.parametrize("seed", X.DRIVEOUT_SEEDS)
def test_driveout_counts(seed):
    r = X.driveout_ref(seed, BLAND)
    assert r["status"] == RR.OPTIMAL and 5 <= r["iters"][1] <= 7
    r = X.driveout_ref(seed, DEVEX)   # Devex cycles in phase I: no anti-cycling rule
    assert r["status"] == RR.ITER_LIMIT and r["iters"] == [X.DRIVEOUT_DEVEX_MAX_ITER, 0, 0, 0]


def test_limit_sweep_mixes_flips_and_pivots():
    A, b, c, lo, hi, mx = K.boxed(160, 320, "mixed", 1)
    seen = [X.ref(("limit", k), DEVEX, A, b, c, lo, hi, mx, 160, max_iter=k) for k in X.LIMIT_SWEEP]
    assert all(r["status"] == RR.ITER_LIMIT and sum(r["iters"]) == k for r, k in zip(seen, X.LIMIT_SWEEP))
    assert seen[-1]["iters"][0] > 0 and seen[-1]["iters"][3] > 0
    assert seen[-1]["iters"] != seen[-2]["iters"]


@pytest.mark.parametrize("name", sorted(X.RESOLVE))
def test_resolve_counts(name):
    start, mx = X.resolve_start(name)
    for rule, iters in X.RESOLVE[name].items():
        r = X.resolve_ref(name, rule, start, mx)
        assert (r["status"], r["iters"]) == (RR.OPTIMAL, iters)
    if name == "bound_max":   # the dual branch: every output is the same under every rule
        for rule in X.NEW_RULES:
            _same(X.resolve_ref(name, rule, start, mx), X.resolve_ref(name, DANTZIG, start, mx))
