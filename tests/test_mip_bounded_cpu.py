"""CPU-only: tests/ref/mip_bounded_ref.c (the definition of lp_mip_bounded_solve: branch-and-bound over variable bounds)
against enumeration, scipy's milp, bounded_resolve_ref.c and mip_ref.c; its limits and refusals; the host-side fits
predicate and the NULL-context refusals of the C ABI."""
import ctypes as C

import numpy as np
import pytest

from simplexmethod_amd import capi
from tests import bounded_ref as B
from tests import bounded_resolve_ref as BR
from tests import mip_bounded_ref as R
from tests import mip_ref as M

OPTIMAL, UNBOUNDED, ITER_LIMIT, SINGULAR, INFEASIBLE, BAD_ARG = range(6)


def _bits_equal(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    nan = np.isnan(a)
    assert np.array_equal(nan, np.isnan(b))
    assert np.array_equal(a[~nan], b[~nan])


def _search(A, b, c, lo, hi, mask, maximize, root, **kw):
    """The search from a cold root; a root that is not optimal gives its status, as the root_status chain does."""
    if root["status"] != OPTIMAL:
        return dict(status=root["status"], found=0, x=np.full(A.shape[1], np.nan), obj=np.nan, bound=np.nan,
                    stats=(0, 0, 0, 0, 0))
    return R.mip(A, b, c, lo, hi, root["basis"], root["at_upper"], mask, maximize, **kw)


def _mk(s):
    """m in 2..6 and k in 4..10, as test_mip_cpu.py draws them for its 64 knapsacks."""
    rng = np.random.default_rng(1000 + s)
    return int(rng.integers(2, 7)), int(rng.integers(4, 11))


@pytest.mark.parametrize("s", range(64))
def test_boxed_knapsack_matches_enumeration(s):
    m, k = _mk(s)
    A, b, c, lo, hi, mask, root = R.boxed_knapsack(s, m, k)
    r = _search(A, b, c, lo, hi, mask, True, root, n_orig=k)
    best, _ = R.enumerate_box(A[:, :k], b, c[:k], lo[:k], hi[:k])
    assert r["status"] in (OPTIMAL, INFEASIBLE)
    if best is None:
        assert r["status"] == INFEASIBLE and r["found"] == 0
        return
    assert r["status"] == OPTIMAL and r["found"] == 1
    assert abs(r["obj"] - best) <= 1e-9 * abs(best)
    x = r["x"]
    assert np.all(np.abs(x - np.round(x)) <= 1e-6)
    assert np.all(x >= lo[:k] - 1e-6) and np.all(x <= hi[:k] + 1e-6)
    assert np.all(A[:, :k] @ x <= b + 1e-6)
    assert r["bound"] == r["obj"]


def test_boxed_knapsacks_reach_both_outcomes():
    st = []
    for s in range(64):
        m, k = _mk(s)
        A, b, c, lo, hi, mask, root = R.boxed_knapsack(s, m, k)
        st.append(_search(A, b, c, lo, hi, mask, True, root, n_orig=k)["status"])
    assert st.count(OPTIMAL) >= 48 and st.count(INFEASIBLE) >= 1


@pytest.mark.parametrize("s", range(32))
def test_mixed_integer_matches_milp(s):
    A, b, c, lo, hi, mask, maximize, root = R.mixed_case(s)
    assert mask.sum() > 0 and mask.sum() < A.shape[1] - A.shape[0]   # half the structural columns stay continuous
    r = _search(A, b, c, lo, hi, mask, maximize, root)
    st, obj = R.milp(A, b, c, lo, hi, mask, maximize)
    assert r["status"] == st
    if st == OPTIMAL:
        assert abs(r["obj"] - obj) <= 1e-7 * max(1.0, abs(obj))
        x = r["x"]
        assert np.all(np.abs(x[mask == 1] - np.round(x[mask == 1])) <= 1e-6)
        assert np.all(x >= lo - 1e-6) and np.all(x <= hi + 1e-6)
        assert np.allclose(A @ x, b, atol=1e-6)


def _cold(i, maximize, m=6, n=16):
    """The i-th boxed LP (by seed) of this sense whose cold solve is optimal."""
    seed = -1
    while i >= 0:
        seed += 1
        A, b, c, lo, hi, _ = B.boxed_lp(seed, m, n, maximize=maximize, kind="mixed")
        cold = B.bounded(A, b, c, lo, hi, maximize)
        i -= cold["status"] == OPTIMAL
    return seed, A, b, c, lo, hi, cold


@pytest.mark.parametrize("kind", ["bound", "cost"])
@pytest.mark.parametrize("maximize", [True, False])
@pytest.mark.parametrize("i", range(6))
def test_zero_mask_is_the_bounded_resolve(i, maximize, kind):
    """bound: the start is only dual feasible (the dual loop); cost: only primal feasible (the primal loop)."""
    m, n = 6, 16
    seed, A, b, c, lo, hi, cold = _cold(i, maximize)
    b2, c2, lo2, hi2 = BR.perturb(seed, kind, b, c, lo, hi, cold["basis"], cold["x"])
    g = BR.resolve(A, b2, c2, lo2, hi2, cold["basis"], cold["at_upper"], maximize, n - m)
    r = R.mip(A, b2, c2, lo2, hi2, cold["basis"], cold["at_upper"], np.zeros(n, np.int32), maximize, n - m)
    assert r["status"] == g["status"]
    assert list(r["stats"][1:4]) == g["iters"]
    assert r["stats"][0] == 1 and r["stats"][4] == 0
    if g["status"] == OPTIMAL:
        assert r["found"] == 1
        _bits_equal(r["x"], g["x"])
        _bits_equal(r["obj"], g["obj"])
        _bits_equal(r["bound"], g["obj"])
    else:
        assert r["found"] == 0 and np.isnan(r["obj"]) and np.all(np.isnan(r["x"]))


def test_zero_mask_cases_take_both_loops():
    dual = primal = 0
    for i in range(6):
        for maximize in (True, False):
            seed, A, b, c, lo, hi, cold = _cold(i, maximize)
            for kind in ("bound", "cost"):
                b2, c2, lo2, hi2 = BR.perturb(seed, kind, b, c, lo, hi, cold["basis"], cold["x"])
                st = R.mip(A, b2, c2, lo2, hi2, cold["basis"], cold["at_upper"], np.zeros(16, np.int32),
                           maximize)["stats"]
                dual += st[1] > 0
                primal += st[2] + st[3] > 0
    assert dual > 0 and primal > 0


def test_zero_mask_follows_every_outcome_of_the_bounded_resolve():
    """The install kept in mip_bounded_ref.c is ref_bounded_resolve's: on one start per outcome of the re-solve
    (complement in the dual loop, flips in the primal loop, infeasible, crossed bounds, unbounded, iteration limit,
    singular, no valid start) the zero-mask search returns its status, counters, x and obj."""
    cases = BR.outcome_cases()
    assert len(cases) == 8
    for name, (A, b, c, lo, hi, basis, up), status in cases:
        n = A.shape[1]
        g = BR.resolve(A, b, c, lo, hi, basis, up, True, max_iter=3)
        r = R.mip(A, b, c, lo, hi, basis, up, np.zeros(n, np.int32), True, max_iter=3)
        assert g["status"] == status == r["status"], name
        assert list(r["stats"][1:4]) == g["iters"] and r["stats"][0] == 1, name
        assert r["found"] == (status == OPTIMAL), name
        _bits_equal(r["x"], g["x"])
        _bits_equal(r["obj"], g["obj"])
        want = {UNBOUNDED: np.inf, ITER_LIMIT: np.inf}.get(status, g["obj"])   # (max: +inf for an unfinished root)
        _bits_equal(r["bound"], want)


@pytest.mark.parametrize("s", range(64))
def test_unboxed_agrees_with_the_row_form(s):
    """lo = 0, hi = inf, the slack basis: the search of mip_ref.c by rows and this one by bounds reach the same
    status and objective (their trees differ, so bit equality is not expected)."""
    m, k = _mk(s)
    A, b, c, basis, mask = M.knapsack(s, m, k, box=2 if k > 7 else 3)
    n = m + k
    g = M.mip(A, b, c, basis, mask, True, k)
    r = R.mip(A, b, c, np.zeros(n), np.full(n, np.inf), basis, np.zeros(n, np.int32), mask, True, k, max_depth=32)
    assert g["status"] == OPTIMAL
    assert r["status"] == g["status"]
    assert abs(r["obj"] - g["obj"]) <= 1e-9 * abs(g["obj"])


def test_search_deeper_than_the_row_form_allows():
    A, b, c, lo, hi, mask, maximize, root = R.deep_case()
    k = R.DEEP_K
    assert root["status"] == OPTIMAL
    r = R.mip(A, b, c, lo, hi, root["basis"], root["at_upper"], mask, maximize, k, max_depth=1024)
    assert r["stats"][4] > 64
    assert r["status"] == OPTIMAL and r["found"] == 1
    st, obj = R.milp(A, b, c, lo, hi, mask, maximize)
    assert st == OPTIMAL and abs(r["obj"] - obj) <= 1e-7 * abs(obj)
    # the row form's cap stops the same search short
    capped = R.mip(A, b, c, lo, hi, root["basis"], root["at_upper"], mask, maximize, k, max_depth=64)
    assert capped["stats"][4] == 64


def _limit_case():
    """A boxed knapsack whose full search branches, finds its incumbent late enough for every limit to bite."""
    for s in range(200):
        A, b, c, lo, hi, mask, root = R.boxed_knapsack(300 + s, 4, 9)
        if root["status"] != OPTIMAL:
            continue
        full = R.mip(A, b, c, lo, hi, root["basis"], root["at_upper"], mask, True, 9)
        if full["status"] == OPTIMAL and full["stats"][0] >= 12 and full["stats"][4] >= 3:
            return A, b, c, lo, hi, mask, root, full
    raise AssertionError("no limit case")


def test_limits_keep_the_incumbent_and_the_bound_side():
    A, b, c, lo, hi, mask, root, full = _limit_case()
    start = (root["basis"], root["at_upper"])
    seen_incumbent = 0
    for nodes in range(1, full["stats"][0]):
        r = R.mip(A, b, c, lo, hi, *start, mask, True, 9, max_nodes=nodes)
        assert r["status"] == ITER_LIMIT and r["stats"][0] == nodes
        assert r["bound"] >= full["obj"] - 1e-9   # max: the bound stays above the optimum
        if r["found"]:
            seen_incumbent += 1
            assert r["obj"] <= full["obj"] + 1e-9 and r["bound"] >= r["obj"]
            assert np.all(np.abs(r["x"] - np.round(r["x"])) <= 1e-6)
    assert seen_incumbent > 0
    d0 = R.mip(A, b, c, lo, hi, *start, mask, True, 9, max_depth=0)
    assert d0["status"] == ITER_LIMIT and d0["found"] == 0 and d0["stats"] == (1,) + d0["stats"][1:4] + (0,)
    assert d0["bound"] >= full["obj"] - 1e-9 and np.isnan(d0["obj"])
    for depth in range(1, full["stats"][4]):
        r = R.mip(A, b, c, lo, hi, *start, mask, True, 9, max_depth=depth)
        assert r["stats"][4] <= depth
        assert r["status"] in (OPTIMAL, ITER_LIMIT)
        assert r["bound"] >= full["obj"] - 1e-9
        if r["status"] == OPTIMAL:
            assert abs(r["obj"] - full["obj"]) <= 1e-9 * abs(full["obj"])
    it = R.mip(A, b, c, lo, hi, *start, mask, True, 9, max_iter=1)
    assert it["status"] == ITER_LIMIT
    assert it["bound"] >= full["obj"] - 1e-9 or np.isinf(it["bound"])
    if it["found"]:
        assert it["obj"] <= full["obj"] + 1e-9


def test_reference_refusals():
    A, b, c, lo, hi, mask, root = R.boxed_knapsack(0, 3, 5)
    n = 8
    ok = dict(A=A, b=b, c=c, lo=lo, hi=hi, basis=root["basis"], at_upper=root["at_upper"], integer=mask, n_orig=5)
    assert R.mip(**ok)["status"] == OPTIMAL

    def refused(**kw):
        return R.mip(**{**ok, **kw})["status"] == BAD_ARG

    # what the bounded re-solve refuses
    assert refused(lo=np.r_[np.nan, lo[1:]]) and refused(lo=np.r_[-np.inf, lo[1:]]) and refused(hi=np.r_[np.nan, hi[1:]])
    assert refused(basis=np.r_[n, root["basis"][1:]]) and refused(basis=np.r_[-1, root["basis"][1:]])
    assert refused(at_upper=np.r_[2, root["at_upper"][1:]])
    up_on_inf = root["at_upper"].copy()
    up_on_inf[n - 1] = 1   # a slack: hi = inf
    assert refused(at_upper=up_on_inf)
    assert refused(n_orig=0) and refused(n_orig=n + 1)
    # what the row-form search refuses
    assert refused(integer=np.r_[2, mask[1:]])
    assert refused(integer=np.r_[mask[:-1], 1])   # a mark at j >= n_orig
    assert refused(int_tol=-1e-3) and refused(int_tol=0.5) and refused(int_tol=np.nan)
    assert refused(gap=-1.0) and refused(gap=np.nan)
    assert refused(max_nodes=0)
    assert refused(max_depth=-1) and refused(max_depth=1025)
    assert not refused(max_depth=1024) and not refused(max_depth=0)
    # new: fractional bounds on a marked column
    assert refused(lo=np.r_[0.5, lo[1:]])
    assert refused(hi=np.r_[hi[0] + 0.5, hi[1:]])
    assert not refused(hi=np.r_[np.inf, hi[1:]], at_upper=np.r_[0, root["at_upper"][1:]])
    # a fractional bound on an unmarked column is fine
    free_mask = mask.copy()
    free_mask[0] = 0
    assert not refused(integer=free_mask, hi=np.r_[hi[0] + 0.5, hi[1:]])


def test_fits_predicate():
    lib = capi.load()
    assert lib.lp_mip_bounded_fits(64, 192, 64) == 1
    assert lib.lp_mip_bounded_fits(32, 96, 256) == 1
    assert lib.lp_mip_bounded_fits(16, 40, 1024) == 1
    assert lib.lp_mip_bounded_fits(160, 320, 0) == 0
    for m, n in ((16, 40), (64, 192), (4, 10)):
        assert lib.lp_mip_bounded_fits(m, n, -1) == 0
        assert lib.lp_mip_bounded_fits(m, n, 1025) == 0
        assert lib.lp_mip_bounded_fits(m, n, 0) == 1
    assert lib.lp_mip_bounded_fits(64, 192, 1024) == 0   # the records alone pass 160 KB
    assert lib.lp_mip_bounded_fits(0, 4, 4) == 0 and lib.lp_mip_bounded_fits(5, 4, 4) == 0
    # the row form trades depth against shape: it cannot hold 64 x 192 at depth 64
    assert lib.lp_mip_fits(64, 192, 64) == 0


def test_capi_refuses_without_a_context():
    lib = capi.load()
    d = (C.c_double * 16)()
    i = (C.c_int * 16)()
    assert lib.lp_mip_bounded_solve(None, d, 2, 4, d, d, d, d, i, i, 1, 2, i, 1e-9, 1e-6, 1e-9, 4, 10, 10, d, d, d, i,
                                    i) == BAD_ARG
    assert lib.lp_mip_bounded_solve_batched(None, 1, d, 2, 4, d, d, d, d, i, i, None, 1, 2, i, 1e-9, 1e-6, 1e-9, 4, 10,
                                            10, d, d, d, i, i, i) == BAD_ARG
    assert lib.lp_mip_bounded_fits(2, 4, 4) == 1   # (the third entry takes no context: a host predicate)
