"""CPU-only checks of Devex pricing: the test restatement (tests/ref/devex_ref.c) equals bland_ref.c bit for
bit in Dantzig mode; under Devex it reaches the optimum scipy's HiGHS and Dantzig's rule reach, keeps every
weight >= 1 and takes at most half of Dantzig's pivots on the badly scaled family; the C ABI refuses null
handles without a device and answers lp_batched_devex_fits from the documented carve."""
import numpy as np
import pytest
from scipy.optimize import linprog

from oracle import pyoracle as o
from simplexmethod_amd import capi
from tests import bland_ref as B
from tests import devex_ref as R
from tests import lpcases

REL = 1e-9


def _close(a, b):
    return abs(a - b) <= REL * max(abs(a), abs(b))


def _highs(A, b, c, maximize):
    r = linprog(-c if maximize else c, A_eq=A, b_eq=b, bounds=(0, None), method="highs")
    assert r.status == 0, r.message
    return -r.fun if maximize else r.fun


def _seeded_lps():
    cases = []
    for seed in range(50):
        m = 2 + seed % 17
        n = 2 * m + seed % 5
        if seed % 3 == 0:
            A, b, c, basis = lpcases.general_lp(seed, m, n)
            cases.append((A, b, c, basis, bool(seed % 2), A.shape[1]))
        else:
            A, b, c, basis = lpcases.random_lp(seed, m, n)
            cases.append((A, b, c, basis, True, n - m))
    return cases


def _min_lps():
    return [lpcases.min_lp(s, m, k, equalities=e, negative_rows=nr, zero_rhs=z)
            for s, (m, k, e, nr, z) in enumerate([(5, 4, 0, 0, 0), (8, 6, 1, 2, 1), (12, 10, 2, 0, 2), (16, 24, 0, 3, 0),
                                                  (32, 40, 3, 2, 2), (24, 30, 4, 0, 0), (24, 30, 0, 5, 0),
                                                  (24, 30, 0, 0, 3)])]


def test_rule0_equals_bland_ref_rule0():
    for A, b, c, basis, mx, no in _seeded_lps():
        q = B.simplex_tableau(A, b, c, basis, mx, no, rule=B.DANTZIG, trace_cap=1 << 14, want_tableau=True)
        r = R.simplex_tableau(A, b, c, basis, mx, no, rule=R.DANTZIG, trace_cap=1 << 14, want_tableau=True)
        assert r["status"] == q["status"] and r["iters"] == q["iters"] and r["trace"] == q["trace"]
        assert np.array_equal(r["basis"], q["basis"]) and np.array_equal(r["tableau"], q["tableau"])
        if q["status"] == o.OPTIMAL:
            assert np.array_equal(r["x"], q["x"]) and r["obj"] == q["obj"]
        assert np.array_equal(r["weights"], np.ones(A.shape[1]))
    for A, b, c, no in _min_lps() + [lpcases.degenerate_eq_lp(s) for s in range(3)]:
        for mx in (False, True):
            q = B.two_phase(A, b, c, mx, no, rule=B.DANTZIG)
            r = R.two_phase(A, b, c, mx, no, rule=R.DANTZIG)
            assert r["status"] == q["status"] and r["iters"] == q["iters"]
            assert np.array_equal(r["basis"], q["basis"])
            if q["status"] == o.OPTIMAL:
                assert np.array_equal(r["x"], q["x"]) and r["obj"] == q["obj"]


def test_refuses_other_rules():
    A, b, c, basis = lpcases.random_lp(0, 4, 9)
    assert R.simplex_tableau(A, b, c, basis, True, 5, rule=1)["status"] == o.BAD_ARG
    assert R.two_phase(A, b, c, True, 5, rule=3)["status"] == o.BAD_ARG


@pytest.mark.parametrize("gen", ["plain", "scaled"])
@pytest.mark.parametrize("m,n", [(3, 8), (12, 24), (32, 96), (64, 192), (128, 256)])
def test_single_phase_optimum(gen, m, n):
    for seed in range(3):
        A, b, c, basis = capi.gen_lp(seed, m, n) if gen == "plain" else R.scaled_lp(seed, m, n)
        no = n - m
        d = R.simplex_tableau(A, b, c, basis, True, no, rule=R.DANTZIG)
        x = R.simplex_tableau(A, b, c, basis, True, no, rule=R.DEVEX, trace_cap=1 << 14)
        assert d["status"] == x["status"] == o.OPTIMAL
        assert _close(x["obj"], d["obj"]) and _close(x["obj"], _highs(A, b, c, True))
        assert len(x["trace"]) == x["iters"] and all(0 <= e < n and 0 <= r < m for e, r in x["trace"])


def test_minimise_sense():
    for seed in range(4):
        A, b, c, basis = R.scaled_lp(seed, 16, 40)
        c = -c   # min -c.x over the same polytope
        d = R.simplex_tableau(A, b, c, basis, False, 24, rule=R.DANTZIG)
        x = R.simplex_tableau(A, b, c, basis, False, 24, rule=R.DEVEX)
        assert d["status"] == x["status"] == o.OPTIMAL
        assert _close(x["obj"], d["obj"]) and _close(x["obj"], _highs(A, b, c, False))


def test_two_phase_optimum():
    cases = _min_lps() + [R.scaled_min_lp(s, 16, 24, negative_rows=s % 3, zero_rhs=s % 2) for s in range(4)]
    for A, b, c, no in cases:
        d = R.two_phase(A, b, c, False, no, rule=R.DANTZIG)
        x = R.two_phase(A, b, c, False, no, rule=R.DEVEX)
        assert d["status"] == x["status"] == o.OPTIMAL
        assert _close(x["obj"], d["obj"]) and _close(x["obj"], _highs(A, b, c, False))
    for s in range(3):   # the drive-out runs between the two weighted phases
        A, b, c, no = lpcases.degenerate_eq_lp(s)
        d = R.two_phase(A, b, c, False, no, rule=R.DANTZIG)
        x = R.two_phase(A, b, c, False, no, rule=R.DEVEX)
        assert d["status"] == x["status"]
        if d["status"] == o.OPTIMAL:
            assert _close(x["obj"], d["obj"])


def test_two_phase_infeasible():
    A = np.array([[1.0, 1.0, 1.0, 0.0], [1.0, 1.0, 0.0, -1.0]])   # x1 + x2 <= 1 and x1 + x2 >= 2
    b = np.array([1.0, 2.0])
    c = np.array([1.0, 1.0, 0.0, 0.0])
    assert R.two_phase(A, b, c, False, 2, rule=R.DEVEX)["status"] == o.INFEASIBLE
    assert R.two_phase(A, b, c, False, 2, rule=R.DANTZIG)["status"] == o.INFEASIBLE


def test_unbounded_and_iteration_limit():
    A, b, c, basis = R.scaled_lp(3, 32, 96)
    full = R.simplex_tableau(A, b, c, basis, True, 64, rule=R.DEVEX, trace_cap=1 << 14)
    assert full["status"] == o.OPTIMAL and full["iters"] > 5
    cut = R.simplex_tableau(A, b, c, basis, True, 64, rule=R.DEVEX, max_iter=5, trace_cap=1 << 14)
    assert cut["status"] == o.ITER_LIMIT and cut["iters"] == 5 and cut["trace"] == full["trace"][:5]
    assert R.simplex_tableau(A, b, c, basis, True, 64, rule=R.DEVEX, max_iter=0)["status"] == o.ITER_LIMIT
    Au = A * np.where(np.arange(96) < 64, -1.0, 1.0)   # every original column non-positive: a ray from the start
    u = R.simplex_tableau(Au, b, c, basis, True, 64, rule=R.DEVEX)
    assert u["status"] == o.UNBOUNDED and u["iters"] == 0


def test_weights_stay_at_least_one_after_every_pivot():
    for gen in (capi.gen_lp, R.scaled_lp):
        A, b, c, basis = gen(1, 24, 64)
        full = R.simplex_tableau(A, b, c, basis, True, 40, rule=R.DEVEX)
        assert full["status"] == o.OPTIMAL
        grew = False
        for k in range(1, full["iters"] + 1):   # the run cut after k pivots is a prefix of the full run
            w = R.simplex_tableau(A, b, c, basis, True, 40, rule=R.DEVEX, max_iter=k)["weights"]
            assert np.all(w >= 1.0) and not np.any(np.isnan(w))
            grew = grew or bool(np.any(w > 1.0))
        assert grew
        assert np.array_equal(R.simplex_tableau(A, b, c, basis, True, 40, rule=R.DEVEX, max_iter=0)["weights"], np.ones(64))


def test_beale():
    """Devex is no anti-cycling rule; on Beale's LP (Dantzig's rule cycles) this restatement happens to reach
    the optimum in 3 pivots.  Recorded from the reference, as the numpy restatement of the rule gave it."""
    A, b, c, basis, no = B.beale()
    assert R.simplex_tableau(A, b, c, basis, True, no, rule=R.DANTZIG)["status"] == o.ITER_LIMIT
    x = R.simplex_tableau(A, b, c, basis, True, no, rule=R.DEVEX, trace_cap=16)
    assert x["status"] == o.OPTIMAL and x["iters"] == 3 and x["trace"] == [(0, 0), (2, 1), (4, 2)]
    assert x["obj"] == 1.0


@pytest.mark.parametrize("m,n", [(128, 256), (256, 512)])
def test_pivot_count_on_scaled_family(m, n):
    dantzig = devex = 0
    for seed in range(6):
        A, b, c, basis = R.scaled_lp(seed, m, n)
        d = R.simplex_tableau(A, b, c, basis, True, n - m, rule=R.DANTZIG)
        x = R.simplex_tableau(A, b, c, basis, True, n - m, rule=R.DEVEX)
        assert d["status"] == x["status"] == o.OPTIMAL and _close(x["obj"], d["obj"])
        dantzig += d["iters"]
        devex += x["iters"]
    print(f"{m}x{n}: Dantzig {dantzig} pivots, Devex {devex} ({devex / dantzig:.3f})")
    assert devex <= 0.5 * dantzig


def test_null_handles_and_names():
    lib = capi.load()
    assert capi.PIVOT_DEVEX == 2
    assert lib.lp_simplex_set_pivot_rule(None, capi.PIVOT_DEVEX) == capi.BAD_ARG
    assert lib.lp_batched_set_pivot_rule(None, capi.PIVOT_DEVEX) == capi.BAD_ARG
    assert capi.pivot_rule_id("devex") == capi.PIVOT_DEVEX and capi.pivot_rule_id("Devex") == 2


def _plain_bytes(m, n):
    """The LDS form's documented carve under Devex: 16 bytes of hand-over words, the (m+1) x pitch
    tableau (pitch = n-m+1 made odd), the pivot row (n-m+1), the eta column (m+1), the ratios (m), 2n ints, then the
    n-m weights; rounded up to 16 before and after the weights."""
    nn = n - m
    W = nn + 1
    pitch = W if W & 1 else W + 1
    base = 8 * (2 + (m + 1) * pitch + W + (m + 1) + m) + 4 * 2 * n
    return (((base + 15) & ~15) + 8 * nn + 15) & ~15


def _two_phase_bytes(m, n):
    """The two-phase carve under Devex: hand-over words, the (m+1) x pitch tableau (pitch = n+1 made odd), the pivot
    row (n+1), the eta column (m+1), n+m ints, rounded up to 16, then the n weights rounded up to 16."""
    W = n + 1
    pitch = W if W & 1 else W + 1
    base = 8 * (2 + (m + 1) * pitch + W + (m + 1)) + 4 * (n + m)
    return ((base + 15) & ~15) + ((8 * n + 15) & ~15)


@pytest.mark.parametrize("two_phase", [0, 1])
def test_batched_devex_fits(two_phase):
    lib = capi.load()
    size = _two_phase_bytes if two_phase else _plain_bytes
    assert lib.lp_batched_devex_fits(128, 256, 0) == 1 and lib.lp_batched_devex_fits(64, 192, 1) == 1
    assert lib.lp_batched_devex_fits(0, 4, two_phase) == 0 and lib.lp_batched_devex_fits(8, 4, two_phase) == 0
    for m in (16, 64, 128):
        fits = [lib.lp_batched_devex_fits(m, n, two_phase) for n in range(m + 1, m + 1200)]
        assert fits[0] == 1 and fits[-1] == 0
        assert fits == sorted(fits, reverse=True)   # monotone in n
        last = m + 1 + fits.index(0) - 1           # the widest shape that fits
        assert size(m, last) <= 160 * 1024 < size(m, last + 1)
    for n in (200, 400):
        fits = [lib.lp_batched_devex_fits(m, n, 1) for m in range(1, n + 1)]
        assert fits == sorted(fits, reverse=True)   # two-phase: monotone in m at fixed n
