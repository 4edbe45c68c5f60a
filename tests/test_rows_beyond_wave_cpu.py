"""The inputs of tests/rowcases.py on the CPU references alone (no GPU): they must put their near-ties across the
lane + 64 k seam of wave 0's ratio registers and depend on eps, or the GPU parity tests of
tests/test_gpu_rows_beyond_wave.py would pass without looking at the seam.  Conditions, not measurements; a seed of
rowcases.py that misses one is replaced by the first of 0..31 that meets it, the condition stays.

  a  Every LP of seam_pairs: the oracle's first pivot leaves at q = p + off at eps = 0 and at p at 1e-12 from the same
     entering column; p < 64 <= q for the offsets 64 and 65 and p // 64 != q // 64 for 63; p < 128 <= q for 127, 128 and
     129 at m = 130; p // 64 != q // 64 for 127 at 128 x 256.
     Every LP of beyond_pairs: the same two first pivots with 64 <= p, so that the answer at eps > 0 lies beyond the
     first register too.
  b  At each tall shape the traces of seam_mixed at eps = 0 and 1e-9 differ on at least 3 LPs, at least 10 pivots of
     the batch at eps = 0 leave from a row >= 64 and, at m = 130, at least one from a row >= 128: for the oracle's traces
     and for devex_ref's, each on its own.
  c  The conditions B, C and D of tests/test_tolerance_entries_cpu.py at the tall shapes, on seam_mixed (eight LPs;
     the counts are those stated there), and for the dual re-solve: at least 2 LPs end with another status or other
     pivot counts at eps = 0 than at 1e-9, and the dual loop runs at eps = 0.

Left out: the warm bounded re-solve at 100 x 150.  Condition B asks for at most 2 cold solves that are not OPTIMAL at
each eps; at eps = 0 both subnormal-pivot LPs end SINGULAR and on every seed of 0..31 at least one more LP does not end
OPTIMAL (test_no_seed_keeps_enough_cold_solves_at_tall).  The cold bounded solve, the bounded MIP and the bounded
parametrics run at that shape; the warm re-solve runs at 130 x 140."""
import numpy as np
import pytest

from oracle import pyoracle as o
from tests import bounded_ref
from tests import devex_ref as D
from tests import resolve_ref
from tests import rowcases as R
from tests import tolcases as T
from tests import tolentries as E

TALL_IDS = [f"{m}x{n}" for m, n in R.TALL_SHAPES]
ALL_SHAPES = R.TALL_SHAPES + (R.BENCH,)


# ---- a ---------------------------------------------------------------------------------------------------------------
def first_pivots(A, b, c, basis):
    """(entering, leaving row) of the oracle's first pivot at eps = 0 and at 1e-12."""
    m, n = A.shape
    return [o.simplex_tableau(A, b, c, basis, True, n - m, eps=e, max_iter=1, trace_cap=1)["trace"][0]
            for e in (0.0, 1e-12)]


def straddles(m, n, off, t0, t12):
    """Condition a for one LP from its two first pivots."""
    (e0, q), (e12, p) = t0, t12
    if e0 != e12 or q - p != off:
        return False
    if off in (127, 128, 129) and m > 128:
        return p < 128 <= q
    if off in (64, 65):
        return p < 64 <= q
    return p // 64 != q // 64


@pytest.mark.parametrize("m,n", ALL_SHAPES, ids=[f"{m}x{n}" for m, n in ALL_SHAPES])
def test_every_seam_pair_straddles_the_seam(m, n):
    A, b, c, basis = R.seam_pairs(m, n)
    cases = R.seam_pair_list(m, n)
    assert len(cases) == len(A) == 2 * len(R.seam_offsets(m, n))
    assert {63, 64, 65} <= {off for off, _ in cases}
    for k, (off, seed) in enumerate(cases):
        t0, t12 = first_pivots(A[k], b[k], c[k], basis[k])
        assert straddles(m, n, off, t0, t12), (off, seed, t0, t12)


@pytest.mark.parametrize("m,n", ALL_SHAPES, ids=[f"{m}x{n}" for m, n in ALL_SHAPES])
def test_every_beyond_pair_lies_beyond_the_first_register(m, n):
    """At eps = 0 the first pivot leaves at q = p + off, at 1e-12 at p, and 64 <= p; the seeds are the first of 0..31
    for which that holds."""
    def beyond(off, seed):
        (e0, q), (e12, p) = first_pivots(*T.near_tie_rows(seed, m, n, off))
        return e0 == e12 and q - p == off and p >= 64

    cases = R.BEYOND[(m, n)]
    assert len(R.beyond_pairs(m, n)[0]) == len(cases) >= 4
    for off in sorted({off for off, _ in cases}):
        seeds = [seed for o_, seed in cases if o_ == off]
        assert [s for s in range(32) if beyond(off, s)][:len(seeds)] == seeds, off
    if m > 128:   # the last pair has p in the second register and q in the third
        off, seed = cases[-1]
        (_, q), (_, p) = first_pivots(*T.near_tie_rows(seed, m, n, off))
        assert 64 <= p < 128 <= q


# ---- b ---------------------------------------------------------------------------------------------------------------
def mixed_traces(m, n, seed, solve):
    A, b, c, basis = R.seam_mixed(m, n, seed)
    return [[solve(A[k], b[k], c[k], basis[k], True, n - m, eps=e, trace_cap=1 << 14)["trace"] for k in range(len(A))]
            for e in (0.0, E.EPS_DEFAULT)]


def mixed_counts(m, n, seed, solve):
    """(LPs whose trace differs between eps = 0 and 1e-9, pivots at eps = 0 leaving from a row >= 64, from >= 128)."""
    t0, t9 = mixed_traces(m, n, seed, solve)
    rows = [r for t in t0 for _, r in t]
    return sum(a != z for a, z in zip(t0, t9)), sum(r >= 64 for r in rows), sum(r >= 128 for r in rows)


@pytest.mark.parametrize("solve", [o.simplex_tableau, D.simplex_tableau], ids=["oracle", "devex"])
@pytest.mark.parametrize("m,n", R.TALL_SHAPES, ids=TALL_IDS)
def test_seam_mixed_depends_on_eps_and_leaves_from_rows_beyond_the_wave(m, n, solve):
    differ, beyond64, beyond128 = mixed_counts(m, n, R.MIXED_SEED[(m, n)], solve)
    assert differ >= 3 and beyond64 >= 10, (differ, beyond64)
    if m > 128:
        assert beyond128 >= 1


# ---- c ---------------------------------------------------------------------------------------------------------------
def _resolve_outcomes(m, n, eps, kind):
    keep, _ = E.resolve_batch(m, n, eps, kind, R.seam_boxed)
    return {k: (r["status"], tuple(r["iters"])) for k, r in zip(keep, E.resolve_ref(m, n, eps, kind, R.seam_boxed))}


@pytest.mark.parametrize("m,n", R.WARM_SHAPES, ids=[f"{m}x{n}" for m, n in R.WARM_SHAPES])
def test_bounded_resolve_depends_on_eps(m, n):
    for eps in R.EPS:
        cold = E.same_eps_start("bounded", m, n, eps, batch=R.seam_boxed)
        assert sum(r["status"] != E.OPTIMAL for r in cold) <= 2, eps
        flips = [it[2] for _, it in _resolve_outcomes(m, n, eps, "cost").values()]
        assert max(flips) > 0, eps
    r0, r9 = (_resolve_outcomes(m, n, e, "bound") for e in (0.0, E.EPS_DEFAULT))
    assert sum(r0.get(k) != r9.get(k) for k in range(len(R.SEAM_NAMES))) >= 2
    assert any(it[0] > 0 for _, it in r0.values())   # the dual loop runs at eps = 0


def test_no_seed_keeps_enough_cold_solves_at_tall():
    """Why the warm bounded re-solve is left out at 100 x 150 (rowcases.BOUNDED_SEED): at eps = 0 more than 2 of the
    cold solves are not OPTIMAL on every seed of 0..31."""
    m, n = R.TALL
    for seed in range(32):
        A, b, c, _ = R.seam_mixed(m, n, seed)
        lo, hi = E.boxes(c.shape, m)
        status = [bounded_ref.bounded(A[k], b[k], c[k], lo[k], hi[k], True, n, eps=0.0)["status"] for k in range(len(A))]
        assert sum(s != E.OPTIMAL for s in status) > 2, seed


def mip_outcomes(m, n, eps, seed):
    return [(root["status"], None if r is None else (r["status"], r["found"], r["stats"]))
            for root, r in E.mip_ref(m, n, eps, seed)]


def mip_depends_on_eps(m, n, seed):
    r0, r9, r2 = (mip_outcomes(m, n, e, seed) for e in (0.0, E.EPS_DEFAULT, 1e-2))
    searched = [r for _, r in r0 if r is not None and r[0] != 5 and r[2][0] > 1]
    return (all(root == E.OPTIMAL for root, _ in r9)
            and sum(a != z for a, z in zip(r2, r9)) >= 3
            and sum(a != z for a, z in zip(r0[:E.MIP_TIES], r9[:E.MIP_TIES])) >= 3
            and len(searched) >= 2
            and sum(r[2][0] > 1 for _, r in r9) >= 5)   # the tie family branches (b + 0.5)


@pytest.mark.parametrize("m,n", R.TALL_SHAPES, ids=TALL_IDS)
def test_bounded_mip_depends_on_eps(m, n):
    assert mip_depends_on_eps(m, n, R.MIP_SEED[(m, n)])


def parametric_depends_on_eps(m, n, seed, which):
    for eps in R.EPS:
        cold = E.same_eps_start("oracle", m, n, eps, seed, R.seam_mixed)
        if not all(r["status"] == E.OPTIMAL for r in cold):
            return False
        if (E.parametric_refs(m, n, eps, which, seed, batch=R.seam_mixed)["nseg"] >= 2).sum() < 3:
            return False
    n0, n9 = (E.parametric_refs(m, n, e, which, seed, batch=R.seam_mixed)["nseg"] for e in (0.0, E.EPS_DEFAULT))
    return (n0 != n9).sum() >= 2


@pytest.mark.parametrize("which", ["rhs", "cost"])
@pytest.mark.parametrize("m,n", R.TALL_SHAPES, ids=TALL_IDS)
def test_parametric_depends_on_eps(m, n, which):
    assert parametric_depends_on_eps(m, n, R.PARAMETRIC_SEED[(m, n)], which)


def dual_resolve_outcomes(m, n, eps, seed):
    keep, (A, b2, c, basis) = R.resolve_start(m, n, eps, seed)
    return {k: (r["status"], r["iters"]) for k, r in
            zip(keep, (resolve_ref.resolve(A[j], b2[j], c[j], basis[j], True, n - m, eps=eps)
                       for j in range(len(keep))))}


def dual_resolve_depends_on_eps(m, n, seed):
    r0, r9 = (dual_resolve_outcomes(m, n, e, seed) for e in (0.0, E.EPS_DEFAULT))
    return (sum(r0.get(k) != r9.get(k) for k in range(len(R.SEAM_NAMES))) >= 2
            and any(it[0] > 0 for _, it in r0.values()))   # the dual loop runs at eps = 0


@pytest.mark.parametrize("m,n", R.TALL_SHAPES, ids=TALL_IDS)
def test_dual_resolve_depends_on_eps(m, n):
    assert dual_resolve_depends_on_eps(m, n, R.RESOLVE_SEED[(m, n)])


def test_inputs_are_deterministic():
    m, n = R.TALL
    for make in (lambda: R.seam_pairs(m, n), lambda: R.seam_mixed(m, n)):
        a = make()
        E._CACHE.clear()
        for x, y in zip(a, make()):
            assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))
