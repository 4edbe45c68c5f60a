"""GPU parity of the one-LP-per-workgroup kernels on rows 64 and beyond, at near-ties: wave 0 holds the ratios of rows
lane, lane + 64, lane + 128, lane + 192 in registers, and the inputs of tests/rowcases.py put ulp near-ties, exact
ties and subnormal pivots across that seam (100 x 150: the second register live; 130 x 140: the third; 128 x 256: the
benchmark's shape).  Every entry against its CPU reference bit for bit, at eps 0, 1e-12 and 1e-2.
tests/test_rows_beyond_wave_cpu.py checks on the references that the inputs straddle the seam and depend on eps.

Floats are compared by their bits, except NaNs: those must sit at the same positions.  Every batched test asserts that
it ran one LP per workgroup and not the per-LP fallback: path() == 1 on the handle form where the entry has one, the
entry's own *_fits predicate (beyond which the entry refuses the shape) elsewhere.  The bodies shared with the shapes
of m <= 64 are the check_* helpers of tests/test_gpu_tolerance_entries.py."""
import numpy as np
import pytest

from tests import bounded_parametric_ref, bounded_rules_ref, mip_ref, parametric_cost_ref, parametric_ref, resolve_ref
from tests import bounded_resolve_ref as W
from tests import rowcases as R
from tests import test_gpu_tolerance_entries as G
from tests import tolentries as E
from tests.test_gpu_tolerance import _assert_lp, _same_bits

pytestmark = pytest.mark.gpu

OPTIMAL = 0
RULES = ("dantzig", "bland", "devex")


def _cases(shapes):
    return [(m, n, eps) for m, n in shapes for eps in R.EPS]


def _ids(cases):
    return [f"{m}x{n}-eps{eps!r}" for m, n, eps in cases]


ALL = _cases(R.TALL_SHAPES + (R.BENCH,))
TALL = _cases(R.TALL_SHAPES)
WARM = _cases(R.WARM_SHAPES)


def _pair_names(m, n):
    return [f"pair@{off}-seed{seed}" for off, seed in R.seam_pair_list(m, n)]


def _beyond_names(m, n):
    return [f"beyond@{off}-seed{seed}" for off, seed in R.BEYOND[(m, n)]]


# ---- A: the plain batched simplex ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("case", ALL, ids=_ids(ALL))
def test_plain_batched(ctx, case, rule):
    """simplex_solve_batched and the batched_problem handle on seam_pairs, beyond_pairs and seam_mixed.  By lp_batched_launch's
    choice all three shapes run the register-resident rows under Dantzig's rule (100 x 150: 1024 threads, 12 rows per
    thread; 130 x 140: 1024 threads, 4 rows; 128 x 256: 512 threads, 44 rows), whose ratio test is
    wave_ratio_select<2> for m <= 128 and <4> up to 256; under Bland's and the Devex rule they run the LDS tableau
    (wave_bland_ratio; wave_ratio_select<4> at every m <= 256).  These are three of the four register forms: the
    fourth (1024 threads, 20 rows), the layouts and the ratio scan beyond m = 256 of all of them are
    tests/test_gpu_batched_forms.py's."""
    m, n, eps = case
    G.check_batched(ctx, m, n, eps, R.seam_pairs, _pair_names(m, n), rule)
    G.check_batched(ctx, m, n, eps, R.beyond_pairs, _beyond_names(m, n), rule)
    G.check_batched(ctx, m, n, eps, R.seam_mixed, R.SEAM_NAMES, rule)


# ---- B: the batched two-phase --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("case", TALL, ids=_ids(TALL))
def test_two_phase_batched(ctx, case, rule):
    m, n, eps = case
    G.check_two_phase(ctx, m, n, eps, R.seam_mixed, R.SEAM_NAMES, rule, single=False)


# ---- C: the bounded simplex, cold and warm -------------------------------------------------------------------------------
def _lp_of(out, k):
    return {key: v[k] for key, v in out.items()}


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("case", TALL, ids=_ids(TALL))
def test_bounded_cold(ctx, case, rule):
    """bounded_batched on seam_mixed and on beyond_pairs with the box recipe under each rule, and the single-LP entry
    on the first and the last LP, against bounded_rules_ref."""
    m, n, eps = case
    assert ctx.bounded_rule_fits(m, n, rule)
    for batch, names in ((R.seam_boxed, R.SEAM_NAMES), (R.beyond_pairs, _beyond_names(m, n))):
        A, b, c, lo, hi = E.bounded_lps(m, n, batch)
        g = ctx.bounded_batched(A, b, c, lo, hi, True, n - m, eps=eps, pivot_rule=rule)
        for k in range(len(A)):
            what = (names[k], eps, rule)
            r = G._ref(("bounded_cold", batch.__name__, rule, m, n, k), eps,
                       lambda: bounded_rules_ref.bounded(A[k], b[k], c[k], lo[k], hi[k], True, n - m, eps=eps,
                                                         rule=RULES.index(rule)))
            G._assert_bounded(_lp_of(g, k), r, what)
            if k in (0, len(A) - 1):
                one = ctx.bounded(A[k], b[k], c[k], lo[k], hi[k], True, n - m, eps=eps, pivot_rule=rule)
                G._assert_bounded(one, r, what)


@pytest.mark.parametrize("kind", W.PERTURBATIONS)
@pytest.mark.parametrize("case", WARM, ids=_ids(WARM))
def test_bounded_resolve(ctx, case, kind):
    """bounded_resolve_batched from the cold reference's bases at the same eps, and the single-LP entry on the first
    and the last kept LP.  (100 x 150 is left out: rowcases.BOUNDED_SEED.)"""
    m, n, eps = case
    G.check_bounded_resolve(ctx, m, n, eps, kind, R.seam_boxed, R.SEAM_NAMES, single=(0, -1))


# ---- D: branch and bound -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", TALL, ids=_ids(TALL))
def test_mip_bounded(ctx, case):
    m, n, eps = case
    G.check_mip_bounded(ctx, m, n, eps, R.MIP_SEED[(m, n)])


@pytest.mark.parametrize("eps", R.EPS)
def test_mip_unbounded(ctx, eps):
    """mip_batched on the LPs of boxed_mip_ties without their boxes, from the slack basis.  100 x 150 alone: mip_fits
    does not hold at 130 x 140 under MIP_LIMITS, and the entry has no other path."""
    m, n = R.TALL
    depth = E.MIP_LIMITS["max_depth"]
    assert ctx.mip_fits(m, n, depth) and not ctx.mip_fits(*R.TALLEST, depth)
    A, b, c, _, _, mask = E.boxed_mip_ties(m, n, R.MIP_SEED[(m, n)])
    slack = np.tile(np.arange(n - m, n, dtype=np.int32), (len(A), 1))
    g = ctx.mip_batched(A, b, c, slack, mask, True, n - m, eps=eps, **E.MIP_LIMITS)
    for k in range(len(A)):
        r = G._ref(("mip_unbounded", m, n, k), eps,
                   lambda: mip_ref.mip(A[k], b[k], c[k], slack[k], mask, True, n - m, eps=eps, **E.MIP_LIMITS))
        assert g["status"][k] == r["status"] and g["found"][k] == r["found"], (k, eps)
        assert tuple(g["stats"][k].tolist()) == r["stats"], (k, eps)
        assert _same_bits(g["x"][k], r["x"]) and _same_bits(g["obj"][k], r["obj"]), (k, eps)
        assert _same_bits(g["bound"][k], r["bound"]), (k, eps)


# ---- E: the parametric analyses ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["rhs", "cost"])
@pytest.mark.parametrize("case", TALL, ids=_ids(TALL))
def test_parametric(ctx, case, which):
    """The batched entry and the handle form after a batched run."""
    m, n, eps = case
    G.check_parametric(ctx, m, n, eps, which, R.PARAMETRIC_SEED[(m, n)], R.seam_mixed, R.SEAM_NAMES, single=False)


def _bounded_parametric_inputs(m, n, eps):
    """seam_mixed with the box recipe at the cold reference's vertices at `eps`: (A, b, c, lo, hi, basis, at_upper),
    the directions d and g of tolentries.parametric_inputs and the cold statuses.  An LP that did not reach an optimum
    gets basis 0 (its own may hold artificials) and keeps its status."""
    def make():
        A, b, c, lo, hi = E.bounded_lps(m, n, R.seam_boxed)
        cold = E.same_eps_start("bounded", m, n, eps, batch=R.seam_boxed)
        status = np.array([r["status"] for r in cold], np.int32)
        basis = np.stack([r["basis"] if r["status"] == OPTIMAL else np.zeros(m, np.int32) for r in cold])
        up = np.stack([r["at_upper"] for r in cold])
        d = np.stack([parametric_ref.direction(1, bk) for bk in b])
        g = np.stack([parametric_cost_ref.direction(1, ck) for ck in c])
        return (A, b, c, lo, hi, basis, up), d, g, status
    return G._ref(("bounded_parametric_inputs", m, n), eps, make)


@pytest.mark.parametrize("which", ["rhs", "cost"])
@pytest.mark.parametrize("case", TALL, ids=_ids(TALL))
def test_bounded_parametric(ctx, case, which):
    """bounded_parametric_batched and bounded_parametric_cost_batched, chained after the cold solve by run_status."""
    m, n, eps = case
    fits, entry = {"rhs": (ctx.bounded_parametric_fits, ctx.bounded_parametric_batched),
                   "cost": (ctx.bounded_parametric_cost_fits, ctx.bounded_parametric_cost_batched)}[which]
    assert fits(m, n)
    at, d, g_, status = _bounded_parametric_inputs(m, n, eps)
    direction = d if which == "rhs" else g_
    want = G._ref(("bounded_parametric", which, m, n), eps,
                  lambda: bounded_parametric_ref.parametric_batched(which, *at, direction, np.inf, True, eps,
                                                                    E.MAX_BREAKS, status))
    got = entry(*at, direction, np.inf, True, eps=eps, max_breaks=E.MAX_BREAKS, run_status=status)
    assert (want["nseg"] >= 1).sum() >= 2
    for k in range(len(status)):
        what = (R.SEAM_NAMES[k], eps, which)
        for key, w in want.items():
            if w.dtype.kind == "f":
                assert _same_bits(got[key][k], w[k]), (what, key)
            else:
                assert np.array_equal(got[key][k], w[k]), (what, key)


# ---- F: the dual re-solve ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", TALL, ids=_ids(TALL))
def test_dual_resolve(ctx, case):
    """resolve_batched from the oracle's optimal bases at the same eps after a change of the right-hand side."""
    m, n, eps = case
    keep, (A, b2, c, basis) = R.resolve_start(m, n, eps)
    assert len(keep) >= len(R.SEAM_NAMES) - 2
    p = ctx.batched_resolve_problem(A, b2, c, basis, True, n - m)
    try:
        assert p.path() == 1
    finally:
        p.free()
    gb = ctx.resolve_batched(A, b2, c, basis, True, n - m, eps=eps)
    for j, k in enumerate(keep):
        what = (R.SEAM_NAMES[k], eps)
        r = G._ref(("dual_resolve", m, n, k), eps,
                   lambda: resolve_ref.resolve(A[j], b2[j], c[j], basis[j], True, n - m, eps=eps))
        assert tuple(gb["iters"][j].tolist()) == r["iters"], what
        _assert_lp(gb, j, r, what)
