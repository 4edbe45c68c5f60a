"""GPU parity of the HBM-tableau selectors at near-ties beyond row and column 1024.  wave_chain_select walks tiles of
1024 entries, block_chain_select gives thread t the entries t, t + 1024, ..., and the Devex pricing of the bounded
selector takes columns 1024 apart with a second outer step at 4096; the inputs of tests/tallcases.py put ulp near-ties,
exact copies, subnormal pivots and the bounded kernels' own decisions (lower against upper leaving, flip against pivot,
violated below against above) across and wholly beyond those seams, at 1100 x 2300 and 24 x 4300.  Every entry against
the CPU reference of the same entry, bit for bit, at eps 0, 1e-12 and 1e-2 and max_iter 1 and 8.
tests/test_tall_seams_cpu.py checks on the references that each input does what its name says.

  A  the single-LP handle on every algorithm that takes 1100 rows: LAUNCH (wave_chain_select<.., 16> for pricing and
     ratio test), OVERLAP (block_chain_select for both), LOOKAHEAD (wave_chain_select; its selector fits LDS with three
     staged pivots at this shape) and AUTO (which picks LOOKAHEAD here).  Left out: RESIDENT, which needs m <= 960 and
     refuses the shape.  Against the oracle's trace, basis and whole tableau.
  B  lp_simplex_resolve on the dual cases with hi = inf, against resolve_ref.
  C  lp_simplex_bounded_resolve_large_ex from the slack basis under the three rules on every primal family, plain and
     boxed, and under Dantzig's on the dual families; the entry without a rule returns what Dantzig's does; with
     hi = inf it ends on the basis of group A.
  D  lp_simplex_bounded_large_ex on the cold forms and on the copy 4096 columns apart.

Floats are compared by the helpers of tests/test_gpu_tolerance.py and tests/test_gpu_bounded.py."""
import numpy as np
import pytest

from simplexmethod_amd import capi
from tests import bounded_rules_ref as RR
from tests import tallcases as C
from tests.test_gpu_bounded import _same
from tests.test_gpu_tolerance import _assert_same, _same_bits

pytestmark = pytest.mark.gpu

OPTIMAL = 0
DANTZIG, BLAND, DEVEX = RR.RULES
NAME = C.RULE_NAMES
ALGOS = (capi.SIMPLEX_LAUNCH, capi.SIMPLEX_OVERLAP, capi.SIMPLEX_LOOKAHEAD, capi.SIMPLEX_AUTO)
GRID = [(eps, k) for eps in C.EPS for k in C.MAX_ITERS]
rules = pytest.mark.parametrize("rule", RR.RULES, ids=NAME)


def _resolve_large(ctx, cs, eps, max_iter, rule):
    m, n = cs.A.shape
    return ctx.bounded_resolve_large(cs.A, cs.b, cs.c, cs.lo, cs.hi, *RR.slack_start(cs.A), True, n - m, eps=eps,
                                     max_iter=max_iter, pivot_rule=None if rule is None else NAME[rule])


def _large(ctx, cs, eps, max_iter, rule):
    m, n = cs.A.shape
    return ctx.bounded_large(cs.A, cs.b, cs.c, cs.lo, cs.hi, True, n - m, eps=eps, max_iter=max_iter,
                             pivot_rule=None if rule is None else NAME[rule])


# ---- A: the single-LP handle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.PLAIN_NAMES)
def test_single_lp_handle(ctx, name):
    """One upload per case, reset before every run.  The identity anchor of group C rides here, where the oracle's
    result is at hand: with hi = inf the bounded re-solve from the slack basis makes the oracle's pivots."""
    cs = C.case(name)
    m, n = cs.A.shape
    p = ctx.simplex_problem(cs.A, cs.b, cs.c, C.slack_basis(cs.A), True, n - m)
    try:
        for eps, max_iter in GRID:
            r = C.ref_oracle(cs, eps, max_iter, want_tableau=True)
            for algo in ALGOS:
                p.reset()
                rc, st = p.run(eps=eps, max_iter=max_iter, algo=algo)
                g = p.download(trace_cap=max(st.pivots, 1), want_tableau=True)
                g.update(status=rc, iters=st.pivots)
                assert st.fell_back == 0, (name, eps, max_iter, algo)
                if algo != capi.SIMPLEX_AUTO:
                    assert st.algo_used == algo, (st.algo_used, algo)
                _assert_same(g, r, (name, eps, max_iter, algo))
            b = _resolve_large(ctx, cs, eps, max_iter, None)
            what = (name, eps, max_iter, "anchor")
            assert b["status"] == r["status"] and b["iters"] == [0, r["iters"], 0], what
            assert np.array_equal(b["basis"], r["basis"]) and not np.any(b["at_upper"]), what
            if r["status"] == OPTIMAL:
                assert _same_bits(b["x"], r["x"]) and _same_bits(b["obj"], r["obj"]), what
    finally:
        p.free()


def test_the_algorithms_of_group_a(ctx):
    """Which algorithms take 1100 x 2300: the chip-resident kernel refuses it (m > 960), AUTO picks the look-ahead."""
    cs = C.case("beyond_rows@1")
    m, n = cs.A.shape
    p = ctx.simplex_problem(cs.A, cs.b, cs.c, C.slack_basis(cs.A), True, n - m)
    try:
        with pytest.raises(capi.LPError) as e:
            p.run(eps=0.0, max_iter=1, algo=capi.SIMPLEX_RESIDENT)
        assert e.value.code == capi.BAD_ARG
        p.reset()
        _, st = p.run(eps=0.0, max_iter=1, algo=capi.SIMPLEX_AUTO)
        assert st.algo_used == capi.SIMPLEX_LOOKAHEAD and st.fell_back == 0
    finally:
        p.free()


# ---- B: the plain dual re-solve ----------------------------------------------------------------------------------------
def _dual_ids():
    return [f"{kind}@{p},{q}" for kind in C.DUAL_KINDS for p, q in C.DUAL_POSITIONS] + list(C.DUAL_COLS)


def _dual_case(ident):
    if ident in C.DUAL_COLS:
        return C.dual_cols(ident), True
    kind, pos = ident.split("@")
    return C.dual_rows(kind, tuple(int(v) for v in pos.split(","))), kind == "below_below"


@pytest.mark.parametrize("ident", [i for i in _dual_ids() if i in C.DUAL_COLS or i.startswith("below_below")])
def test_plain_dual_resolve(ctx, ident):
    cs, plain = _dual_case(ident)
    assert plain
    m, n = cs.A.shape
    for eps, max_iter in GRID:
        what = (ident, eps, max_iter)
        r = C.ref_dual(cs, eps, max_iter)
        g = ctx.simplex_resolve(cs.A, cs.b, cs.c, C.slack_basis(cs.A), True, n - m, eps=eps, max_iter=max_iter)
        assert g["status"] == r["status"] and g["iters"] == r["iters"], what
        assert np.array_equal(g["basis"], r["basis"]), what
        if r["status"] == OPTIMAL:
            assert _same_bits(g["x"], r["x"]) and _same_bits(g["obj"], r["obj"]), what


# ---- C: the bounded re-solve from the slack basis ----------------------------------------------------------------------
def _flip_ids():
    return [f"flip_{which}@{eps!r}" for eps in C.PAIR_EPS for which in C.FLIP_WHICH]


def _primal_forms(name, rule):
    """The plain and the boxed form of a primal case; under Bland's rule with the entering column at index 0."""
    if name.startswith("flip_"):
        which, eps = name[5:].split("@")
        cs = C.flip_edge(which, float(eps))
        forms = (cs, C.flip_boxed(cs))
    else:
        cs = C.case(name)
        forms = (cs, C.boxed(cs))
    return [C.bland_form(f) for f in forms] if rule == BLAND else forms


PRIMAL_NAMES = C.PLAIN_NAMES + tuple(C.DUP_WIDE) + tuple(C.UPPER_TWIN) + tuple(_flip_ids())


@rules
@pytest.mark.parametrize("name", PRIMAL_NAMES)
def test_bounded_resolve_large_primal(ctx, name, rule):
    for cs in _primal_forms(name, rule):
        for eps, max_iter in GRID:
            r = C.ref_resolve(cs, eps, max_iter, rule)
            g = _resolve_large(ctx, cs, eps, max_iter, rule)
            _same(g, r)
            if rule == DANTZIG:   # the entry without a rule
                _same(_resolve_large(ctx, cs, eps, max_iter, None), g)


@pytest.mark.parametrize("ident", _dual_ids())
def test_bounded_resolve_large_dual(ctx, ident):
    """The dual branch (the rule governs the primal branch only): Dantzig's _ex call and the entry without a rule."""
    cs, _ = _dual_case(ident)
    for form in (cs, C.dual_boxed(cs)):
        for eps, max_iter in GRID:
            r = C.ref_resolve(form, eps, max_iter)
            g = _resolve_large(ctx, form, eps, max_iter, DANTZIG)
            _same(g, r)
            _same(_resolve_large(ctx, form, eps, max_iter, None), g)


# ---- D: the cold solve -------------------------------------------------------------------------------------------------
@rules
@pytest.mark.parametrize("name", tuple(C.ROW_PAIRS) + tuple(C.DUP_COLS) + tuple(C.DUP_WIDE))
def test_bounded_large_cold(ctx, name, rule):
    cs = C.cold_form(C.case(name), rule)
    for eps, max_iter in GRID:
        r = C.ref_cold(cs, eps, max_iter, rule)
        g = _large(ctx, cs, eps, max_iter, rule)
        _same(g, r)
        if rule == DANTZIG:
            _same(_large(ctx, cs, eps, max_iter, None), g)
