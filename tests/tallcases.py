"""Inputs of the tests of the HBM-tableau selectors beyond row and column 1024 (inputs only, built on tests/tolcases.py
and tests/tolentries.py, in the style of tests/rowcases.py).  Every selector that works on the tableau in HBM scans in
pieces of 1024: wave_chain_select<.., 16> walks tiles of 64 x 16 entries and replays near-ties per tile,
block_chain_select gives thread t the entries t, t + 1024, ... and the Devex pricing of select_bounded_rule takes four
columns per thread and step, 1024 apart, with a second outer step at column 4096.  The families of tolcases.py are
carried across those seams: near-tie pairs (p, q) with p < 1024 <= q (straddle_*) and with 1024 <= p < q (beyond_*: at
eps > 0 a straddling pair's answer is p < 1024, which a replay that reads the first tile alone still finds).
tests/test_tall_seams_cpu.py checks on the references that each input does what its name says,
tests/test_gpu_tall_seams.py runs them on the GPU.

Shapes:
  TALL  1100 x 2300  the smallest shape the project uses past 1024 rows; 1200 original columns
  WIDE    24 x 4300  more columns than one step of the Devex pricing (4 x 1024)

A case is a Case: the LP (A, b, c, lo, hi) in slack form [A_orig | I], maximise, started from the slack basis, with the
intended entering column e and its pinned rows (p, q) or columns (e, e2).  lo = 0 throughout; hi = +inf unless the family
sets a bound.  Forms of a case: boxed (the box recipe of tolentries.boxes around it, hi[e] = +inf), bland_form (the
entering column moved to index 0: Bland's rule enters the smallest eligible index) and cold_form (the entering column
times 4, so that phase I of the cold solve enters it first and every ratio is scaled exactly)."""
import types

import numpy as np

from oracle import pyoracle as o
from simplexmethod_amd import capi
from tests import bounded_rules_ref as RR
from tests import resolve_ref
from tests import tolcases as T
from tests import tolentries as E

SEAM = 1024
TALL, WIDE = (1100, 2300), (24, 4300)
SEED = 11
EPS = E.EPS
PAIR_EPS = (0.0, 1e-12)     # the two eps at which a pinned pair must give q and p
MAX_ITERS = (1, 8)
INF = np.inf
DANTZIG, BLAND, DEVEX = RR.RULES
RULE_NAMES = ("dantzig", "bland", "devex")

# name -> (p, q): rows of the near-tie pair of near_tie_rows.  m - 1 = 1099.
STRADDLE_ROWS = {"straddle_rows@1023": (30, 1053), "straddle_rows@1024": (31, 1055), "straddle_rows@1025": (21, 1046),
                 "straddle_rows@m-1": (500, 1099)}
BEYOND_ROWS = {"beyond_rows@1": (1030, 1031), "beyond_rows@17": (1040, 1057), "beyond_rows@64": (1029, 1093)}
# a near-tie pair inside the first tile and a clear winner behind it in the second: a replay that ends the scan after
# the tile it ran in misses the winner
LATE_ROWS = {"late_rows": (100, 200)}
LATE_WINNER = 1060
# name -> (e, e2): columns of the near-tie pair of near_tie_cols, among the 1200 original columns
STRADDLE_COLS = {"straddle_cols@1023": (3, 1026), "straddle_cols@1024": (25, 1049), "straddle_cols@1025": (170, 1195)}
BEYOND_COLS = {"beyond_cols@1": (1100, 1101), "beyond_cols@17": (1150, 1167)}
# exact copies, cost included.  @1: neighbouring lanes; @64: the same lane of waves 0 and 1 of the Devex pricing (the
# smaller index in the EARLIER wave, so that a combine that prefers the later wave is wrong) and of one tile of the chain;
# @1024: one thread's first and second column of a Devex step, two tiles of the chain; @4096 (WIDE): one thread's two
# outer steps
DUP_COLS = {"dup_cols@1": (40, 41), "dup_cols@64": (40, 104), "dup_cols@1024": (100, 1124)}
DUP_WIDE = {"dup_cols@4096": (50, 4146)}
# name -> (u, (p, q)): the degenerate row q past 1024
TINY = {"tiny5e-324": (5e-324, (40, 1064)), "tiny1e-310": (1e-310, (1030, 1090))}
UPPER_TWIN = {"upper_twin@straddle": "straddle_rows@1024", "upper_twin@beyond": "beyond_rows@64"}
FLIP_BASE = "beyond_rows@1"     # both rows of the pair past 1024: the winner lies there at every eps
FLIP_WHICH = ("below", "equal", "above")
DUAL_POSITIONS = ((20, 1044), (1030, 1031), (1029, 1093))
DUAL_KINDS = ("below_below", "below_above", "above_above")
DUAL_COL_ROW = 1050             # the leaving row of dual_cols
DUAL_COLS = {"dual_cols@1": (40, 41), "dual_cols@64": (40, 104), "dual_cols@1024": (100, 1124),
             "dual_cols@1025": (100, 1125), "dual_cols@beyond1": (1100, 1101), "dual_cols@beyond64": (1130, 1194)}

ROW_PAIRS = {**STRADDLE_ROWS, **BEYOND_ROWS}
COL_PAIRS = {**STRADDLE_COLS, **BEYOND_COLS}


def Case(name, A, b, c, e, rows=None, cols=None, lo=None, hi=None):
    n = A.shape[1]
    return types.SimpleNamespace(name=name, A=A, b=b, c=c, e=e, rows=rows, cols=cols,
                                 lo=np.zeros(n) if lo is None else lo, hi=np.full(n, INF) if hi is None else hi)


def _entering(c, no):
    """The column _force_entering chose: the largest cost."""
    return int(np.argmax(c[:no]))


def _make(name):
    m, n = TALL
    no = n - m
    if name in ROW_PAIRS or name in LATE_ROWS:
        p, q = {**ROW_PAIRS, **LATE_ROWS}[name]
        A, b, c, _ = T.near_tie_rows(SEED, m, n, q - p, pair=(p, q))
        e = _entering(c, no)
        if name in LATE_ROWS:
            b[LATE_WINNER] = 0.5 * (b[q] / A[q, e]) * A[LATE_WINNER, e]
        return Case(name, A, b, c, e, rows=(p, q))
    if name in COL_PAIRS:
        e, e2 = COL_PAIRS[name]
        A, b, c, _ = T.near_tie_cols(SEED, m, n, e2 - e, cols=(e, e2))
        return Case(name, A, b, c, e, cols=(e, e2))
    if name in DUP_COLS or name in DUP_WIDE:
        if name in DUP_WIDE:
            m, n = WIDE
            no = n - m
        e, e2 = {**DUP_COLS, **DUP_WIDE}[name]
        A, b, c, _ = capi.gen_lp(SEED, m, n)
        T._force_entering(A, c, no, e)
        A[:, e2] = A[:, e]
        c[e2] = c[e]
        return Case(name, A, b, c, e, cols=(e, e2))
    if name in TINY:
        u, (p, q) = TINY[name]
        A, b, c, _ = T.tiny_entry(SEED, m, n, u, q - p, pair=(p, q))
        return Case(name, A, b, c, _entering(c, no), rows=(p, q))
    if name in UPPER_TWIN:
        return _upper_twin(name)
    raise KeyError(name)


def case(name):
    """The case `name` of any primal family, built once."""
    return E._memo(("tall_case", name), lambda: _make(name))


PLAIN_NAMES = tuple(ROW_PAIRS) + tuple(LATE_ROWS) + tuple(COL_PAIRS) + tuple(DUP_COLS) + tuple(TINY)   # group A


def slack_basis(A):
    m, n = A.shape
    return np.arange(n - m, n, dtype=np.int32)


# ---- forms -----------------------------------------------------------------------------------------------------------
def boxed(cs):
    """cs inside the box recipe of tolentries.boxes: hi[e] (and hi[e2] of a column pair) stay +inf, so that the first
    iteration is the pivot of the plain case; a bound the family set itself stays."""
    m, n = cs.A.shape
    _, hi = E.boxes(cs.c.shape, m)
    hi[cs.e] = INF
    if cs.cols is not None:
        hi[cs.cols[1]] = INF
    own = np.isfinite(cs.hi)
    hi[own] = cs.hi[own]
    return Case(cs.name + "-boxed", cs.A, cs.b, cs.c, cs.e, cs.rows, cs.cols, cs.lo, hi)


def bland_form(cs):
    """cs with the entering column at index 0 (columns 0 and e exchanged): Bland's rule enters the smallest eligible
    index, and c_e > eps at every eps of the grid."""
    A, c, lo, hi = cs.A.copy(), cs.c.copy(), cs.lo.copy(), cs.hi.copy()
    e = cs.e
    for v in (c, lo, hi):
        v[[0, e]] = v[[e, 0]]
    A[:, [0, e]] = A[:, [e, 0]]
    cols = None if cs.cols is None else (0, cs.cols[1])
    return Case(cs.name + "-bland", A, cs.b, c, 0, cs.rows, cols, lo, hi)


COLD_SCALE = 4.0


def cold_form(cs, rule=DANTZIG):
    """The cold solve's form of a row or dup case: column e (and its copy) times COLD_SCALE, a power of two, so that the
    column sum of e is the largest and phase I enters e first while every ratio is scaled exactly; boxes by
    tolentries.boxes with hi[e] = +inf; for Bland's rule the entering column at index 0."""
    A = cs.A.copy()
    A[:, cs.e] *= COLD_SCALE
    if cs.cols is not None:
        A[:, cs.cols[1]] *= COLD_SCALE
    out = boxed(Case(cs.name + "-cold", A, cs.b, cs.c, cs.e, cs.rows, cs.cols, cs.lo, cs.hi))
    return bland_form(out) if rule == BLAND else out


# ---- references ------------------------------------------------------------------------------------------------------
def ref_resolve(cs, eps, max_iter, rule=DANTZIG):
    """bounded_rules_ref.resolve of cs from the slack basis, once per (case name, eps bits, max_iter, rule)."""
    m, n = cs.A.shape
    return E._memo(("tall_resolve", cs.name, E.eps_key(eps), max_iter, rule),
                   lambda: RR.resolve(cs.A, cs.b, cs.c, cs.lo, cs.hi, *RR.slack_start(cs.A), True, n - m, eps, max_iter,
                                      rule))


def ref_cold(cs, eps, max_iter, rule=DANTZIG):
    """bounded_rules_ref.bounded of cs (a cold form), once per key."""
    m, n = cs.A.shape
    return E._memo(("tall_cold", cs.name, E.eps_key(eps), max_iter, rule),
                   lambda: RR.bounded(cs.A, cs.b, cs.c, cs.lo, cs.hi, True, n - m, eps, max_iter, rule))


def ref_oracle(cs, eps, max_iter, want_tableau=False):
    """The oracle's tableau restatement of cs (hi = +inf) from the slack basis.  With the tableau it is not kept."""
    m, n = cs.A.shape
    assert not np.isfinite(cs.hi).any()

    def run():
        return o.simplex_tableau(cs.A, cs.b, cs.c, slack_basis(cs.A), True, n - m, eps=eps, max_iter=max_iter,
                                 trace_cap=16, want_tableau=want_tableau)
    return run() if want_tableau else E._memo(("tall_oracle", cs.name, E.eps_key(eps), max_iter), run)


def ref_dual(cs, eps, max_iter):
    """resolve_ref.resolve of a dual case with hi = +inf from the slack basis, once per key."""
    m, n = cs.A.shape
    assert not np.isfinite(cs.hi).any()
    return E._memo(("tall_dual", cs.name, E.eps_key(eps), max_iter),
                   lambda: resolve_ref.resolve(cs.A, cs.b, cs.c, slack_basis(cs.A), True, n - m, eps=eps,
                                               max_iter=max_iter))


def changed(r, A):
    """The basis positions that no longer hold their slack."""
    return np.flatnonzero(np.asarray(r["basis"]) != slack_basis(A)).tolist()


def ratio(cs, t):
    return cs.b[t] / cs.A[t, cs.e]


def ulps(x, y):
    """The distance of two doubles of one sign in units of the last place."""
    a, b = (int(np.float64(v).view(np.int64)) for v in (x, y))
    return abs(a - b)


# ---- upper_twin ------------------------------------------------------------------------------------------------------
UPPER_NUDGES = (0, -1, 1, -2, 2, -3, 3, -4, 4, -5, 5, -6, 6, -7, 7, -8, 8)


def _upper_twin(name):
    """The lower/upper pair: the original part of row q of a near-tie row pair negated, b_q = 1 and slack q bounded by
    U = b_q + s * b_p (s * b_p: the twin's old right-hand side), so that row q reaches its UPPER bound at the step at
    which it reached 0.  U is nudged by ulps until, with max_iter = 1, the reference leaves on q at its upper bound at
    eps = 0 and on p at 1e-12; no nudge within +-8 ulp: an error."""
    base = case(UPPER_TWIN[name])
    m, n = base.A.shape
    no = n - m
    p, q = base.rows
    A, b = base.A.copy(), base.b.copy()
    A[q, :no] = -A[q, :no]
    twin_b = b[q]
    b[q] = 1.0
    U0 = 1.0 + twin_b
    for k in UPPER_NUDGES:
        U = U0
        for _ in range(abs(k)):
            U = np.nextafter(U, INF if k > 0 else -INF)
        hi = np.full(n, INF)
        hi[no + q] = U
        cs = Case(name, A, b, base.c, base.e, rows=(p, q), hi=hi)
        r0, r12 = (RR.resolve(A, b, cs.c, cs.lo, hi, *RR.slack_start(A), True, no, eps, 1) for eps in PAIR_EPS)
        if changed(r0, A) == [q] and r0["at_upper"][no + q] == 1 and changed(r12, A) == [p]:
            cs.nudge = k
            return cs
    raise AssertionError(f"{name}: no nudge of U within +-8 ulp")


# ---- flip_edge -------------------------------------------------------------------------------------------------------
def flip_theta(theta_eps):
    """The first ratio of FLIP_BASE under the chain at theta_eps: row q's at eps = 0, row p's at 1e-12 (the near-tie)."""
    base = case(FLIP_BASE)
    p, q = base.rows
    return ratio(base, q if theta_eps == 0.0 else p)


def flip_edge(which, theta_eps=0.0):
    """FLIP_BASE with hi[e] one ulp below theta, at theta or one ulp above it (the bound flip against the pivot,
    ue <= theta), theta the chain's first ratio at theta_eps.  For Bland's rule take bland_form of theta_eps = 0: its
    theta* is the exact minimum, row q's ratio, at every eps."""
    def make():
        base = case(FLIP_BASE)
        theta = flip_theta(theta_eps)
        hi = np.full(base.A.shape[1], INF)
        hi[base.e] = {"below": np.nextafter(theta, -INF), "equal": theta, "above": np.nextafter(theta, INF)}[which]
        return Case(f"flip_{which}@eps{theta_eps!r}", base.A, base.b, base.c, base.e, rows=base.rows, hi=hi)
    return E._memo(("tall_flip", which, E.eps_key(theta_eps)), make)


def flip_boxed(cs):
    """boxed() of a flip case, which would free hi[e]: the bound on e is put back."""
    out = boxed(cs)
    out.hi[cs.e] = cs.hi[cs.e]
    return out


# ---- the dual loop ---------------------------------------------------------------------------------------------------
def _dual_base():
    m, n = TALL
    A, b, c, _ = capi.gen_lp(SEED, m, n)
    c = -np.abs(c)      # dual feasible at the slack basis of a maximisation
    return A, b, c, n - m


def dual_rows(kind, pair):
    """Violation pairs of the dual selector's leaving scan: rows p < q whose violations differ by one ulp, q's the
    larger.  "below": xB = -2 (q: the next double below), the row's original part negated so that it has entering
    candidates (gen_lp's rows are non-negative); "above": the slack bounded by 1 and xB = 3 (q: the next double above),
    the complemented row then has them.  hi = +inf everywhere for below_below: the plain dual re-solve's form."""
    def make():
        A, b, c, no = _dual_base()
        hi = np.full(A.shape[1], INF)
        for t, side, later in zip(pair, kind.split("_"), (False, True)):
            if side == "below":
                A[t, :no] = -A[t, :no]
                b[t] = np.nextafter(-2.0, -INF) if later else -2.0
            else:
                hi[no + t] = 1.0
                b[t] = np.nextafter(3.0, INF) if later else 3.0
        return Case(f"dual_rows-{kind}@{pair[0]},{pair[1]}", A, b, c, None, rows=pair, hi=hi)
    return E._memo(("tall_dual_rows", kind, pair), make)


def dual_cols(name):
    """Quotient twins of the dual selector's entering scan: row DUAL_COL_ROW leaves (xB = -2, negated), column e holds
    the smallest quotient d_e / a_e by a factor of four and column e2 is its copy with the cost a few ulp nearer zero
    (the first of 1..4 ulp at which the quotient is another double; one ulp may round to the same quotient)."""
    def make():
        A, b, c, no = _dual_base()
        r = DUAL_COL_ROW
        e, e2 = DUAL_COLS[name]
        A[:, e] = np.maximum(A[:, e], 0.05)
        A[r, :no] = -A[r, :no]
        b[r] = -2.0
        others = np.delete(np.arange(no), [e, e2])
        with np.errstate(divide="ignore"):
            least = float(np.min(c[others] / A[r, others]))
        c[e] = 0.25 * least * A[r, e]
        A[:, e2] = A[:, e]
        c[e2] = c[e]
        for _ in range(4):
            c[e2] = np.nextafter(c[e2], 0.0)
            if c[e2] / A[r, e2] < c[e] / A[r, e]:
                break
        else:
            raise AssertionError(f"{name}: no cost within 4 ulp gives another quotient")
        return Case(name, A, b, c, e, rows=(r, r), cols=(e, e2))
    return E._memo(("tall_dual_cols", name), make)


def dual_boxed(cs):
    """A dual case inside the box recipe (no entering column to keep free)."""
    m, n = cs.A.shape
    _, hi = E.boxes(cs.c.shape, m)
    own = np.isfinite(cs.hi)
    hi[own] = cs.hi[own]
    return Case(cs.name + "-boxed", cs.A, cs.b, cs.c, cs.e, cs.rows, cs.cols, cs.lo, hi)
