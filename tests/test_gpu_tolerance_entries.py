"""GPU parity across the tolerance eps for the entries added after tests/test_gpu_tolerance.py: Devex pricing (launch
path, batched LDS form, two-phase, batched two-phase), the bounded-variable re-solve, branch-and-bound over bounds, the
parametric right-hand side and the parametric cost, each against its CPU reference bit for bit, at eps 0, 1e-12 and
1e-2 on a four-wave shape (16 x 48, there also -0.0 and +inf) and a sixteen-wave shape (64 x 160), on the inputs of
tests/tolentries.py.  tests/test_tolerance_entries_cpu.py checks on the references that these inputs depend on eps.

Floats are compared by their bits (-0.0 is not +0.0), except NaNs: those must sit at the same positions, but their
payloads differ between the host and the device.  The binding does not expose the Devex weights; the trace, the
final tableau and the vertex pin them."""
import numpy as np
import pytest

from oracle import pyoracle as o
from simplexmethod_amd import capi
from tests import bland_ref, bounded_ref, lpcases, mip_bounded_ref, parametric_cost_ref, parametric_ref
from tests import bounded_resolve_ref as W
from tests import devex_ref as D
from tests import tolentries as E
from tests.test_gpu_tolerance import _assert_lp, _assert_same, _bad_arg, _same_bits

pytestmark = pytest.mark.gpu

OPTIMAL, UNBOUNDED, ITER_LIMIT, SINGULAR, INFEASIBLE, BAD_ARG = range(6)
BATCH = len(E.PICKS)
CASES = [(m, n, eps) for m, n in E.SHAPES for eps in E.eps_grid((m, n))]


def _id(case):
    m, n, eps = case
    return f"{m}x{n}-eps{eps!r}"


IDS = [_id(cs) for cs in CASES]
_REF = {}


def _ref(key, eps, make):
    """A reference result, once per (case, eps bits)."""
    k = (key, E.eps_key(eps))
    if k not in _REF:
        _REF[k] = make()
    return _REF[k]


# ---- A: Devex ---------------------------------------------------------------------------------------------------------
def _run_devex(ctx, A, b, c, basis, eps, algo):
    m, n = A.shape
    p = ctx.simplex_problem(A, b, c, basis, True, n - m)
    try:
        p.set_pivot_rule("devex")
        rc, st = p.run(eps=eps, algo=algo)
        out = p.download(trace_cap=max(st.pivots, 1), want_tableau=True)
    finally:
        p.free()
    assert st.fell_back == 0 and st.algo_used == capi.SIMPLEX_LAUNCH, (st.algo_used, algo)
    out.update(status=rc, iters=st.pivots)
    return out


def _devex_ref(key, A, b, c, basis, eps):
    m, n = A.shape
    return _ref(("devex",) + key, eps, lambda: D.simplex_tableau(A, b, c, basis, True, n - m, eps=eps,
                                                                 trace_cap=1 << 14, want_tableau=True))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_devex_single_lp_launch_and_auto(ctx, case):
    m, n, eps = case
    A, b, c, basis = E.mixed(m, n)
    for k in range(BATCH):
        r = _devex_ref((m, n, k), A[k], b[k], c[k], basis[k], eps)
        for algo in (capi.SIMPLEX_LAUNCH, capi.SIMPLEX_AUTO):
            _assert_same(_run_devex(ctx, A[k], b[k], c[k], basis[k], eps, algo), r, (E.NAMES[k], eps, algo))


def _batch_key(batch, m, n, k):
    """The memo key of LP k of batch(m, n); E.mixed keeps the key it always had (shared with the single-LP test)."""
    return (m, n, k) if batch is E.mixed else (batch.__name__, m, n, k)


def _rule_ref(rule, batch, m, n, k, A, b, c, basis, eps):
    """The reference of the plain simplex from a basis under `rule`, once per (rule, LP, eps bits)."""
    if rule == "devex":
        return _devex_ref(_batch_key(batch, m, n, k), A, b, c, basis, eps)
    if rule == "bland":
        return _ref(("bland",) + _batch_key(batch, m, n, k), eps,
                    lambda: bland_ref.simplex_tableau(A, b, c, basis, True, n - m, rule=bland_ref.BLAND, eps=eps))
    return _ref(("dantzig",) + _batch_key(batch, m, n, k), eps,
                lambda: o.simplex_tableau(A, b, c, basis, True, n - m, eps=eps))


def check_batched(ctx, m, n, eps, batch=E.mixed, names=E.NAMES, rule="devex"):
    """simplex_solve_batched and the batched_problem handle on batch(m, n) under `rule`, on the one-LP-per-workgroup
    kernel, against the rule's reference: status, iters, basis, x, obj per LP."""
    A, b, c, basis = batch(m, n)
    if rule == "devex":
        assert ctx.batched_devex_fits(m, n)
    g = ctx.simplex_solve_batched(A, b, c, basis, True, n - m, eps=eps, pivot_rule=rule)
    p = ctx.batched_problem(A, b, c, basis, True, n - m)
    try:
        assert p.path() == 1
        p.set_pivot_rule(rule)
        p.run(eps=eps)
        h = p.download()
    finally:
        p.free()
    for k in range(len(A)):
        r = _rule_ref(rule, batch, m, n, k, A[k], b[k], c[k], basis[k], eps)
        for out in (g, h):
            assert out["iters"][k] == r["iters"], (names[k], eps)
            _assert_lp(out, k, r, (names[k], eps))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_devex_batched(ctx, case):
    m, n, eps = case
    check_batched(ctx, m, n, eps)


TWO_PHASE_REF = {   # the references of the two-phase tests of each rule
    "dantzig": lambda A, b, c, no, eps: o.two_phase(A, b, c, True, no, eps=eps),
    "bland": lambda A, b, c, no, eps: bland_ref.two_phase(A, b, c, True, no, rule=bland_ref.BLAND, eps=eps),
    "devex": lambda A, b, c, no, eps: D.two_phase(A, b, c, True, no, eps=eps),
}


def check_two_phase(ctx, m, n, eps, batch=E.mixed, names=E.NAMES, rule="devex", single=True):
    """two_phase_batched on two_phase_form(batch(m, n)) under `rule` against the rule's reference; single: the
    single-LP entry too.  With single=False the handle form says that the batch ran one LP per workgroup."""
    A, b, c, _ = batch(m, n)
    A, b, c = E.two_phase_form(A, b, c)
    if rule == "devex":
        assert ctx.batched_devex_fits(m, n, True)
    if not single:
        p = ctx.batched_two_phase_problem(A, b, c, True, n - m)
        try:
            assert p.path() == 1
        finally:
            p.free()
    gb = ctx.two_phase_batched(A, b, c, True, n - m, eps=eps, pivot_rule=rule)
    for k in range(len(A)):
        what = (names[k], eps, rule)
        r = _ref((rule + "2",) + _batch_key(batch, m, n, k), eps,
                 lambda: TWO_PHASE_REF[rule](A[k], b[k], c[k], n - m, eps))
        if single:
            g = ctx.two_phase(A[k], b[k], c[k], True, n - m, eps=eps, pivot_rule=rule)
            assert g["status"] == r["status"] and g["iters"] == r["iters"], what
            assert np.array_equal(g["basis"], r["basis"]), what
            if r["status"] == OPTIMAL:
                assert _same_bits(g["x"], r["x"]) and _same_bits(g["obj"], r["obj"]), what
        assert gb["iters"][k].tolist() == list(r["iters"]), what
        _assert_lp(gb, k, r, what)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_devex_two_phase_and_batched(ctx, case):
    m, n, eps = case
    check_two_phase(ctx, m, n, eps)


def test_devex_scaled_costs(ctx):
    """c * 2^+-600 at eps = 0: d * d and (t * t) * we overflow or underflow long before d does, and the reference
    takes another path than on the unscaled costs; 2^+-300 stays inside fp64.  Compared with the reference on the
    scaled inputs (no invariance is claimed)."""
    m, n = 64, 160
    cases, refs = [], []
    for fam, seed, idx in E.SCALED:
        for k in E.SCALED_DIFFERENT + E.SCALED_SAME:
            A, b, c, basis = E.scaled_cost_case(fam, seed, idx, k)
            r = _devex_ref(("scaled", fam, k), A, b, c, basis, 0.0)
            _assert_same(_run_devex(ctx, A, b, c, basis, 0.0, capi.SIMPLEX_LAUNCH), r, (fam, k))
            cases.append((A, b, c, basis))
            refs.append(r)
    A, b, c, basis = (np.stack(v) for v in zip(*cases))
    g = ctx.simplex_solve_batched(A, b, c, basis, True, n - m, eps=0.0, pivot_rule="devex")
    for k, r in enumerate(refs):
        assert g["iters"][k] == r["iters"], k
        _assert_lp(g, k, r, k)


# ---- B: bounded re-solve ----------------------------------------------------------------------------------------------
def _assert_bounded(g, r, what):
    assert g["status"] == r["status"], what
    assert list(g["iters"]) == list(r["iters"]), what
    assert np.array_equal(g["basis"], r["basis"]) and np.array_equal(g["at_upper"], r["at_upper"]), what
    assert _same_bits(g["x"], r["x"]) and _same_bits(g["obj"], r["obj"]), what


def check_bounded_resolve(ctx, m, n, eps, kind, batch=E.mixed, names=E.NAMES, single=None):
    """bounded_resolve_batched on the warm starts of batch(m, n) perturbed by `kind`, and the single-LP entry on the
    kept LPs at the positions `single` (None: all of them), against bounded_resolve_ref."""
    assert ctx.bounded_fits(m, n)
    keep, warm = E.resolve_batch(m, n, eps, kind, batch)
    refs = E.resolve_ref(m, n, eps, kind, batch)
    assert len(keep) >= len(names) - 2
    gb = ctx.bounded_resolve_batched(*warm, True, n - m, eps=eps)
    for j, (k, r) in enumerate(zip(keep, refs)):
        what = (names[k], eps, kind)
        _assert_bounded({key: v[j] for key, v in gb.items()}, r, what)
        if single is not None and j not in [s % len(keep) for s in single]:
            continue
        one = [w[j] for w in warm]
        if r["status"] == BAD_ARG:   # no valid start: a status in a batch, an error for one LP
            _bad_arg(lambda: ctx.bounded_resolve(*one, True, n - m, eps=eps))
        else:
            _assert_bounded(ctx.bounded_resolve(*one, True, n - m, eps=eps), r, what)


@pytest.mark.parametrize("kind", W.PERTURBATIONS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_bounded_resolve_and_batched(ctx, case, kind):
    m, n, eps = case
    check_bounded_resolve(ctx, m, n, eps, kind)


# ---- C: bounded MIP ---------------------------------------------------------------------------------------------------
def _assert_mip(g, r, what):
    assert g["status"] == r["status"] and g["found"] == r["found"], what
    assert tuple(int(v) for v in g["stats"]) == r["stats"], what
    assert _same_bits(g["x"], r["x"]) and _same_bits(g["obj"], r["obj"]) and _same_bits(g["bound"], r["bound"]), what


def check_mip_bounded(ctx, m, n, eps, seed):
    """mip_bounded_solve_batched on boxed_mip_ties(m, n, seed) under MIP_LIMITS, and the single-LP entry on the first
    and the last LP with an OPTIMAL root, against mip_bounded_ref."""
    no = n - m
    assert ctx.mip_bounded_fits(m, n, E.MIP_LIMITS["max_depth"])
    A, b, c, lo, hi, mask = E.boxed_mip_ties(m, n, seed)
    refs = E.mip_ref(m, n, eps, seed)
    ok = np.array([root["status"] == OPTIMAL for root, _ in refs])
    assert ok.sum() >= len(refs) - 3
    root_status = np.array([root["status"] for root, _ in refs], np.int32)
    basis = np.stack([root["basis"] if o_ else np.zeros(m, np.int32) for o_, (root, _) in zip(ok, refs)])
    up = np.stack([root["at_upper"] if o_ else np.zeros(n, np.int32) for o_, (root, _) in zip(ok, refs)])
    g = ctx.mip_bounded_solve_batched(A, b, c, lo, hi, mask, basis, up, root_status, True, no, eps=eps, **E.MIP_LIMITS)
    for k, (root, r) in enumerate(refs):
        row = dict(status=int(g["status"][k]), found=int(g["found"][k]), x=g["x"][k], obj=g["obj"][k],
                   bound=g["bound"][k], stats=g["stats"][k])
        if r is None:   # kept out of the search by its root status
            assert row["status"] == root["status"] and row["found"] == 0 and not row["stats"].any(), (k, eps)
            assert np.isnan(row["obj"]) and np.isnan(row["bound"]) and np.all(np.isnan(row["x"])), (k, eps)
        else:
            _assert_mip(row, r, (k, eps))
    for k in np.flatnonzero(ok)[[0, -1]]:   # a tie LP and a near-tie LP through the single entry
        r = refs[k][1]
        args = (A[k], b[k], c[k], lo[k], hi[k], basis[k], up[k], mask, True, no)
        if r["status"] == BAD_ARG:
            _bad_arg(lambda: ctx.mip_bounded_solve(*args, eps=eps, **E.MIP_LIMITS))
        else:
            _assert_mip(ctx.mip_bounded_solve(*args, eps=eps, **E.MIP_LIMITS), r, (k, eps))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_mip_bounded_batched_and_single(ctx, case):
    m, n, eps = case
    check_mip_bounded(ctx, m, n, eps, E.MIP_SEED[(m, n)])


# ---- D: parametric right-hand side and cost ---------------------------------------------------------------------------
REFUSED = (SINGULAR, BAD_ARG)
_PARAMETRIC = {
    "rhs": dict(mod=parametric_ref, fits="basis_parametric_fits", batched="basis_parametric_batched",
                single="basis_parametric", handle="parametric"),
    "cost": dict(mod=parametric_cost_ref, fits="basis_parametric_cost_fits", batched="basis_parametric_cost_batched",
                 single="basis_parametric_cost", handle="parametric_cost"),
}


def _assert_path(g, r, what):
    """One LP: g and r trimmed dicts (status, t, obj, slope, enter, leave, basis)."""
    assert g["status"] == r["status"], what
    if r["status"] in REFUSED:
        return
    for key in ("enter", "leave", "basis"):
        assert np.array_equal(g[key], r[key]), (what, key)
    for key in ("t", "obj", "slope"):
        assert _same_bits(g[key], r[key]), (what, key)


def _lp_of(out, k):
    return {key: v[k] for key, v in out.items()}


def check_parametric(ctx, m, n, eps, which, seed, batch=E.mixed, names=E.NAMES, single=True):
    """The parametric RHS or cost path on batch(m, n, seed) at the oracle's final bases: the batched entry, the handle
    form after a batched run at the same eps (one LP per workgroup) and, with single, the single-LP entry."""
    P = _PARAMETRIC[which]
    trim = P["mod"].trim
    assert getattr(ctx, P["fits"])(m, n)
    A, b, c, basis, d, g_, status = E.parametric_inputs(m, n, eps, seed, batch)
    direction = d if which == "rhs" else g_
    ref = E.parametric_refs(m, n, eps, which, seed, batch=batch)
    kw = dict(eps=eps, max_breaks=E.MAX_BREAKS)
    # the batched entry
    gb = getattr(ctx, P["batched"])(A, b, c, basis, direction, np.inf, True, **kw)
    # the handle after a batched run at the same eps
    slack = np.tile(np.arange(n - m, n, dtype=np.int32), (len(A), 1))
    p = ctx.batched_problem(A, b, c, slack, True, n - m)
    try:
        assert p.path() == 1
        p.run(eps=eps)
        run = p.download()
        gh = getattr(p, P["handle"])(direction, **kw)
    finally:
        p.free()
    assert np.array_equal(run["status"], status) and np.array_equal(run["basis"], basis)
    href = E.parametric_refs(m, n, eps, which, seed, handle=True, batch=batch)
    for k in range(len(A)):
        what = (names[k], eps, which)
        r = _lp_of(ref, k)
        assert gb["nseg"][k] == r["nseg"] or r["status"] in REFUSED, what
        _assert_path(trim(_lp_of(gb, k)), trim(r), what)
        rh = _lp_of(href, k)
        assert gh["nseg"][k] == rh["nseg"] or rh["status"] in REFUSED, what
        _assert_path(trim(_lp_of(gh, k)), trim(rh), what)
        if not single:
            continue
        # the single-LP entry
        call = lambda: getattr(ctx, P["single"])(A[k], b[k], c[k], basis[k], direction[k], np.inf, True, **kw)  # noqa: E731
        if r["status"] == BAD_ARG:
            _bad_arg(call)
        else:
            _assert_path(call(), trim(r), what)


@pytest.mark.parametrize("which", ["rhs", "cost"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_parametric_three_calling_forms(ctx, case, which):
    m, n, eps = case
    check_parametric(ctx, m, n, eps, which, E.PARAMETRIC_SEED[(m, n)])


# ---- E: the domain of eps ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", E.BAD_EPS, ids=["neg", "neginf", "nan"])
def test_entries_refuse_eps_outside_its_domain_and_work_afterwards(ctx, eps):
    m, n = 8, 24
    no = n - m
    A, b, c, basis = lpcases.random_lp(3, m, n)
    two = lambda v: np.stack([v, v])   # noqa: E731
    AB, bB, cB, basisB = (two(v) for v in (A, b, c, basis))
    lo, hi = np.zeros(n), np.full(n, np.inf)
    hi[:no] = 2.0
    mask = np.r_[np.ones(no), np.zeros(m)].astype(np.int32)
    root = bounded_ref.bounded(A, b, c, lo, hi, True, no)
    assert root["status"] == OPTIMAL
    bs, up = root["basis"], root["at_upper"]
    kw = dict(max_depth=12, max_nodes=300)

    rr = W.resolve(A, b, c, lo, hi, bs, up, True, no)
    _bad_arg(lambda: ctx.bounded_resolve(A, b, c, lo, hi, bs, up, True, no, eps=eps))
    _assert_bounded(ctx.bounded_resolve(A, b, c, lo, hi, bs, up, True, no), rr, "resolve")
    _bad_arg(lambda: ctx.bounded_resolve_batched(AB, bB, cB, two(lo), two(hi), two(bs), two(up), True, no, eps=eps))
    gb = ctx.bounded_resolve_batched(AB, bB, cB, two(lo), two(hi), two(bs), two(up), True, no)
    _assert_bounded({key: v[1] for key, v in gb.items()}, rr, "resolve batched")

    rm = mip_bounded_ref.mip(A, b, c, lo, hi, bs, up, mask, True, no, **kw)
    _bad_arg(lambda: ctx.mip_bounded_solve(A, b, c, lo, hi, bs, up, mask, True, no, eps=eps, **kw))
    _assert_mip(ctx.mip_bounded_solve(A, b, c, lo, hi, bs, up, mask, True, no, **kw), rm, "mip")
    _bad_arg(lambda: ctx.mip_bounded_solve_batched(AB, bB, cB, two(lo), two(hi), mask, two(bs), two(up), None, True, no,
                                                   eps=eps, **kw))
    gm = ctx.mip_bounded_solve_batched(AB, bB, cB, two(lo), two(hi), mask, two(bs), two(up), None, True, no, **kw)
    _assert_mip(dict(status=int(gm["status"][1]), found=int(gm["found"][1]), x=gm["x"][1], obj=gm["obj"][1],
                     bound=gm["bound"][1], stats=gm["stats"][1]), rm, "mip batched")

    rd = D.simplex_tableau(A, b, c, basis, True, no)
    rt = D.two_phase(A, b, c, True, no)
    _bad_arg(lambda: ctx.simplex_solve(A, b, c, basis, True, no, eps=eps, pivot_rule="devex"))
    g = ctx.simplex_solve(A, b, c, basis, True, no, pivot_rule="devex")
    assert g["status"] == rd["status"] and g["iters"] == rd["iters"] and _same_bits(g["x"], rd["x"])
    _bad_arg(lambda: ctx.two_phase(A, b, c, True, no, eps=eps, pivot_rule="devex"))
    g = ctx.two_phase(A, b, c, True, no, pivot_rule="devex")
    assert g["status"] == rt["status"] and g["iters"] == rt["iters"] and _same_bits(g["x"], rt["x"])
    _bad_arg(lambda: ctx.simplex_solve_batched(AB, bB, cB, basisB, True, no, eps=eps, pivot_rule="devex"))
    g = ctx.simplex_solve_batched(AB, bB, cB, basisB, True, no, pivot_rule="devex")
    assert g["iters"][1] == rd["iters"]
    _assert_lp(g, 1, rd, "devex batched")
    _bad_arg(lambda: ctx.two_phase_batched(AB, bB, cB, True, no, eps=eps, pivot_rule="devex"))
    g = ctx.two_phase_batched(AB, bB, cB, True, no, pivot_rule="devex")
    assert g["iters"][1].tolist() == rt["iters"]
    _assert_lp(g, 1, rt, "devex two-phase batched")
    # the handles with the rule set
    p = ctx.simplex_problem(A, b, c, basis, True, no)
    try:
        p.set_pivot_rule("devex")
        _bad_arg(lambda: p.run(eps=eps))
        rc, st = p.run()
        assert rc == rd["status"] and st.pivots == rd["iters"]
    finally:
        p.free()
    for tp in (False, True):
        bp = ctx.batched_two_phase_problem(AB, bB, cB, True, no) if tp else \
            ctx.batched_problem(AB, bB, cB, basisB, True, no)
        try:
            bp.set_pivot_rule("devex")
            _bad_arg(lambda: bp.run(eps=eps))
            bp.run()
            _assert_lp(bp.download(), 0, rt if tp else rd, "handle")
        finally:
            bp.free()
