"""The inputs of tests/mip_tie_cases.py do what their names say, shown on the references alone
(tests/ref/mip_bounded_ref.c and tests/ref/mip_ref.c), so that the GPU comparisons of tests/test_gpu_mip_ties.py
cannot pass on vacuous inputs: the tied dist values are equal bit for bit, the depth ladder names the branching order (and no other set of columns gives
its bounds), the int_tol and gap edges fall on the stated side, the directions show in the counters, the objective
chain's three sums differ, and the recorded result of the 1100-row case is the reference's."""
import numpy as np
import pytest

from simplexmethod_amd import capi
from tests import bounded_resolve_ref as BR
from tests import mip_bounded_large_cases as Q
from tests import mip_tie_cases as K
from tests.test_gpu_mip_bounded import _same

OPTIMAL, UNBOUNDED, ITER_LIMIT, SINGULAR, INFEASIBLE, BAD_ARG = range(6)


def _bits(v):
    return np.float64(v).view(np.uint64)


def _agree(p, r):
    """The row form's result against the bounded form's: everything but the counters' layout."""
    assert (p["status"], p["found"]) == (r["status"], r["found"])
    assert p["stats"] == r["stats"][:3] + r["stats"][4:]
    for k in ("x", "obj", "bound"):
        assert np.array_equal(_bits(p[k]), _bits(r[k]))


def _ladder(cs, order, run_plain, **kw):
    """The reference's bound at every depth is the designed order's sum and no other set's."""
    k = len(order)
    full = cs.order if hasattr(cs, "order") else order
    for d in K.depths(cs):
        r = K.ref_bounded(cs, max_depth=d, **kw)
        if d < k:
            assert (r["status"], r["found"]) == (ITER_LIMIT, 0) and np.all(np.isnan(r["x"]))
            assert r["bound"] == K.ladder_bound(cs, full[:d])
            others = K.other_sets(cs, d)
            assert others and all(K.ladder_bound(cs, s) != r["bound"] for s in others)
            assert r["stats"][4] == d
        else:
            assert (r["status"], r["found"]) == (OPTIMAL, 1)
            assert r["obj"] == r["bound"] == K.ladder_bound(cs, full)
            assert r["stats"] == (2 * k + 1, k, 0, 0, k)
            want = {j: np.floor(v) for j, v, _ in cs.rows}
            assert all(r["x"][j] == v for j, v in want.items()) and np.count_nonzero(r["x"]) == len(want)
        if run_plain and cs.plain and K.fits(K.PLAIN_FITS_TO, cs.shape, d):
            _agree(K.ref_plain(cs, max_depth=d, **kw), r)


def test_fits_tables_are_the_library_s():
    lib = capi.load()
    for shape in (K.WIDE, K.LDS16, K.LDS4, K.SMALL, K.TALL):
        for d in (0, 1, 14, 21, 22, 23, 64, 65, 185, 186, 1024):
            assert bool(lib.lp_mip_bounded_fits(*shape, d)) == K.fits(K.BOUNDED_FITS_TO, shape, d)
            assert bool(lib.lp_mip_fits(*shape, d)) == K.fits(K.PLAIN_FITS_TO, shape, d)


# ---- A: the order of tied columns
@pytest.mark.parametrize("name,shape", K.ORDER_CASES)
def test_order_ladders(name, shape):
    cs = K.order_case(name, shape)
    assert K.designed_order(cs) == cs.order and len(cs.order) == len(cs.frac)
    _ladder(cs, cs.order, True)


def test_tied_dists_are_equal_bit_for_bit_and_sit_on_the_seams():
    def dists(cs):
        return {j: K.dist(v) for j, v, _ in cs.frac}

    d = dists(K.order_case("wide_thread", K.WIDE))
    assert len({_bits(v) for v in d.values()}) == 1
    assert {5 % 1024, 1029 % 1024, 2053 % 1024, 4101 % 1024} == {5} and 70 // 64 == 1 and 4102 % 1024 == 6
    assert 4101 >= 4096   # past one chunk of the objective chain, the thread's fifth column
    d = dists(K.order_case("wide_last_wave", K.WIDE))
    assert len({_bits(v) for v in d.values()}) == 1
    assert (min(d) % 1024) // 64 == 15 and sorted((j % 1024) // 64 for j in d) == [0, 1, 14, 15]
    for name, shape, stride in (("wide_lanes", K.WIDE, 1024), ("lds_lanes", K.LDS16, 64), ("lds_lanes", K.LDS4, 64)):
        cs = K.order_case(name, shape)
        d = dists(cs)
        pairs = list(zip(cs.order[::2], cs.order[1::2]))
        for (a, b), (off, hi_lane, lo_lane) in zip(pairs, K.BUTTERFLY):
            assert _bits(d[a]) == _bits(d[b]) and a < b
            # the lower index in the higher lane, one bit apart: the pair meets at that offset of the butterfly
            assert (a % stride % 64, b % stride % 64) == (hi_lane, lo_lane) and hi_lane ^ lo_lane == off
            assert hi_lane > lo_lane
        assert sorted(off for off, _, _ in K.BUTTERFLY) == [1, 2, 4, 8, 16, 32]
        assert len(set(d.values())) == len(pairs)
        if stride == 64:
            a, b = pairs[-1]
            assert (a, b) == K.SAME_LANE and b == a + 64 and _bits(d[a]) == _bits(d[b])
        else:   # one thread holds only its own pair's higher column
            assert all(b - 1024 < 64 for _, b in pairs)
    d = dists(K.order_case("lds_equal", K.LDS16))
    assert len({_bits(v) for v in d.values()}) == 1 and {75 - 11, 72 - 40 - 32, 68 - 20 - 48} == {64, 0}
    for name, shape, stride in (("wide_larger", K.WIDE, 1024), ("lds_larger", K.LDS16, 64)):
        cs = K.order_case(name, shape)
        d = dists(cs)
        lo_pair, big = cs.order[2:], cs.order[:2]
        assert _bits(d[lo_pair[0]]) == _bits(d[lo_pair[1]]) and d[big[0]] == d[big[1]] > d[lo_pair[0]]
        assert min(big) > max(lo_pair)   # the larger dist at the higher index


# ---- B: dist against int_tol
@pytest.mark.parametrize("name", sorted(K.TOL_CASES))
def test_int_tol_edge(name):
    cs = K.tol_case(name)
    shape, cols, vs, kw, (status, found, stats, xs) = K.TOL_CASES[name]
    int_tol = kw["int_tol"]
    edge = [K.dist(v) for v in vs]
    if name.endswith("edge"):
        assert all(_bits(d) == _bits(int_tol) for d in edge)
    elif int_tol > 0.0:
        # 2^-50 above: the smallest step both values can carry (one ulp of 5 - 2^-20, two of 3 + 2^-20)
        assert all(d == int_tol * (1.0 + 2.0 ** -30) == int_tol + K.TOL_STEP for d in edge)
        assert vs[1] == np.nextafter(5.0 - int_tol, 0.0)
        assert vs[0] == np.nextafter(np.nextafter(3.0 + int_tol, 4.0), 4.0)
    else:
        assert edge == [K.TINY]
    if len(vs) == 2:   # the f side and the 1 - f side
        assert vs[0] - np.floor(vs[0]) < 0.5 < vs[1] - np.floor(vs[1])
    r = K.ref_bounded(cs, **cs.kw)
    assert (r["status"], r["found"], r["stats"]) == (status, found, stats)
    if found:
        assert tuple(r["x"][list(cols)]) == xs
    else:
        assert np.all(np.isnan(r["x"])) and r["bound"] == K.root_z(cs)   # every node of the dive keeps the 2^-40
    if K.fits(K.PLAIN_FITS_TO, shape, K.DEEP):
        _agree(K.ref_plain(cs, **cs.kw), r)
    if shape == K.WIDE:
        assert min(cols) >= 1024


# ---- C: direction, negative values, flagged basic columns
@pytest.mark.parametrize("name", sorted(K.DIR_COLS))
def test_directions(name):
    cs = K.dir_case(name)
    assert K.designed_order(cs) == cs.order
    _ladder(cs, cs.order, True)
    full = K.ref_bounded(cs, max_depth=K.DEEP)
    for j, v, _ in cs.frac:
        assert full["x"][j] == np.floor(v)   # (with lo != 0 the node's x is lo + w: still the dyadic value)
    assert full["x"][3] == (-3.0 if name in K.DIR_LO else 2.0)
    # the same nodes by one re-solve per node: the first children that end INFEASIBLE are the up-first columns'
    h = Q.host_search(BR.resolve, *K.bounded_args(cs), max_depth=K.DEEP)
    assert h["nodes"] == full["stats"][0] and h["infeasible_dives"] == K.DIR_UP_FIRST[name]
    assert K.DIR_UP_FIRST[name] == sum(v - np.floor(v) > 0.5 for _, v, _ in cs.frac)
    # and the node-limit ladder sees them: a down-first dive is the node that adds a dual pivot, an up-first dive adds
    # none and its rebuild does
    pivots = [K.ref_bounded(cs, max_depth=K.DEEP, max_nodes=nodes)["stats"][1] for nodes in K.node_limits(cs)]
    firsts = []
    node = 1
    for j in cs.order:   # the dives of the way down are nodes 2, 3, ... with a rebuild after each up-first one
        (v,) = [v for q, v, _ in cs.frac if q == j]
        up_first = v - np.floor(v) > 0.5
        firsts.append(pivots[node] - pivots[node - 1] == (0 if up_first else 1))
        node += 2 if up_first else 1
    assert all(firsts)
    if cs.plain:
        for nodes in K.node_limits(cs):
            kw = dict(max_depth=K.DEEP, max_nodes=nodes)
            _agree(K.ref_plain(cs, **kw), K.ref_bounded(cs, **kw))


def test_half_goes_down_and_one_step_above_goes_up():
    half, above = K.dir_case("half"), K.dir_case("half_above")
    assert half.frac[0][1] - 2.0 == 0.5 and above.frac[0][1] - 2.0 == 0.5 + 2.0 ** -30
    a = K.ref_bounded(half, max_depth=K.DEEP, max_nodes=2)
    b = K.ref_bounded(above, max_depth=K.DEEP, max_nodes=2)
    # two nodes: the down child is the incumbent after one dual pivot, the up child is infeasible without one
    assert (a["status"], a["found"], a["stats"]) == (ITER_LIMIT, 1, (2, 1, 0, 0, 1))
    assert (b["status"], b["found"], b["stats"]) == (ITER_LIMIT, 0, (2, 0, 0, 0, 1))


def test_flagged_basic_columns_are_a_valid_start():
    cs = K.dir_case("dir_flagged")
    plain = K.dir_case("dir_neg")
    assert [j for j in range(cs.n_orig) if cs.up[j]] == list(K.DIR_FLAGGED["dir_flagged"])
    assert all(j in cs.basis for j in K.DIR_FLAGGED["dir_flagged"]) and np.all(np.isfinite(cs.hi[cs.up == 1]))
    a, b = K.ref_bounded(cs, max_depth=K.DEEP), K.ref_bounded(plain, max_depth=K.DEEP)
    _same(a, b)   # a basic column's flag changes how its value is held, not the search


# ---- D: z against zstar +- gap
@pytest.mark.parametrize("shape", [K.SMALL, K.WIDE])
@pytest.mark.parametrize("maximize", [True, False])
def test_gap_edge(shape, maximize):
    cs = K.gap_case(shape, maximize)
    assert cs.root_status == OPTIMAL and sorted(cs.basis) == sorted(cs.structural) and not cs.up.any()
    if shape == K.WIDE:
        assert cs.x >= 1024
    sgn = 1.0 if maximize else -1.0
    K_ = cs.K
    for gap, (obj, x, y) in zip(K.GAPS, ((2.0, 2.0, 0.0), (2.0, 2.0, 0.0), (2.25, 3.0, 0.5))):
        r = K.ref_bounded(cs, gap=gap, max_depth=K.DEEP)
        assert (r["status"], r["found"], r["stats"]) == (OPTIMAL, 1, (3, 2, 0, 0, 1))
        assert r["obj"] == r["bound"] == sgn * (obj + K_) and (r["x"][cs.x], r["x"][cs.y]) == (x, y)
        if K.fits(K.PLAIN_FITS_TO, shape, K.DEEP):
            _agree(K.ref_plain(cs, gap=gap, max_depth=K.DEEP), r)
    # the sums the edge rests on are exact
    z2, z225 = sgn * (2.0 + K_), sgn * (2.25 + K_)
    assert z2 + sgn * K.GAP_EDGE == z225 and z2 + sgn * K.GAPS[2] != z225 and z2 + sgn * K.GAPS[1] != z225


@pytest.mark.parametrize("shape", [K.SMALL, K.WIDE])
@pytest.mark.parametrize("maximize", [True, False])
def test_gap_edge_at_the_depth_limit(shape, maximize):
    """y integer as well: the 2.25 node is fractional, and at max_depth = 1 it is pruned at the edge and abandoned
    beyond it: the final status and the bound flip."""
    cs = K.gap_case(shape, maximize, y_marked=True)
    assert cs.mask[cs.y] == 1 and cs.root_status == OPTIMAL
    sgn = 1.0 if maximize else -1.0
    for gap, (status, bound) in zip(K.GAPS, ((OPTIMAL, 2.0), (OPTIMAL, 2.0), (ITER_LIMIT, 2.25))):
        r = K.ref_bounded(cs, gap=gap, max_depth=1)
        assert (r["status"], r["found"], r["stats"]) == (status, 1, (3, 2, 0, 0, 1))
        assert r["obj"] == sgn * (2.0 + cs.K) and r["bound"] == sgn * (bound + cs.K)
        assert (r["x"][cs.x], r["x"][cs.y]) == (2.0, 0.0)
        if K.fits(K.PLAIN_FITS_TO, shape, 1):
            _agree(K.ref_plain(cs, gap=gap, max_depth=1), r)


@pytest.mark.parametrize("maximize", [True, False])
def test_gap_edge_of_the_final_bound_at_the_node_limit(maximize):
    """Two nodes: the incumbent 2 and the root's record still open at z = 2.5: the bound is the open z only beyond the
    edge."""
    cs = K.gap_case(K.SMALL, maximize)
    sgn = 1.0 if maximize else -1.0
    for gap, bound in zip(K.LIMIT_GAPS, (2.0, 2.0, 2.5)):
        r = K.ref_bounded(cs, gap=gap, max_depth=K.DEEP, max_nodes=2)
        assert (r["status"], r["found"], r["stats"]) == (ITER_LIMIT, 1, (2, 1, 0, 0, 1))
        assert r["obj"] == sgn * (2.0 + cs.K) and r["bound"] == sgn * (bound + cs.K)
        _agree(K.ref_plain(cs, gap=gap, max_depth=K.DEEP, max_nodes=2), r)


def test_two_abandoned_nodes_of_equal_z():
    cs = K.gap_twin_case()
    status, found, stats, obj, bound = K.TWIN_WANT
    r = K.ref_bounded(cs, **K.TWIN_RUN)
    assert (r["status"], r["found"], r["stats"]) == (status, found, stats)
    assert r["obj"] == obj + cs.K and r["bound"] == bound + cs.K
    assert [r["x"][j] for pair in K.TWIN_XY for j in pair] == [2.0, 0.0, 2.0, 0.0]
    assert (2.0 + 2.25) + cs.K == (2.25 + 2.0) + cs.K < bound + cs.K   # the two abandoned nodes before the last
    # without the depth limit the abandoned nodes lead nowhere (y = 1 makes x = 3.5): the incumbent is the optimum
    deep = K.ref_bounded(cs, max_depth=K.DEEP)
    assert (deep["status"], deep["obj"], deep["bound"]) == (OPTIMAL, 4.0 + cs.K, 4.0 + cs.K) and deep["stats"][4] > 2
    _agree(K.ref_plain(cs, **K.TWIN_RUN), r)


# ---- E: the objective chain across 4096 products
def test_chain_sums_differ():
    cs = K.chain_case()
    assert [j for j, *_ in K.CHAIN_COLS] == [4090, 4094, 4100] and not cs.A[:, [4090, 4094, 4100]].any()
    r = K.ref_bounded(cs, max_depth=K.DEEP)
    assert (r["status"], r["found"], r["stats"]) == (OPTIMAL, 1, (13, 6, 0, 0, 6))
    x = np.zeros(cs.A.shape[1])
    x[:cs.n_orig] = r["x"]
    assert (x[4090], x[4094], x[4100]) == (8.0, 1.0, 8.0)
    serial, chunked, exact = K.chain_sums(cs, x)
    assert r["obj"] == serial and len({serial, chunked, exact}) == 3
    # everything before column 4100 is rounded away: what is left is the sum of the columns behind it
    assert serial == float(sum(cs.c[j] * x[j] for j in range(4101, cs.n_orig))) and chunked == 0.0
    assert exact == K.ref_bounded(K.order_case("wide_thread", K.WIDE), max_depth=K.DEEP)["obj"] + 0.375
    runs = [K.ref_bounded(cs, max_depth=d) for d in K.depths(cs)]
    assert [q["stats"][0] for q in runs] == [3, 5, 7, 9, 11, 13, 13]


# ---- F: the branching column at a basis position >= 1024
def test_tall_fixture_is_the_reference():
    """About 6 s: two crashes of 1100 pivots on a 1101 x 2201 tableau."""
    cs = K.tall_case()
    assert cs.shape[0] > 1024 and list(cs.basis) == list(range(cs.shape[0]))
    want = K.tall_fixture()
    _same(K.ref_bounded(cs, **K.TALL_RUN), want)
    assert (want["status"], want["bound"], want["stats"]) == K.TALL_WANT
    assert K.designed_order(cs) == (1030, 1090, 7) and cs.basis[1030] == 1030
    assert want["bound"] == K.ladder_bound(cs, (1030,))
    assert all(K.ladder_bound(cs, s) != want["bound"] for s in K.other_sets(cs, 1))


# ---- the batch
def test_batch_rows_take_different_decisions():
    cases = K.batch_cases(False)
    assert all(c.shape == K.SMALL and np.array_equal(c.mask, cases[0].mask) and c.maximize for c in cases)
    stats = [K.ref_bounded(c, **K.BATCH_KW)["stats"] for c in cases]
    assert len(set(stats)) >= 5
    plain = K.batch_cases(True)
    assert 4 <= len(plain) < len(cases)
    for c in plain:
        _agree(K.ref_plain(c, **K.BATCH_KW), K.ref_bounded(c, **K.BATCH_KW))
