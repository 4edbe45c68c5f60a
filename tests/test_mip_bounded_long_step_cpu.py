"""The bound-flipping ratio test in the branch-and-bound over the bounds, on the reference alone (no GPU):
tests/ref/mip_bounded_long_step_ref.c equals mip_bounded_snapshots_ref.c bit for bit under TEXTBOOK on every case the GPU
tests use; under LONG_STEP those cases reach a flip in each of the four kinds of dual loop, a node that ends infeasible
after a flip, a node at max_iter and every outcome of the nine-outcome batch; where both ratio tests finish, the
objectives agree within gap plus rounding; an unknown ratio writes nothing.  Then the library's new symbols, signatures
and keyword arguments."""
import ctypes as C
import inspect

import numpy as np
import pytest

from simplexmethod_amd import capi
from tests import mip_bounded_long_step_cases as LC
from tests import mip_bounded_long_step_ref as L
from tests import mip_bounded_snapshots_ref as S

OPTIMAL, UNBOUNDED, ITER_LIMIT, SINGULAR, INFEASIBLE, BAD_ARG = range(6)
TEXTBOOK, LONG_STEP = LC.TEXTBOOK, LC.LONG_STEP
GAP = 1e-9


def _bits_equal(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    nan = np.isnan(a)
    assert np.array_equal(nan, np.isnan(b))
    assert np.array_equal(a[~nan], b[~nan])


def _same(a, b):
    assert a["status"] == b["status"] and a["found"] == b["found"] and a["stats"] == b["stats"]
    _bits_equal(a["x"], b["x"])
    _bits_equal(a["obj"], b["obj"])
    _bits_equal(a["bound"], b["bound"])


def _all_cases():
    """(key, args, kw, Ks) of every search the GPU tests compare."""
    for key, kw in LC.lds_keys():
        args = LC.args_of(key)
        if args is not None:
            yield key, args, kw, LC.LDS_KS + (kw["max_depth"],)
    for key, kw in LC.beyond_keys():
        yield key, LC.args_of(key), kw, LC.BEYOND_KS
    key, args, kw = LC.root_after_bound_change()
    yield key, args, kw, (0, 2)
    for key, args, kw in LC.node_at_max_iter():
        yield key, args, kw, (0, 2)
    args, kw = LC.deep_args()
    yield ("deep",), args, kw, (0,)


def _outcome_rows():
    A, b, c, lo, hi, basis, up, mask, kinds, kw, expect = LC.outcome_cases()
    for k, kind in enumerate(kinds):
        yield kind, (A[k], b[k], c[k], lo[k], hi[k], basis[k], up[k], mask, True, 4), kw, expect[kind]


def test_textbook_is_the_snapshots_reference_bit_for_bit():
    n = 0
    for key, args, kw, Ks in _all_cases():
        for K in Ks:
            a = LC.ref(key, args, dual_ratio=TEXTBOOK, snapshots=K, **kw)
            b = S.mip(*args, snapshots=K, **kw)
            _same(a, b)
            assert a["diag"]["restored_infeasible"] == b["restored_infeasible"]
            n += 1
    for kind, args, kw, _ in _outcome_rows():
        for K in (0, 2):
            _same(L.mip(*args, dual_ratio=TEXTBOOK, snapshots=K, **kw), S.mip(*args, snapshots=K, **kw))
    assert n > 100


def test_every_kind_of_dual_loop_flips():
    total = dict.fromkeys(L.DIAG, 0)
    per_shape = {}
    for key, args, kw, Ks in _all_cases():
        for K in Ks:
            r = LC.ref(key, args, dual_ratio=LONG_STEP, snapshots=K, **kw)
            for name in L.DIAG:
                total[name] += r["diag"][name]
            d = r["diag"]
            # stats[3] is the dual loops' flips plus the primal loops' (none of these roots is primal feasible only)
            assert r["stats"][3] >= d["flips_root"] + d["flips_first"] + d["flips_rebuilt"] + d["flips_restored"]
            assert (d["flips_restored"] > 0) <= (r["stats"][5] > 0) and (K > 0 or r["stats"][5] == 0)
            if isinstance(key[0], int):
                per_shape[key[:2]] = per_shape.get(key[:2], 0) + (r["stats"][0] > 1 and r["stats"][3] > 0)
    for name in ("flips_root", "flips_first", "flips_rebuilt", "flips_restored", "infeasible_after_flip",
                 "dual_iter_limit", "restored_infeasible"):
        assert total[name] > 0, name
    # at least one searched case per shape flips, in LDS and beyond
    shapes = [s[:2] for s in LC.LDS_SHAPES] + list(LC.BEYOND_SHAPES)
    assert all(per_shape.get(s, 0) > 0 for s in shapes), per_shape


def test_the_root_flips_after_a_bound_change():
    key, args, kw = LC.root_after_bound_change()
    r = LC.ref(key, args, dual_ratio=LONG_STEP, snapshots=0, **kw)
    assert r["diag"]["flips_root"] > 0 and r["stats"][0] > 1
    # the root alone (max_nodes 1 stops on its branching): its flips are the whole count
    one = L.mip(*args, dual_ratio=LONG_STEP, max_depth=kw["max_depth"], max_nodes=1)
    assert one["stats"][0] == 1 and one["stats"][3] == r["diag"]["flips_root"] and one["stats"][2] == 0


def test_a_node_at_max_iter_stops_the_search():
    cases = LC.node_at_max_iter()
    assert len(cases) == 2
    flipped = 0
    for key, args, kw in cases:
        for K in (0, 2):
            r = LC.ref(key, args, dual_ratio=LONG_STEP, snapshots=K, **kw)
            assert r["status"] == ITER_LIMIT and r["diag"]["dual_iter_limit"] == 1
            assert 1 < r["stats"][0] < kw["max_nodes"]
            flipped += r["stats"][3]
    assert flipped > 0
    # max_iter bounds the dual pivots alone: a node of the second case made max_iter pivots and flips besides
    key, args, kw = cases[1]
    r = LC.ref(key, args, dual_ratio=LONG_STEP, snapshots=0, **kw)
    assert r["stats"][1] <= kw["max_iter"] * r["diag"]["dual_loops"] and r["stats"][3] > 0


def test_every_outcome_under_long_step():
    rows = list(_outcome_rows())
    assert len(rows) == 9, [k for k, *_ in rows]
    flips = 0
    for kind, args, kw, want in rows:
        r = L.mip(*args, dual_ratio=LONG_STEP, **kw)
        assert r["status"] == want, kind
        flips += r["stats"][3]
        if kind == "depth_limit":
            assert r["found"] and r["bound"] > r["obj"] and r["stats"][4] == kw["max_depth"]
        if kind == "node_limit":
            assert r["stats"][0] == kw["max_nodes"]
        if kind == "integer_infeasible":
            assert r["stats"][0] > 1 and not r["found"]
    assert flips > 0


def test_objectives_agree_where_both_finish():
    """Both searches LP_OPTIMAL: the same optimum within gap (each may stop at an incumbent that the other's beats by
    less than gap) plus the rounding of a sum of n products."""
    both = 0
    for key, args, kw, Ks in _all_cases():
        for K in Ks:
            a = LC.ref(key, args, dual_ratio=LONG_STEP, snapshots=K, **kw)
            b = LC.ref(key, args, dual_ratio=TEXTBOOK, snapshots=K, **kw)
            if a["status"] == OPTIMAL and b["status"] == OPTIMAL:
                n = args[0].shape[1]
                scale = float(np.abs(args[2]).sum() * max(1.0, np.abs(a["x"]).max()))
                assert abs(a["obj"] - b["obj"]) <= GAP + 4 * n * np.finfo(float).eps * scale, key
                both += 1
    assert both >= 20


@pytest.mark.parametrize("dual_ratio", [2, -1])
def test_the_reference_refuses_an_unknown_ratio_before_writing(dual_ratio):
    key, kw = LC.lds_keys()[0]
    args = LC.args_of(LC.lds_keys()[3][0])
    m, n = args[0].shape
    x = np.full(n - m, 7.0)
    obj, bound = C.c_double(7.0), C.c_double(7.0)
    found = C.c_int(7)
    stats, diag = np.full(7, 7, np.int32), np.full(8, 7, np.int32)
    A, b, c, lo, hi, basis, up, mask, mx, no = args
    Af = np.ascontiguousarray(A.T).reshape(-1)
    bad_basis = np.full(m, -7, np.int32)   # (ahead of everything else: a bad basis and a bad snapshot count beside it)
    st = L.lib().ref_mip_bounded_long_step(L._d(Af), m, n, L._d(b), L._d(c), L._d(lo), L._d(hi), L._i(bad_basis),
                                           L._i(np.ascontiguousarray(up, np.int32)),
                                           int(mx), no, L._i(np.ascontiguousarray(mask, np.int32)), 1e-9, 1e-6, 1e-9,
                                           kw["max_depth"], 10, 100, L._d(x), C.byref(obj), C.byref(bound),
                                           C.byref(found), L._i(stats), -3, L._i(diag), dual_ratio)
    assert st == BAD_ARG
    assert np.all(x == 7.0) and obj.value == 7.0 and bound.value == 7.0 and found.value == 7
    assert np.all(stats == 7) and np.all(diag == 7)


def test_new_entries_exist_and_refuse_a_null_context():
    lib = capi.load()
    assert lib.lp_abi_version() == 4
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    args = LC.args_of(LC.lds_keys()[3][0])
    A, b, c, lo, hi, basis, up, mask, mx, no = args
    m, n = A.shape
    Af = capi.colmajor(A)
    z, zi = np.zeros(n), np.zeros(n, np.int32)
    d = lambda a: np.ascontiguousarray(a, np.float64).ctypes.data_as(dp)   # noqa: E731
    i = lambda a: np.ascontiguousarray(a, np.int32).ctypes.data_as(ip)   # noqa: E731
    head = (d(Af), m, n, d(b), d(c), d(lo), d(hi), i(basis), i(up))
    tail = (int(mx), no, i(mask), 1e-9, 1e-6, 1e-9, 8, 10, 100, d(z), d(z), d(z), i(zi), i(zi))
    assert lib.lp_mip_bounded_solve_ratio_ex(None, *head, *tail, 1) == BAD_ARG
    assert lib.lp_mip_bounded_solve_large_ratio_ex(None, *head, *tail, 2, 1) == BAD_ARG
    assert lib.lp_mip_bounded_solve_batched_ratio_ex(None, 1, *head, None, *tail, i(zi), 1) == BAD_ARG


def test_bindings():
    for name in ("mip_bounded_solve", "mip_bounded_solve_batched", "mip_bounded_solve_large"):
        p = inspect.signature(getattr(capi.Context, name)).parameters
        assert "dual_ratio" in p and p["dual_ratio"].default is None
    sig = capi.SIGNATURES
    assert sig["lp_mip_bounded_solve_ratio_ex"][1] == sig["lp_mip_bounded_solve"][1] + [C.c_int]
    assert sig["lp_mip_bounded_solve_batched_ratio_ex"][1] == sig["lp_mip_bounded_solve_batched"][1] + [C.c_int]
    assert sig["lp_mip_bounded_solve_large_ratio_ex"][1] == sig["lp_mip_bounded_solve_large_ex"][1] + [C.c_int]
