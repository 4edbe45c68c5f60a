"""lp_mip_bounded_solve_large_ex and lp_mip_bounded_snapshot_bytes without a GPU: the entries are declared, bound and
exported and refuse what needs no device; tests/ref/mip_bounded_snapshots_ref.c with no snapshot is
tests/ref/mip_bounded_ref.c bit for bit, and with snapshots takes the same nodes to the same status; and the inputs of
tests/test_gpu_mip_bounded_snapshots.py reach what that file claims for them (restores, ring overwrites with rebuilds,
restored children that end infeasible, vertices that tell a restore from a rebuild), on the reference alone."""
import ctypes as C

import numpy as np

from simplexmethod_amd import build, capi
from tests import mip_bounded_large_cases as Q
from tests import mip_bounded_ref as R
from tests import mip_bounded_snapshots_cases as SC
from tests import mip_bounded_snapshots_ref as S
from tests.test_gpu_mip_bounded import _same

OPTIMAL, UNBOUNDED, ITER_LIMIT, SINGULAR, INFEASIBLE, BAD_ARG = range(6)

_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)


def test_entries_are_declared_bound_and_exported():
    sig = capi.SIGNATURES
    assert sig["lp_mip_bounded_solve_large_ex"] == (C.c_int, sig["lp_mip_bounded_solve_large"][1] + [C.c_int])
    assert sig["lp_mip_bounded_snapshot_bytes"] == (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint64)])
    lib = capi.load()
    assert hasattr(lib, "lp_mip_bounded_solve_large_ex") and hasattr(lib, "lp_mip_bounded_snapshot_bytes")
    build.build_hip()
    raw = C.CDLL(build.HIP_LIB)
    assert hasattr(raw, "lp_mip_bounded_solve_large_ex") and hasattr(raw, "lp_mip_bounded_snapshot_bytes")
    assert callable(getattr(capi.Context, "mip_bounded_snapshot_bytes"))
    assert lib.lp_abi_version() == 4


def _raw_call():
    d = np.zeros(16).ctypes.data_as(_dp)
    i = np.zeros(16, np.int32).ctypes.data_as(_ip)
    return [None, d, 2, 4, d, d, d, d, i, i, 1, 4, i, 1e-9, 1e-6, 1e-9, 4, 10, 10, d, d, d, i, i]


def test_refusals_that_need_no_device():
    lib = capi.load()
    fn = lib.lp_mip_bounded_solve_large_ex
    # without a context every call is refused, whatever snapshots is, and no output is touched
    x = np.full(4, 7.0)
    obj, bound = np.full(1, 7.0), np.full(1, 7.0)
    found, stats = np.full(1, 7, np.int32), np.full(7, 7, np.int32)
    call = _raw_call()
    call[19:24] = [x.ctypes.data_as(_dp), obj.ctypes.data_as(_dp), bound.ctypes.data_as(_dp), found.ctypes.data_as(_ip),
                   stats.ctypes.data_as(_ip)]
    for snapshots in (-1, 0, 3, 1024, 1025):
        assert fn(*call, snapshots) == BAD_ARG
    assert np.all(x == 7.0) and obj[0] == bound[0] == 7.0 and found[0] == 7 and np.all(stats == 7)
    # the reference refuses the same range before anything else
    args = SC.knapsack_args(1)
    for snapshots in (-1, 1025):
        assert S.mip(*args, snapshots=snapshots, **SC.KNAP_KW)["status"] == BAD_ARG
    assert S.mip(*args, snapshots=1024, **SC.KNAP_KW)["status"] == OPTIMAL


def test_snapshot_bytes():
    lib = capi.load()
    fn = lib.lp_mip_bounded_snapshot_bytes
    out = C.c_uint64(99)
    assert fn(4, 14, 3, None) == BAD_ARG
    for bad in ((0, 14, 3), (4, 3, 3), (4, 14, -1), (4, 14, 1025)):
        assert fn(*bad, C.byref(out)) == BAD_ARG and out.value == 99

    def slot(m, n):   # the (m+1) x ld tableau, ld = n + 1 rounded up to 8, then U and lo, n doubles rounded up to 2
        ld = (n + 1 + 7) // 8 * 8
        return 8 * ((m + 1) * ld + 2 * ((n + 1) // 2 * 2))

    for m, n in ((4, 14), (67, 201), (160, 320), (1100, 2300), (2048, 4096), (9960, 30000)):
        last = -1
        for K in (0, 1, 2, 4, 64, 1024):
            assert fn(m, n, K, C.byref(out)) == OPTIMAL
            assert out.value == K * slot(m, n) and out.value > last
            last = out.value
    assert slot(67, 201) == 8 * (68 * 208 + 2 * 202)
    assert slot(9960, 30000) > 2 ** 31   # one slot passes 2^31 bytes at a shape the entry accepts


def test_no_snapshot_is_the_plain_reference_and_snapshots_keep_the_search():
    searched = 0
    for key, args, kw in SC.large_cases():
        plain = Q.searched(*key, **kw)[1]
        r0 = SC.ref(key, args, snapshots=0, **kw)
        _same(dict(r0, stats=r0["stats"][:5]), plain)
        nodes, deepest = plain["stats"][0], plain["stats"][4]
        assert r0["stats"][5] == 0 and r0["stats"][6] < nodes
        for K in (4, kw["max_depth"]):
            r = SC.ref(key, args, snapshots=K, **kw)
            assert (r["status"], r["found"], r["stats"][0], r["stats"][4]) == (plain["status"], plain["found"], nodes,
                                                                               deepest)
            assert r["stats"][5] + r["stats"][6] == r0["stats"][6]
            if K == kw["max_depth"]:
                assert r["stats"][6] == 0
            if plain["found"]:
                assert abs(r["obj"] - plain["obj"]) <= 1e-9 * abs(plain["obj"])
        searched += nodes > 1
    assert searched >= 30


def test_knapsacks_reach_what_is_claimed():
    for seed, (nodes, restores, rebuilds, infeasible) in SC.KNAP_AT_3.items():
        args = SC.knapsack_args(seed)
        r = SC.ref(("knap", seed), args, snapshots=3, **SC.KNAP_KW)
        assert r["status"] == OPTIMAL and r["found"]
        assert (r["stats"][0], r["stats"][5], r["stats"][6], r["restored_infeasible"]) == (nodes, restores, rebuilds,
                                                                                          infeasible)
        plain = R.mip(*args, **SC.KNAP_KW)
        for K in SC.KNAP_KS:
            rk = SC.ref(("knap", seed), args, snapshots=K, **SC.KNAP_KW)
            assert (rk["status"], rk["found"], rk["stats"][0]) == (plain["status"], plain["found"], plain["stats"][0])
            assert rk["stats"][5] + rk["stats"][6] == restores + rebuilds
            assert abs(rk["obj"] - plain["obj"]) <= 1e-9 * abs(plain["obj"])
        # one slot: every level overwrites it; 24 = max_depth: nothing is ever rebuilt
        assert 0 < SC.ref(("knap", seed), args, snapshots=1, **SC.KNAP_KW)["stats"][5] < restores
        assert SC.ref(("knap", seed), args, snapshots=24, **SC.KNAP_KW)["stats"][6] == 0


def test_larger_searches_reach_what_is_claimed():
    m, n, seed, mx = 160, 320, 3, False
    kw = dict(max_depth=Q.BEYOND_DEPTH, max_nodes=60)
    args = Q.searched(m, n, seed, mx, "mixed", 2, **kw)[0]
    for K, want in SC.MIXED_3_MIN.items():
        r = SC.ref((m, n, seed, mx, "mixed", 2), args, snapshots=K, **kw)
        assert (r["stats"][5], r["stats"][6]) == want
    for seed in Q.BOX_SEEDS:
        kw = dict(max_depth=8, max_nodes=60)
        args = Q.searched(160, 320, seed, True, "box", 1, **kw)[0]
        r = SC.ref((160, 320, seed, True, "box", 1), args, snapshots=3, **kw)
        assert (r["stats"][5], r["stats"][6]) == SC.BOX_AT_3
    m, n, seed, mx, every, nodes = Q.BEYOND_INFEASIBLE_DIVES
    kw = dict(max_depth=Q.BEYOND_DEPTH, max_nodes=nodes)
    args = Q.searched(m, n, seed, mx, "mixed", every, **kw)[0]
    r = SC.ref((m, n, seed, mx, "mixed", every), args, snapshots=3, **kw)
    assert (r["stats"][5], r["stats"][6], r["restored_infeasible"]) == SC.INFEASIBLE_DIVES_AT_3
    # every GPU case restores something, and the small rings also rebuild somewhere
    runs = restored = rebuilt = 0
    for key, args, kw, Ks in SC.gpu_cases():
        for K in Ks:
            r = SC.ref(key, args, snapshots=K, **kw)
            runs += 1
            restored += r["stats"][5] > 0
            rebuilt += r["stats"][6] > 0
    assert runs == 19 and restored == runs and rebuilt >= 6


def test_a_restore_can_be_told_from_a_rebuild():
    """The incumbent of a search that restores differs from the rebuilt one's in some bit of x in at least five of the
    cases the GPU tests compare, so a kernel that restored nothing, or rebuilt nothing, could not pass them all."""
    differ = 0
    for key, args, kw, _ in SC.gpu_cases():
        r0 = SC.ref(key, args, snapshots=0, **kw)
        rk = SC.ref(key, args, snapshots=kw["max_depth"], **kw)
        if r0["found"] and rk["found"]:
            differ += r0["x"].tobytes() != rk["x"].tobytes()
    for seed in SC.KNAP_AT_3:
        args = SC.knapsack_args(seed)
        r0 = SC.ref(("knap", seed), args, snapshots=0, **SC.KNAP_KW)
        rk = SC.ref(("knap", seed), args, snapshots=24, **SC.KNAP_KW)
        differ += r0["x"].tobytes() != rk["x"].tobytes()
    assert differ >= 5, differ


def test_stopping_rules_reach_each_stop():
    pts = SC.stop_points(1, 3)
    assert set(pts) == {"branching", "second", "restore"}
    args = SC.knapsack_args(1)
    for kind, N in pts.items():
        r = SC.ref(("knap", 1), args, snapshots=3, max_depth=SC.KNAP_KW["max_depth"], max_nodes=N)
        assert r["status"] == ITER_LIMIT and r["stats"][0] == N
    args, kw = SC.iter_limit_case()
    for K, (restored, rebuilt) in ((0, (0, 1)), (3, (1, 0))):
        r = S.mip(*args, snapshots=K, **kw)
        assert r["status"] == ITER_LIMIT and r["stats"] == (3, 1, 0, 0, 1, restored, rebuilt) and not r["found"]
    assert S.mip(*args, snapshots=3, **dict(kw, max_iter=100))["status"] == OPTIMAL


def test_tall_fixture_is_recorded_from_the_reference():
    """The fixture's header says what it records; tests/golden/make_mip_bounded_snapshots_golden.py regenerates it (the
    root alone is 4368 primal pivots on a 1101 x 2301 tableau, about half a minute, so it is not re-run here)."""
    want, data = SC.tall_fixture()
    assert (data["max_depth"], data["max_nodes"], data["snapshots"]) == (SC.TALL_DEPTH, SC.TALL_NODES,
                                                                         SC.TALL_SNAPSHOTS)
    status, stats = Q.TALL_RUNS[(SC.TALL_DEPTH, SC.TALL_NODES)]
    # the same status, nodes and deepest level as the plain search of the same budget; both second children restored
    assert want["status"] == status and (want["stats"][0], want["stats"][4]) == (stats[0], stats[4])
    assert want["stats"][5:] == (2, 0)
    plain = Q.tall_fixture()[(SC.TALL_DEPTH, SC.TALL_NODES)]
    assert want["found"] == plain["found"]
