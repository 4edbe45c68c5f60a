"""The pivot rules of the bounded-variable simplex without a GPU: tests/ref/bounded_rules_ref.c and
tests/ref/bounded_resolve_rules_ref.c in Dantzig mode equal bounded_ref.c and bounded_resolve_ref.c bit for bit; with
lo = 0 and hi = inf Bland and Devex equal bland_ref's and devex_ref's two-phase; Beale's LP with boxed columns cycles
under Dantzig's rule and is solved by the other two, cold and re-solved from the slack basis; on 200 seeded LPs the
three rules agree on the status and the optimum; the recorded statuses and counts; and the host-side refusals of the
_ex entries and lp_simplex_bounded_rule_fits."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from simplexmethod_amd import capi
from tests import bland_ref, devex_ref
from tests import bounded_ref as B
from tests import bounded_resolve_ref as W
from tests import bounded_rules_ref as R

OPTIMAL, UNBOUNDED, ITER_LIMIT, SINGULAR, INFEASIBLE, BAD_ARG = range(6)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bounded_rules_cases.json")


def _identical(g, r):
    assert g["status"] == r["status"]
    assert list(g["iters"]) == list(r["iters"])
    assert np.array_equal(g["basis"], r["basis"]) and np.array_equal(g["at_upper"], r["at_upper"])
    assert np.array_equal(g["x"], r["x"], equal_nan=True)
    assert g["obj"] == r["obj"] or (np.isnan(g["obj"]) and np.isnan(r["obj"]))


def test_dantzig_mode_is_bounded_ref():
    for A, b, c, lo, hi, mx in R.seeded_lps(100):
        _identical(R.bounded(A, b, c, lo, hi, mx, rule=R.DANTZIG), B.bounded(A, b, c, lo, hi, mx))
    for m, n in ((8, 20), (32, 96)):
        A, b, c, lo, hi, mx = B.boxed_lp(1, m, n)
        _identical(R.bounded(A, b, c, lo, hi, mx, n - m, max_iter=7), B.bounded(A, b, c, lo, hi, mx, n - m, max_iter=7))


def test_dantzig_mode_is_bounded_resolve_ref():
    seen = set()
    for seed in range(36):
        A, b, c, lo, hi, mx = B.boxed_lp(seed, 6 + seed % 5, 18 + seed % 7)
        cold = B.bounded(A, b, c, lo, hi, mx)
        if cold["status"] != OPTIMAL:
            continue
        b2, c2, lo2, hi2 = W.perturb(seed, W.PERTURBATIONS[seed % 3], b, c, lo, hi, cold["basis"], cold["x"])
        r = W.resolve(A, b2, c2, lo2, hi2, cold["basis"], cold["at_upper"], mx)
        seen.add("dual" if r["iters"][0] else "primal" if r["iters"][1] + r["iters"][2] else "none")
        _identical(R.resolve(A, b2, c2, lo2, hi2, cold["basis"], cold["at_upper"], mx, rule=R.DANTZIG), r)
        if r["iters"][0]:   # the dual branch is the same under every rule
            for rule in (R.BLAND, R.DEVEX):
                _identical(R.resolve(A, b2, c2, lo2, hi2, cold["basis"], cold["at_upper"], mx, rule=rule), r)
    assert {"dual", "primal"} <= seen


@pytest.mark.parametrize("rule,ref", [(R.BLAND, bland_ref), (R.DEVEX, devex_ref)])
def test_identity_anchor_equals_the_two_phase_refs(rule, ref):
    def check(A, b, c, mx, no):
        n = A.shape[1]
        g = R.bounded(A, b, c, np.zeros(n), np.full(n, np.inf), mx, no, rule=rule)
        t = ref.two_phase(A, b, c, mx, no, rule=rule)
        assert g["status"] == t["status"] and g["iters"][:3] == list(t["iters"])[:3] and g["iters"][3] == 0
        assert np.array_equal(g["basis"], t["basis"]) and not g["at_upper"].any()
        if t["status"] == OPTIMAL:
            assert np.array_equal(g["x"], t["x"]) and g["obj"] == t["obj"]

    A, b, c, _, no = bland_ref.beale()
    for mx in (True, False):
        check(A, b, c if mx else -c, mx, no)
    for seed in range(12):
        A, b, c, _ = capi.gen_lp(seed, 6 + seed % 4, 16 + seed % 6)
        if seed % 3 == 0:
            b[::2] *= -1.0   # rows that change sign in phase I
        for mx in (False, True):
            check(A, b, c if mx else -c, mx, A.shape[1] - A.shape[0])


@pytest.mark.parametrize("maximize", [True, False])
def test_beale_boxed_cycles_under_dantzig_only(maximize):
    A, b, c, lo, hi = R.beale_boxed(100.0)
    c = c if maximize else -c
    basis, flags = R.slack_start(A)
    d = R.bounded(A, b, c, lo, hi, maximize, rule=R.DANTZIG)
    assert d["status"] == ITER_LIMIT and d["iters"] == [4, 0, 10000, 0]
    w = R.resolve(A, b, c, lo, hi, basis, flags, maximize, rule=R.DANTZIG)
    assert w["status"] == ITER_LIMIT and w["iters"] == [0, 10000, 0]
    for rule in (R.BLAND, R.DEVEX):
        for r in (R.bounded(A, b, c, lo, hi, maximize, rule=rule),
                  R.resolve(A, b, c, lo, hi, basis, flags, maximize, rule=rule)):
            assert r["status"] == OPTIMAL and r["obj"] == (1.0 if maximize else -1.0)
            assert np.array_equal(r["x"][:4], [1.0, 0.0, 1.0, 0.0])


def test_rules_agree_on_200_seeded_lps():
    seen = set()
    for A, b, c, lo, hi, mx in R.seeded_lps(200):
        rs = [R.bounded(A, b, c, lo, hi, mx, rule=rule) for rule in R.RULES]
        assert rs[0]["status"] == rs[1]["status"] == rs[2]["status"]
        seen.add(rs[0]["status"])
        if rs[0]["status"] != OPTIMAL:
            continue
        for r in rs:
            assert abs(r["obj"] - rs[0]["obj"]) <= 1e-9 * max(1.0, abs(rs[0]["obj"]))
            assert np.all(r["x"] >= lo - 1e-7) and np.all(r["x"] <= hi + 1e-7)
            assert np.abs(A @ r["x"] - b).max() <= 1e-7
    assert seen == {OPTIMAL, UNBOUNDED, INFEASIBLE}


def test_golden_statuses_and_counts():
    with open(GOLDEN) as f:
        cases = json.load(f)
    names = set()
    for cs in cases:
        names.add(cs["name"])
        mx, rule = bool(cs["maximize"]), cs["rule"]
        if cs["name"].startswith("beale_boxed"):
            A, b, c, lo, hi = R.beale_boxed()
            c = c if mx else -c
            if cs["name"].endswith("cold"):
                r = R.bounded(A, b, c, lo, hi, mx, rule=rule)
            else:
                r = R.resolve(A, b, c, lo, hi, *R.slack_start(A), mx, rule=rule)
        elif cs["name"] == "cycling_boxed":
            r = R.bounded(*R.cycling_boxed(), mx, max_iter=cs["max_iter"], rule=rule)
        else:
            A, b, c, lo, hi, mx2 = B.boxed_lp(cs["seed"], cs["m"], cs["n"], kind=cs["kind"])
            assert mx2 == mx
            r = R.bounded(A, b, c, lo, hi, mx, cs["n"] - cs["m"], rule=rule)
        assert (r["status"], r["iters"]) == (cs["status"], cs["iters"]), cs
        if cs["status"] == OPTIMAL:
            assert r["obj"] == float.fromhex(cs["obj"]), cs
    assert names == {"beale_boxed_cold", "beale_boxed_resolve", "cycling_boxed", "boxed_lp"}
    cyc = {cs["rule"]: cs["status"] for cs in cases if cs["name"] == "cycling_boxed"}
    assert cyc == {R.DANTZIG: ITER_LIMIT, R.BLAND: OPTIMAL, R.DEVEX: OPTIMAL}


def test_ex_entries_refuse_without_a_context_and_a_bad_rule():
    lib = capi.load()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    z = np.zeros(16)
    zi = np.zeros(16, np.int32)
    d, i = z.ctypes.data_as(dp), zi.ctypes.data_as(ip)
    for rule in (capi.PIVOT_DANTZIG, capi.PIVOT_BLAND, capi.PIVOT_DEVEX, 7, -1):
        assert lib.lp_simplex_bounded_ex(None, d, 2, 4, d, d, d, d, 1, 4, 1e-9, 10, d, i, i, d, i, rule) == BAD_ARG
        assert lib.lp_simplex_bounded_batched_ex(None, 1, d, 2, 4, d, d, d, d, 1, 4, 1e-9, 10, d, i, i, d, i, i,
                                                 rule) == BAD_ARG
        assert lib.lp_simplex_bounded_resolve_ex(None, d, 2, 4, d, d, d, d, i, i, 1, 4, 1e-9, 10, d, i, i, d, i,
                                                 rule) == BAD_ARG
        assert lib.lp_simplex_bounded_resolve_batched_ex(None, 1, d, 2, 4, d, d, d, d, i, i, 1, 4, 1e-9, 10, d, i, i, d,
                                                         i, i, rule) == BAD_ARG
    for rule in (7, -1, 3):
        assert lib.lp_simplex_bounded_rule_fits(8, 20, rule) == 0


def test_rule_fits_is_bounded_fits_except_for_devex_weights():
    lib = capi.load()
    for m, n in ((4, 12), (64, 192), (130, 140), (160, 320), (0, 4), (8, 4)):
        plain = lib.lp_simplex_bounded_fits(m, n)
        assert lib.lp_simplex_bounded_rule_fits(m, n, capi.PIVOT_DANTZIG) == plain
        assert lib.lp_simplex_bounded_rule_fits(m, n, capi.PIVOT_BLAND) == plain
        assert lib.lp_simplex_bounded_rule_fits(m, n, capi.PIVOT_DEVEX) <= plain
    assert lib.lp_simplex_bounded_rule_fits(130, 140, capi.PIVOT_DEVEX) == 1
    # the n doubles of weights: some widths at m = 64 fit plain and not under Devex
    edge = [n for n in range(64, 400) if lib.lp_simplex_bounded_fits(64, n)
            and not lib.lp_simplex_bounded_rule_fits(64, n, capi.PIVOT_DEVEX)]
    assert edge and edge == list(range(edge[0], edge[-1] + 1))
    assert not lib.lp_simplex_bounded_fits(64, edge[-1] + 1)
    assert lib.lp_simplex_bounded_rule_fits(64, edge[0] - 1, capi.PIVOT_DEVEX) == 1
    # the carve restated: Published (16 bytes), the tableau with an odd pitch, prow, lcol, U, lo as doubles, slotvar,
    # basis and flags as ints, then the weights 8-byte aligned, all rounded up to 16
    m, n = 64, edge[0]
    W_ = n + 1
    pitch = W_ if W_ % 2 else W_ + 1
    o = 16 + 8 * ((m + 1) * pitch + W_ + (m + 1) + 2 * n) + 4 * (2 * n + m)
    assert (o + 15) // 16 * 16 <= 160 * 1024
    o = (o + 7) // 8 * 8 + 8 * n
    assert (o + 15) // 16 * 16 > 160 * 1024
