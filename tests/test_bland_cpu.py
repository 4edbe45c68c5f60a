"""CPU-only checks of Bland's pivot rule: the test restatement (tests/ref/bland_ref.c) equals the oracle
bit for bit in Dantzig mode, and under Bland's rule it solves Beale's cycling LP; the C ABI refuses a bad
rule and null handles without a device."""
import json
import os

import numpy as np
import pytest

from oracle import pyoracle as o
from simplexmethod_amd import capi
from tests import bland_ref as R
from tests import lpcases

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _beale_golden():
    return json.load(open(os.path.join(GOLDEN, "bland_cases.json")))["beale"]


def _same(r, q, tableau=True):
    assert r["status"] == q["status"]
    assert r["iters"] == q["iters"]
    assert r["trace"] == q["trace"]
    assert np.array_equal(r["basis"], q["basis"])
    if q["status"] == o.OPTIMAL:
        assert np.array_equal(r["x"], q["x"]) and r["obj"] == q["obj"]
    if tableau:
        assert np.array_equal(r["tableau"], q["tableau"])


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


def test_restatement_dantzig_matches_oracle():
    for A, b, c, basis, mx, no in _seeded_lps():
        q = o.simplex_tableau(A, b, c, basis, mx, no, trace_cap=1 << 14, want_tableau=True)
        r = R.simplex_tableau(A, b, c, basis, mx, no, rule=R.DANTZIG, trace_cap=1 << 14, want_tableau=True)
        _same(r, q)


def test_restatement_dantzig_matches_oracle_on_golden_cases():
    for g in json.load(open(os.path.join(GOLDEN, "simplex_cases.json"))):
        A, b, c, basis = lpcases.random_lp(g["seed"], g["m"], g["n"])
        no = g["n"] - g["m"]
        q = o.simplex_tableau(A, b, c, basis, True, no, trace_cap=1 << 14, want_tableau=True)
        r = R.simplex_tableau(A, b, c, basis, True, no, rule=R.DANTZIG, trace_cap=1 << 14, want_tableau=True)
        _same(r, q)
        assert r["iters"] == g["iters"] and r["basis"].tolist() == g["basis"]
    for g in json.load(open(os.path.join(GOLDEN, "two_phase_cases.json"))):
        if g["kind"] == "min":
            a = g["args"]
            A, b, c, no = lpcases.min_lp(g["seed"], a[0], a[1], equalities=a[2], negative_rows=a[3], zero_rhs=a[4])
        else:
            A, b, c, no = lpcases.degenerate_eq_lp(g["seed"])
        q = o.two_phase(A, b, c, False, no)
        r = R.two_phase(A, b, c, False, no, rule=R.DANTZIG)
        assert r["status"] == q["status"] and r["iters"] == q["iters"] == g["iters"]
        assert np.array_equal(r["basis"], q["basis"]) and np.array_equal(r["x"], q["x"]) and r["obj"] == q["obj"]


def test_restatement_two_phase_dantzig_matches_oracle():
    for seed in range(12):
        A, b, c, no = lpcases.min_lp(seed, 3 + seed % 6, 4 + seed % 5, equalities=seed % 2, negative_rows=seed % 3,
                                     zero_rhs=seed % 2)
        for mx in (False, True):
            q = o.two_phase(A, b, c, mx, no)
            r = R.two_phase(A, b, c, mx, no, rule=R.DANTZIG)
            assert r["status"] == q["status"] and r["iters"] == q["iters"]
            assert np.array_equal(r["basis"], q["basis"])
            if q["status"] == o.OPTIMAL:
                assert np.array_equal(r["x"], q["x"]) and r["obj"] == q["obj"]


def test_beale_cycles_under_dantzig_and_not_under_bland():
    g = _beale_golden()
    A, b, c, basis, no = R.beale()
    assert np.array_equal(A[:, :4], np.array(g["A0"])) and np.array_equal(c[:4], np.array(g["c0"]))
    d = R.simplex_tableau(A, b, c, basis, True, no, rule=R.DANTZIG, trace_cap=12)
    assert d["status"] == g["dantzig"]["status"] == o.ITER_LIMIT and d["iters"] == g["dantzig"]["iters"]
    assert d["trace"][:6] == [tuple(t) for t in g["dantzig"]["trace_head"]]
    assert d["trace"][6:12] == d["trace"][:6]   # period 6
    q = o.simplex_tableau(A, b, c, basis, True, no, trace_cap=12)
    assert q["status"] == o.ITER_LIMIT and q["trace"] == d["trace"]
    e = R.simplex_tableau(A, b, c, basis, True, no, rule=R.BLAND, trace_cap=64)
    gb = g["bland"]
    assert e["status"] == gb["status"] == o.OPTIMAL and e["iters"] == gb["iters"] == 7
    assert e["trace"] == [tuple(t) for t in gb["trace"]]
    assert e["basis"].tolist() == gb["basis"] and e["obj"] == gb["obj"] == 1.0 and e["x"].tolist() == gb["x"]


def test_beale_two_phase_under_bland():
    g = _beale_golden()
    A, b, c, _, no = R.beale()
    for mx, cost, key in ((True, c, "two_phase_bland_max"), (False, -c, "two_phase_bland_min")):
        d = R.two_phase(A, b, cost, mx, no, rule=R.DANTZIG)
        assert d["status"] == o.ITER_LIMIT and d["iters"] == g["two_phase_dantzig"]["iters"]
        q = o.two_phase(A, b, cost, mx, no)
        assert q["status"] == o.ITER_LIMIT and q["iters"] == d["iters"]
        e = R.two_phase(A, b, cost, mx, no, rule=R.BLAND)
        assert e["status"] == g[key]["status"] == o.OPTIMAL and e["iters"] == g[key]["iters"]
        assert e["basis"].tolist() == g[key]["basis"] and e["obj"] == g[key]["obj"] and e["x"].tolist() == g[key]["x"]


@pytest.mark.parametrize("m,n,seed", [(64, 128, 7), (128, 256, 7), (256, 512, 7)])
def test_cycling_family(m, n, seed):
    """Beale blocks embedded beside a random block: Dantzig's rule cycles, Bland's reaches the optimum."""
    A, b, c, basis, no = R.cycling_lp(seed, m, n)
    assert R.simplex_tableau(A, b, c, basis, True, no, rule=R.DANTZIG)["status"] == o.ITER_LIMIT
    e = R.simplex_tableau(A, b, c, basis, True, no, rule=R.BLAND)
    assert e["status"] == o.OPTIMAL and e["iters"] < capi.MAX_ITER


def test_bad_rule_and_null_handles():
    lib = capi.load()
    assert lib.lp_simplex_set_pivot_rule(None, capi.PIVOT_BLAND) == capi.BAD_ARG
    assert lib.lp_simplex_set_pivot_rule(None, 7) == capi.BAD_ARG
    assert lib.lp_batched_set_pivot_rule(None, capi.PIVOT_DANTZIG) == capi.BAD_ARG
    x = np.zeros(4)
    assert lib.lp_simplex_solve_ex(None, None, 1, 2, None, None, None, 1, 1, 1e-9, 10, capi._d(x), None, None,
                                   None, capi.PIVOT_BLAND) == capi.BAD_ARG
    assert lib.lp_simplex_two_phase_ex(None, None, 1, 2, None, None, 1, 1, 1e-9, 10, capi._d(x), None, None, None,
                                       2) == capi.BAD_ARG
    assert lib.lp_simplex_solve_batched_ex(None, 1, None, 1, 2, None, None, None, 1, 1, 1e-9, 10, capi._d(x),
                                           None, None, None, None, 3) == capi.BAD_ARG
    assert lib.lp_simplex_two_phase_batched_ex(None, 1, None, 1, 2, None, None, 1, 1, 1e-9, 10, capi._d(x), None,
                                               None, None, None, capi.PIVOT_BLAND) == capi.BAD_ARG
    assert capi.pivot_rule_id("bland") == capi.PIVOT_BLAND and capi.pivot_rule_id("Dantzig") == capi.PIVOT_DANTZIG
    with pytest.raises(ValueError):
        capi.pivot_rule_id("steepest")
