"""Writes tests/golden/ranging_cases.json: optimal objectives from scipy.optimize.linprog (HiGHS) with one b_i or
c_j moved just inside and just outside the range tests/ref/ranging_ref.c computes, the independent yardstick of
tests/test_ranging_cpu.py.

Each LP is solved in its canonical equality form, min / max c.x subject to A x = b, x >= 0.  Only LPs with a
non-degenerate unique optimum are kept (exactly m columns with x_j > 1e-7, every non-basic reduced cost away from
zero), so the basis is those m columns and every range is tight.  For each finite end e of the range of v (b_i or
c_j, current value v0), the points v0 + (1 - 1e-3) (e - v0) (inside) and e + 0.05 (1 + |e - v0|) sign(e - v0)
(outside) are re-solved; the stored objective is null when HiGHS finds the moved LP infeasible or
unbounded.  Inside the range
the objective is the line z + y_i (b_i - v0) or z + x_j (c_j - v0); outside it leaves that line.  Inputs are
regenerated from the stored generator arguments (capi.gen_lp for max problems, tests/lpcases.min_lp for min).

Run from the repo root:  python tests/golden/make_ranging_golden.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from simplexmethod_amd import capi        # noqa: E402
from tests import lpcases                 # noqa: E402
from tests import ranging_ref as RR       # noqa: E402
from scipy.optimize import linprog        # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def solve(A, b, c, maximize):
    r = linprog(-c if maximize else c, A_eq=A, b_eq=b, bounds=(0, None), method="highs")
    if r.status in (2, 3):   # infeasible, unbounded
        return None, None
    assert r.status == 0, r.message
    return float(c @ r.x), r


def unique_optimum(A, b, c, maximize):
    z, r = solve(A, b, c, maximize)
    y = -r.eqlin.marginals if maximize else r.eqlin.marginals
    basis = np.flatnonzero(r.x > 1e-7)
    d = c - A.T @ y
    nonbasic = np.setdiff1d(np.arange(A.shape[1]), basis)
    return len(basis) == A.shape[0] and np.abs(d[nonbasic]).min() > 1e-6, basis.astype(np.int32), z


def points(A, b, c, maximize, basis):
    rg = RR.ranging(A, b, c, basis, maximize)
    assert rg["status"] == 0
    out = []
    for what, v0s, lo, hi in (("b", b, rg["b_lo"], rg["b_hi"]), ("c", c, rg["c_lo"], rg["c_hi"])):
        for k in range(len(v0s)):
            for side, e in ((0, lo[k]), (1, hi[k])):
                if not np.isfinite(e):
                    continue
                v0 = float(v0s[k])
                s = 1.0 if e >= v0 else -1.0
                vin = v0 + (1 - 1e-3) * (e - v0)
                vout = float(e) + 0.05 * (1 + abs(e - v0)) * s
                objs = []
                for v in (vin, vout):
                    bb, cc = b.copy(), c.copy()
                    (bb if what == "b" else cc)[k] = v
                    objs.append(solve(A, bb, cc, maximize)[0])
                out.append(dict(what=what, k=k, side=side, inside=[vin, objs[0]], outside=[vout, objs[1]]))
    return out


cases = []
for seed in range(12):
    m, n = 3 + seed % 6, 10 + 2 * seed
    A, b, c, _ = capi.gen_lp(seed, m, n)
    unique, basis, z = unique_optimum(A, b, c, True)
    if unique:
        cases.append(dict(kind="gen_lp", args=[seed, m, n], maximize=True, basis=basis.tolist(), obj=z,
                          points=points(A, b, c, True, basis)))
for seed in range(12):
    m, k = 3 + seed % 5, 4 + seed % 7
    A, b, c, _ = lpcases.min_lp(seed, m, k)
    unique, basis, z = unique_optimum(A, b, c, False)
    if unique:
        cases.append(dict(kind="min_lp", args=[seed, m, k], maximize=False, basis=basis.tolist(), obj=z,
                          points=points(A, b, c, False, basis)))
assert len(cases) >= 12, len(cases)
with open(os.path.join(HERE, "ranging_cases.json"), "w") as f:
    f.write("[\n" + ",\n".join(json.dumps(case) for case in cases) + "\n]\n")
print(len(cases), "cases,", sum(len(g["points"]) for g in cases), "points")
