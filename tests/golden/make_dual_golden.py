"""Writes tests/golden/dual_cases.json: shadow prices of small LPs from scipy.optimize.linprog (HiGHS), the
independent yardstick of tests/test_duals_cpu.py.

Each LP is solved in its canonical equality form, min / max c.x subject to A x = b, x >= 0.  HiGHS reports
eqlin.marginals = d(fun)/d(b); fun is c.x for min problems and -c.x for max problems, so the shadow prices
y = dz/db are the marginals for min and their negatives for max.  Only LPs with a non-degenerate optimum are
kept (exactly m columns with x_j > 1e-7, every non-basic reduced cost away from zero), so the dual is unique;
the basis is those m columns.  Inputs are regenerated from the stored generator arguments (capi.gen_lp for max
problems, tests/lpcases.min_lp for min problems).

Run from the repo root:  python tests/golden/make_dual_golden.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from simplexmethod_amd import capi        # noqa: E402
from tests import lpcases                 # noqa: E402
from scipy.optimize import linprog        # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def highs(A, b, c, maximize):
    r = linprog(-c if maximize else c, A_eq=A, b_eq=b, bounds=(0, None), method="highs")
    assert r.status == 0
    y = -r.eqlin.marginals if maximize else r.eqlin.marginals
    basis = np.flatnonzero(r.x > 1e-7)
    d = c - A.T @ y
    nonbasic = np.setdiff1d(np.arange(A.shape[1]), basis)
    unique = len(basis) == A.shape[0] and np.abs(d[nonbasic]).min() > 1e-6
    return unique, basis, y, float(c @ r.x)


cases = []
for seed in range(12):
    m, n = 3 + seed % 6, 10 + 2 * seed
    A, b, c, _ = capi.gen_lp(seed, m, n)
    unique, basis, y, z = highs(A, b, c, True)
    if unique:
        cases.append(dict(kind="gen_lp", args=[seed, m, n], maximize=True, basis=basis.tolist(), y=y.tolist(), obj=z))
for seed in range(12):
    m, k = 3 + seed % 5, 4 + seed % 7
    A, b, c, _ = lpcases.min_lp(seed, m, k)
    unique, basis, y, z = highs(A, b, c, False)
    if unique:
        cases.append(dict(kind="min_lp", args=[seed, m, k], maximize=False, basis=basis.tolist(), y=y.tolist(),
                          obj=z))
assert len(cases) >= 12, len(cases)
with open(os.path.join(HERE, "dual_cases.json"), "w") as f:
    f.write("[\n" + ",\n".join(json.dumps(case) for case in cases) + "\n]\n")
print(len(cases), "cases")
