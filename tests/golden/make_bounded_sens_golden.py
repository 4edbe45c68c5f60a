"""Writes tests/golden/bounded_sens_cases.json: the dual solution of small bounded-variable LPs from
scipy.optimize.linprog (HiGHS) with bounds=, the independent yardstick of tests/test_bounded_sens_cpu.py.

Each LP is tests/bounded_ref.boxed_lp(seed, m, n): opt c.x subject to A x = b, lo <= x <= hi.  HiGHS solves min c.x,
or min -c.x for a max problem, and reports eqlin.marginals = d(fun)/d(b) and lower.marginals + upper.marginals =
d(fun)/d(bound), the reduced cost of a column held at a bound.  For a max problem both are negated, which gives the
shadow prices y = dz/db and the reduced costs d = c - A^T y of the problem as stated.  Only LPs with a non-degenerate
optimum are kept (exactly m columns strictly between their bounds by 1e-7, every other column's reduced cost beyond
1e-6 unless the column is fixed), so the basis and the dual are unique.  The file holds the generator arguments only,
plus HiGHS's objective, y and the reduced costs of the non-basic columns as [j, d_j] pairs.

Run from the repo root:  python tests/golden/make_bounded_sens_golden.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import bounded_ref as B        # noqa: E402
from scipy.optimize import linprog        # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))

cases, senses, upper, with_fixed = [], set(), 0, 0
for m, n in ((4, 12), (8, 20)):
    for seed in range(40):
        A, b, c, lo, hi, mx = B.boxed_lp(seed, m, n)
        sign = -1.0 if mx else 1.0
        r = linprog(sign * c, A_eq=A, b_eq=b, bounds=[(lo[j], None if np.isinf(hi[j]) else hi[j]) for j in range(n)],
                    method="highs")
        if r.status != 0:
            continue
        y = sign * r.eqlin.marginals
        d = sign * (r.lower.marginals + r.upper.marginals)
        inside = (r.x > lo + 1e-7) & (r.x < hi - 1e-7)
        fixed = lo == hi
        if inside.sum() != m or (np.abs(d[~inside & ~fixed]) <= 1e-6).any():
            continue
        senses.add(bool(mx))
        upper += int((~inside & ~fixed & np.isfinite(hi) & (np.abs(r.x - hi) <= 1e-9)).any())
        with_fixed += int(fixed.any())
        cases.append(dict(args=[seed, m, n], obj=float(c @ r.x), y=y.tolist(),
                          d_nonbasic=[[int(j), float(d[j])] for j in np.flatnonzero(~inside)]))
        if len([g for g in cases if g["args"][1] == m]) >= 10:
            break
assert len(cases) >= 12, len(cases)
assert senses == {True, False} and upper >= 1 and with_fixed >= 1
with open(os.path.join(HERE, "bounded_sens_cases.json"), "w") as f:
    f.write("[\n" + ",\n".join(json.dumps(case) for case in cases) + "\n]\n")
print(len(cases), "cases")
