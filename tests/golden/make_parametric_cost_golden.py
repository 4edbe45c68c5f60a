"""Writes tests/golden/parametric_cost_cases.json: optimal objectives from scipy.optimize.linprog (HiGHS) along the
parametric cost paths tests/ref/parametric_cost_ref.c computes, the independent yardstick of
tests/test_parametric_cost_cpu.py.

Each LP is solved in its canonical equality form, min / max (c + t g).x subject to A x = b, x >= 0, at every finite
breakpoint and at the midpoint of every segment of the reference's path (t_k + 1 + |t_k| for a segment that ends at
+inf) and, for a path that ends LP_UNBOUNDED at t*, at t* + 0.05 (1 + |t*|) just past it.  The stored objective is
null when HiGHS finds the LP unbounded there.  Inputs are regenerated from tests/parametric_cost_ref.py's named cases.

Run from the repo root:  python tests/golden/make_parametric_cost_golden.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import parametric_cost_ref as P   # noqa: E402
from scipy.optimize import linprog           # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def solve(A, b, c, maximize):
    r = linprog(-c if maximize else c, A_eq=A, b_eq=b, bounds=(0, None), method="highs")
    if r.status == 3:   # unbounded
        return None
    assert r.status == 0, r.message
    return float(c @ r.x)


def main():
    out = []
    for name, (A, b, c, basis, g, mx) in sorted(P.named_cases().items()):
        r = P.parametric_cost(A, b, c, basis, g, np.inf, mx)
        ns = r["nseg"]
        pts, seg = [], []
        for k in range(ns):
            t0, t1 = r["t"][k], r["t"][k + 1]
            pts.append(float(t0))
            seg.append(k)
            pts.append(float(t0 + 1.0 + abs(t0)) if t1 == np.inf else float(0.5 * (t0 + t1)))
            seg.append(k)
        if r["t"][ns] != np.inf:
            pts.append(float(r["t"][ns]))
            seg.append(ns - 1)
        if r["status"] == P.UNBOUNDED:
            te = r["t"][ns]
            pts.append(float(te + 0.05 * (1.0 + abs(te))))
            seg.append(ns)
        out.append(dict(name=name, status=int(r["status"]), nseg=int(ns), points=pts, segment=seg,
                        objectives=[solve(A, b, c + t * g, mx) for t in pts]))
    with open(os.path.join(HERE, "parametric_cost_cases.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", len(out), "cases,", sum(len(k["points"]) for k in out), "points")


if __name__ == "__main__":
    main()
