"""Writes tests/golden/bounded_parametric_cases.json: optimal objectives from scipy.optimize.linprog (HiGHS) along the
parametric right-hand-side and cost paths tests/ref/bounded_parametric_ref.c computes for boxed LPs, the independent
yardstick of tests/test_bounded_parametric_cpu.py.

Each LP is tests/bounded_parametric_ref.py's boxed_case(path, seed, m, n, maximize, kind), solved by HiGHS as
min / max c.x subject to A x = b + t d (path "rhs") or (c + t g).x subject to A x = b (path "cost") under
lo <= x <= hi, at both ends and at the midpoint of every segment of the reference's path (t_k + 1 + |t_k| for a segment
that ends at +inf) and, for a path that ends INFEASIBLE or UNBOUNDED at t*, at t* + 0.05 (1 + |t*|) just past it.  The
stored objective is null where HiGHS finds the LP infeasible or unbounded.  The file holds the generator's arguments,
the sample points and the objectives; the test regenerates the inputs from the arguments.

Run from the repo root:  python tests/golden/make_bounded_parametric_golden.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import bounded_parametric_ref as P   # noqa: E402
from scipy.optimize import linprog              # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = ((6, 14, 8), (12, 30, 6))   # m, n, cases per path


def solve(A, b, c, lo, hi, maximize):
    bounds = [(l, None if h == np.inf else h) for l, h in zip(lo, hi)]
    r = linprog(-c if maximize else c, A_eq=A, b_eq=b, bounds=bounds, method="highs")
    if r.status in (2, 3):   # infeasible, unbounded
        return None
    assert r.status == 0, r.message
    return float(c @ r.x)


def main():
    out = []
    for path in P.PATHS:
        for m, n, count in SHAPES:
            seed, taken = 1, 0
            while taken < count:
                args = dict(path=path, seed=seed, m=m, n=n, maximize=bool(taken % 2),
                            kind="ray" if taken % 4 == 3 else "mixed")
                seed += 1
                case = P.boxed_case(**args)
                if case is None:
                    continue
                taken += 1
                A, b, c, lo, hi, basis, up, direction, mx = case
                r = P.parametric(path, A, b, c, lo, hi, basis, up, direction, np.inf, mx)
                ns = r["nseg"]
                pts, seg = [], []
                for k in range(ns):
                    t0, t1 = r["t"][k], r["t"][k + 1]
                    pts += [float(t0), float(t0 + 1.0 + abs(t0)) if t1 == np.inf else float(0.5 * (t0 + t1))]
                    seg += [k, k]
                    if t1 != np.inf:
                        pts.append(float(t1))
                        seg.append(k)
                if r["status"] in (P.INFEASIBLE, P.UNBOUNDED):
                    te = r["t"][ns]
                    pts.append(float(te + 0.05 * (1.0 + abs(te))))
                    seg.append(ns)
                if path == "rhs":
                    objs = [solve(A, b + t * direction, c, lo, hi, mx) for t in pts]
                else:
                    objs = [solve(A, b, c + t * direction, lo, hi, mx) for t in pts]
                out.append(dict(args=args, status=int(r["status"]), nseg=int(ns), points=pts, segment=seg,
                                objectives=objs))
    with open(os.path.join(HERE, "bounded_parametric_cases.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", len(out), "cases,", sum(len(k["points"]) for k in out), "points")


if __name__ == "__main__":
    main()
