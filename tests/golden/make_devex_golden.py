"""Writes tests/golden/devex_cases.json: small LPs with the results tests/ref/devex_ref.c gives under Devex
pricing (rule 2), the yardstick of tests/cpp/test_devex_gpu.cpp (Solver::setPivotRule(PivotRule::Devex) on solve()
and twoPhaseSimplex()).  Data only: per case the LP (A row-major m x n, b, c, basis for the single-phase cases), the
sense, and the reference's status, pivot counts (three per case: phase I, drive-out, phase II; a single-phase run
counts as phase II), final basis, x and objective.  Every double is written with repr(), which round-trips.

Run from the repo root:  python tests/golden/make_devex_golden.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from simplexmethod_amd import capi       # noqa: E402
from tests import bland_ref as B         # noqa: E402
from tests import devex_ref as R         # noqa: E402
from tests import lpcases                # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def single(name, A, b, c, basis, maximize, no):
    r = R.simplex_tableau(A, b, c, basis, maximize, no, rule=R.DEVEX)
    return dict(name=name, two_phase=0, maximize=int(maximize), m=A.shape[0], n=A.shape[1], n_orig=no,
                A=np.asarray(A, dtype=np.float64).reshape(-1).tolist(), b=list(map(float, b)), c=list(map(float, c)),
                basis=list(map(int, basis)), status=r["status"], iters=[0, 0, r["iters"]],
                basis_out=r["basis"].tolist(), x=r["x"].tolist() if r["status"] == 0 else [],
                obj=r["obj"] if r["status"] == 0 else 0.0)


def two_phase(name, A, b, c, maximize, no):
    r = R.two_phase(A, b, c, maximize, no, rule=R.DEVEX)
    return dict(name=name, two_phase=1, maximize=int(maximize), m=A.shape[0], n=A.shape[1], n_orig=no,
                A=np.asarray(A, dtype=np.float64).reshape(-1).tolist(), b=list(map(float, b)), c=list(map(float, c)),
                basis=[], status=r["status"], iters=list(map(int, r["iters"])), basis_out=r["basis"].tolist(),
                x=r["x"].tolist() if r["status"] == 0 else [], obj=r["obj"] if r["status"] == 0 else 0.0)


def main():
    cases = []
    A, b, c, basis, no = B.beale()
    cases.append(single("beale_max", A, b, c, basis, True, no))
    A, b, c, basis = R.scaled_lp(1, 8, 20)
    cases.append(single("scaled_8x20_max", A, b, c, basis, True, 12))
    A, b, c, basis = R.scaled_lp(2, 12, 30)
    cases.append(single("scaled_12x30_min", A, b, -c, basis, False, 18))
    A, b, c, basis = capi.gen_lp(3, 16, 40)
    cases.append(single("plain_16x40_max", A, b, c, basis, True, 24))
    A, b, c, basis = R.scaled_lp(3, 8, 20)
    A[:, :4] *= -1.0   # four columns without a positive entry: a ray
    cases.append(single("unbounded_8x20", A, b, c, basis, True, 12))
    cases.append(two_phase("min_8x14", *lpcases.min_lp(1, 8, 6, equalities=1, negative_rows=2, zero_rhs=1)[:3], False, 6))
    cases.append(two_phase("scaled_min_16x40", *R.scaled_min_lp(2, 16, 24, negative_rows=2, zero_rhs=1)[:3], False, 24))
    cases.append(two_phase("scaled_min_16x40_max", *R.scaled_min_lp(1, 16, 24)[:3], True, 24))
    A, b, c, no = lpcases.degenerate_eq_lp(7)
    cases.append(two_phase("drive_out", A, b, c, False, no))
    Ai = np.array([[1.0, 1.0, 1.0, 0.0], [1.0, 1.0, 0.0, -1.0]])
    cases.append(two_phase("infeasible", Ai, np.array([1.0, 2.0]), np.array([1.0, 1.0, 0.0, 0.0]), False, 2))
    assert cases[8]["iters"][1] > 0 and cases[9]["status"] == 4 and cases[4]["status"] == 1
    with open(os.path.join(HERE, "devex_cases.json"), "w") as f:
        f.write("{\"cases\": [\n" + ",\n".join(json.dumps(q) for q in cases) + "\n]}\n")
    print(len(cases), "cases")


if __name__ == "__main__":
    main()
