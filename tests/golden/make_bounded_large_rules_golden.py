"""Writes tests/golden/bounded_large_rules_cases.json for tests/cpp/bounded_large_rules_gpu.cpp: what
tests/ref/bounded_rules_ref.c returns under Devex pricing on the 160 x 320 boxed LP of make_bounded_large_golden.py, and
the cycling boxed LP of tests/bounded_rules_ref.py (its structural block, b and costs: numpy draws them, so the program
cannot restate it) with what the reference returns on it under Bland's rule.  Data only; python's repr of a double reads
back exactly through strtod.

Run from the repo root:  python tests/golden/make_bounded_large_rules_golden.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import bounded_rules_ref as RR                               # noqa: E402
from tests.golden.make_bounded_large_golden import boxed_problem        # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_ITER = 10000   # Solver::MAX_ITER


def floats(a):
    return [float(v) for v in a]


def ints(a):
    return [int(v) for v in a]


if __name__ == "__main__":
    seed, m, k, maximize = 11, 160, 160, 1
    A, b, c, lo, hi = boxed_problem(seed, m, k)
    r = RR.bounded(A, b, c, lo, hi, bool(maximize), m + k, max_iter=MAX_ITER, rule=RR.DEVEX)
    d = RR.bounded(A, b, c, lo, hi, bool(maximize), m + k, max_iter=MAX_ITER, rule=RR.DANTZIG)
    assert r["status"] == RR.OPTIMAL and r["iters"][0] > 0 and r["iters"][2] > 0 and r["iters"][3] > 0, r["iters"]
    assert r["iters"] != d["iters"]
    rec = dict(dev_seed=seed, dev_m=m, dev_k=k, dev_maximize=maximize, dev_status=int(r["status"]),
               dev_iters=ints(r["iters"]), dev_obj=float(r["obj"]), dev_x=floats(r["x"]), dev_basis=ints(r["basis"]),
               dev_at_upper=ints(r["at_upper"]))

    A, b, c, lo, hi = RR.cycling_boxed()
    cm, cn = A.shape
    assert (A[:, cn - cm:] == np.eye(cm)).all() and not c[cn - cm:].any()
    assert RR.bounded(A, b, c, lo, hi, True, max_iter=MAX_ITER, rule=RR.DANTZIG)["status"] == RR.ITER_LIMIT
    r = RR.bounded(A, b, c, lo, hi, True, max_iter=MAX_ITER, rule=RR.BLAND)
    assert r["status"] == RR.OPTIMAL
    rec.update(cyc_m=cm, cyc_n=cn, cyc_hi=float(hi[0]), cyc_A0=floats(A[:, :cn - cm].reshape(-1)), cyc_b=floats(b),
               cyc_c0=floats(c[:cn - cm]), cyc_status=int(r["status"]), cyc_iters=ints(r["iters"]),
               cyc_obj=float(r["obj"]), cyc_x=floats(r["x"]), cyc_basis=ints(r["basis"]),
               cyc_at_upper=ints(r["at_upper"]))
    path = os.path.join(HERE, "bounded_large_rules_cases.json")
    with open(path, "w") as f:
        f.write(json.dumps(rec) + "\n")
    print(path, os.path.getsize(path), "bytes", rec["dev_iters"], rec["cyc_iters"])
