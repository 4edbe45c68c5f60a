"""Writes tests/golden/bounded_large_case.json: what tests/ref/bounded_ref.c returns on the 160 x 320 boxed LP that
tests/cpp/test_bounded_large_gpu.cpp builds from its seed (the same splitmix64 stream, restated here).  Data only: the
result vector (status, iters, obj, x, basis, at_upper); python's repr of a double reads back exactly through strtod.

Run from the repo root:  python tests/golden/make_bounded_large_golden.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import bounded_ref as R            # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
MASK = (1 << 64) - 1


class SplitMix:
    def __init__(self, s):
        self.s = s & MASK

    def u01(self):
        self.s = (self.s + 0x9E3779B97F4A7C15) & MASK
        z = self.s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
        z ^= z >> 31
        return float(z >> 11) * (1.0 / 9007199254740992.0)


def boxed_problem(seed, m, k):
    """test_bounded_large_gpu.cpp's boxed_problem, draw for draw."""
    g = SplitMix(seed * 7919 + 29)
    n = k + m
    A = np.zeros((m, n))
    b = np.zeros(m)
    c = np.zeros(n)
    for i in range(m):
        for j in range(k):
            A[i, j] = g.u01()
        A[i, k + i] = 1.0
        b[i] = 0.125 * k * (1.0 + g.u01())
    lo, hi = np.zeros(n), np.full(n, np.inf)
    for j in range(k):
        c[j] = g.u01() - 0.3
        q = j % 4
        if q == 1:
            hi[j] = 0.2 + 2.0 * g.u01()
        elif q == 2:
            lo[j] = hi[j] = g.u01()
        elif q == 3:
            lo[j] = -g.u01()
            hi[j] = 1.0 + g.u01()
    return A, b, c, lo, hi


if __name__ == "__main__":
    seed, m, k, maximize = 11, 160, 160, 1
    A, b, c, lo, hi = boxed_problem(seed, m, k)
    r = R.bounded(A, b, c, lo, hi, bool(maximize), m + k)
    assert r["status"] == R.OPTIMAL and r["iters"][0] > 0 and r["iters"][2] > 0 and r["iters"][3] > 0, r["iters"]
    rec = dict(name="boxed_160x320", seed=seed, m=m, k=k, maximize=maximize, status=int(r["status"]),
               iters=[int(v) for v in r["iters"]], obj=float(r["obj"]), x=[float(v) for v in r["x"]],
               basis=[int(v) for v in r["basis"]], at_upper=[int(v) for v in r["at_upper"]])
    path = os.path.join(HERE, "bounded_large_case.json")
    with open(path, "w") as f:
        f.write(json.dumps(rec) + "\n")
    print(path, os.path.getsize(path), "bytes", rec["iters"], int(sum(rec["at_upper"])))
