"""Writes tests/golden/mip_bounded_large_tall.json: what the unchanged tests/ref/mip_bounded_ref.c returns for the
1100 x 2300 problem of tests/mip_bounded_large_cases.py under its two limit pairs (about 25 s on one core).  The GPU test
compares lp_mip_bounded_solve_large with it; the CPU test regenerates it and compares bit for bit.

    python tests/golden/make_mip_bounded_large_golden.py
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from tests import mip_bounded_large_cases as Q   # noqa: E402
from tests import mip_bounded_ref as R   # noqa: E402


def main():
    args = Q.tall_args(1)
    runs = []
    for (depth, nodes) in sorted(Q.TALL_RUNS):
        r = R.mip(*args, max_depth=depth, max_nodes=nodes, max_iter=Q.TALL_MAX_ITER)
        print(depth, nodes, r["status"], r["found"], r["stats"], r["obj"], r["bound"])
        runs.append(dict(max_depth=depth, max_nodes=nodes, result=Q.pack(r)))
    with open(Q.TALL_FIXTURE, "w") as f:
        json.dump(dict(generator="tests/mip_bounded_large_cases.py: tall(1)", max_iter=Q.TALL_MAX_ITER, runs=runs), f)
        f.write("\n")


if __name__ == "__main__":
    main()
