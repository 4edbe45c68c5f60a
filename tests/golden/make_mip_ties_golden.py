"""Writes tests/golden/mip_ties_tall.json: what the unchanged tests/ref/mip_bounded_ref.c returns for the 1100 x 2200
problem of tests/mip_tie_cases.py (tall_case) at max_depth = 1 (about 6 s on one core).  The GPU test compares
lp_mip_bounded_solve_large with it; the CPU test regenerates it and compares bit for bit.

    python tests/golden/make_mip_ties_golden.py
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from tests import mip_bounded_ref as R   # noqa: E402
from tests import mip_tie_cases as K   # noqa: E402


def main():
    r = R.mip(*K.bounded_args(K.tall_case()), **K.TALL_RUN)
    print(r["status"], r["found"], r["stats"], r["obj"], r["bound"])
    with open(K.TALL_FIXTURE, "w") as f:
        json.dump(dict(generator="tests/mip_tie_cases.py: tall_case()", run=K.TALL_RUN, result=K.pack(r)), f)
        f.write("\n")


if __name__ == "__main__":
    main()
