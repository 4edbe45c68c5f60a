"""Writes tests/golden/mip_bounded_snapshots_tall.json: what tests/ref/mip_bounded_snapshots_ref.c returns for
mip_bounded_large_cases.tall_args(1) (1100 x 2300, 1200 marked columns) at the depth, node budget and snapshot count of
tests/mip_bounded_snapshots_cases.py, the floats as hex strings.  About half a minute on a CPU (the root alone is 4368
primal pivots on a 1101 x 2301 tableau); the GPU test compares against the recorded result.  Run from the repository
root:  python tests/golden/make_mip_bounded_snapshots_golden.py"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from tests import mip_bounded_large_cases as Q   # noqa: E402
from tests import mip_bounded_snapshots_cases as SC   # noqa: E402
from tests import mip_bounded_snapshots_ref as S   # noqa: E402


def main():
    r = S.mip(*Q.tall_args(1), max_depth=SC.TALL_DEPTH, max_nodes=SC.TALL_NODES, max_iter=Q.TALL_MAX_ITER,
              snapshots=SC.TALL_SNAPSHOTS)
    data = dict(problem="mip_bounded_large_cases.tall_args(1)", shape=list(Q.TALL_SHAPE), max_iter=Q.TALL_MAX_ITER,
                max_depth=SC.TALL_DEPTH, max_nodes=SC.TALL_NODES, snapshots=SC.TALL_SNAPSHOTS, result=Q.pack(r))
    with open(SC.TALL_FIXTURE, "w") as f:
        json.dump(data, f, indent=1)
        f.write("\n")
    print(SC.TALL_FIXTURE, r["status"], r["stats"])


if __name__ == "__main__":
    main()
