"""Writes tests/golden/bounded_rules_cases.json: the statuses, iteration counts and objectives that
tests/ref/bounded_rules_ref.c and tests/ref/bounded_resolve_rules_ref.c give under each pivot rule (0 Dantzig, 1 Bland,
2 Devex) on LPs that the tests rebuild from their seeds: Beale's LP with boxed columns (cold and re-solved from the
slack basis, both senses), the boxed cycling LP, and bounded_ref.boxed_lp at two shapes.  Data only; every double is
written with float.hex().

Run from the repo root:  python tests/golden/make_bounded_rules_golden.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import bounded_ref as B            # noqa: E402
from tests import bounded_rules_ref as R      # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def record(name, r, **how):
    return dict(name=name, status=int(r["status"]), iters=[int(v) for v in r["iters"]],
                obj=float(r["obj"]).hex() if r["status"] == R.OPTIMAL else None, **how)


def cases():
    out = []
    A, b, c, lo, hi = R.beale_boxed()
    basis, flags = R.slack_start(A)
    for maximize in (1, 0):
        cc = c if maximize else -c
        for rule in R.RULES:
            out.append(record("beale_boxed_cold", R.bounded(A, b, cc, lo, hi, maximize, rule=rule), rule=rule,
                              maximize=maximize))
            out.append(record("beale_boxed_resolve", R.resolve(A, b, cc, lo, hi, basis, flags, maximize, rule=rule),
                              rule=rule, maximize=maximize))
    A, b, c, lo, hi = R.cycling_boxed()
    for rule in R.RULES:
        out.append(record("cycling_boxed", R.bounded(A, b, c, lo, hi, True, max_iter=2000, rule=rule), rule=rule,
                          maximize=1, max_iter=2000))
    for m, n in ((8, 20), (16, 48)):
        for seed in range(3):
            for kind in ("mixed", "box"):
                A, b, c, lo, hi, mx = B.boxed_lp(seed, m, n, kind=kind)
                for rule in R.RULES:
                    out.append(record("boxed_lp", R.bounded(A, b, c, lo, hi, mx, n - m, rule=rule), rule=rule,
                                      maximize=int(mx), m=m, n=n, seed=seed, kind=kind))
    return out


if __name__ == "__main__":
    path = os.path.join(HERE, "bounded_rules_cases.json")
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in cases()) + "\n]\n")   # one record per line
    print(path, os.path.getsize(path), "bytes")
