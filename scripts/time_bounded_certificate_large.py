"""Time of the Farkas / unbounded-ray certificate of a bounded-variable LP beyond one workgroup's LDS
(lp_basis_bounded_certificate_large) at the basis and flags lp_simplex_bounded_large_ex (LP_PIVOT_DEVEX) stops at.
Workloads at 512 x 1024 and 2048 x 4096, from tests/bounded_ref.boxed_lp(1, m, n, kind="mixed"):
  phase1  its last row replaced by row 0 with b[-1] = b[0] + 1 (two contradicting rows): INFEASIBLE with one artificial
          basic on a mixed basis;
  ray     tests/bounded_certcases.rich_unbounded_lp: UNBOUNDED, the ray moves a column and every basic variable;
  dual    the LP itself solved to its optimum, then the lower bound of a basic column raised beyond the largest value
          lp_simplex_bounded_resolve_large finds for it (cost e_j), re-solved: INFEASIBLE after dual pivots.  The first
          DUAL_TRIES basic columns are tried; without an INFEASIBLE re-solve among them the case is recorded as missing.
Then ROUNDS alternated rounds in one session, after one warm-up round, of the certificate at each basis and of the
yardstick, lp_basis_bounded_ranging_large (existing code: the same crash on [B | I | b'] and the same B^-1 A) at the ray
LP's basis and at the LP's own optimum (every basis of original columns of the phase1 LP is singular: its A has two
equal rows): each as host wall clock of the whole call (upload, every launch, download; ends in a device
synchronise): median, min and max.  tests/ref/bounded_certificate_ref.c runs each case once on one core; the
certificates are compared with it bit for bit and checked by tests/bounded_certcases.check.

  python scripts/time_bounded_certificate_large.py [out.json]   the timed run; writes profiles/bounded_certificate_large.json
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/time_bounded_certificate_large.py --calls-only
      the solves and every call once per shape, nothing written: the kernels' own durations"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (kernel_source_hash)
from simplexmethod_amd import capi  # noqa: E402
from tests import bounded_certcases as BC  # noqa: E402
from tests import bounded_certificate_ref as CR  # noqa: E402
from tests import bounded_ref as R  # noqa: E402

SHAPES = [(512, 1024), (2048, 4096)]
ROUNDS = 5
MAX_ITER = 1000000
DUAL_TRIES = 3
OPTIMAL, UNBOUNDED, INFEASIBLE = 0, 1, 4


def _stats(ms):
    return {"ms_median": round(float(np.median(ms)), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
            "runs": len(ms)}


def _clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def _case(A, b, c, lo, hi, mx, sol):
    return dict(A=A, b=b, c=c, lo=lo, hi=hi, maximize=bool(mx), basis=sol["basis"], at_upper=sol["at_upper"],
                run=int(sol["status"]), iters=sol["iters"])


def _dual_case(ctx, A, b, c, lo, hi, mx, opt):
    """The re-solve that ends INFEASIBLE, or None."""
    m, n = A.shape
    for t in range(min(DUAL_TRIES, m)):
        j = int(opt["basis"][t])
        e = np.zeros(n)
        e[j] = 1.0
        far = ctx.bounded_resolve_large(A, b, e, lo, hi, opt["basis"], opt["at_upper"], True, max_iter=MAX_ITER)
        if far["status"] != OPTIMAL:
            continue
        lo2, hi2 = lo.copy(), hi.copy()
        lo2[j] = far["obj"] + 1.0
        hi2[j] = max(hi2[j], lo2[j] + 1.0)
        g = ctx.bounded_resolve_large(A, b, c, lo2, hi2, opt["basis"], opt["at_upper"], mx, max_iter=MAX_ITER)
        if g["status"] == INFEASIBLE:
            return _case(A, b, c, lo2, hi2, mx, g)
    return None


def _workload(ctx, m, n):
    """The cases (name -> case dict) and the yardstick calls (name -> callable)."""
    A, b, c, lo, hi, mx = R.boxed_lp(1, m, n, kind="mixed")
    opt = ctx.bounded_large(A, b, c, lo, hi, mx, max_iter=MAX_ITER, pivot_rule="devex")
    assert opt["status"] == OPTIMAL and opt["basis"].max() < n, opt["status"]
    A1, b1 = A.copy(), b.copy()
    A1[-1] = A1[0]
    b1[-1] = b1[0] + 1.0
    s1 = ctx.bounded_large(A1, b1, c, lo, hi, mx, max_iter=MAX_ITER, pivot_rule="devex")
    assert s1["status"] == INFEASIBLE, s1["status"]
    A2, b2, c2, lo2, hi2, mx2 = BC.rich_unbounded_lp(1, m, n)
    s2 = ctx.bounded_large(A2, b2, c2, lo2, hi2, mx2, max_iter=MAX_ITER, pivot_rule="devex")
    assert s2["status"] == UNBOUNDED and s2["basis"].max() < n, s2["status"]
    cases = dict(phase1=_case(A1, b1, c, lo, hi, mx, s1), ray=_case(A2, b2, c2, lo2, hi2, mx2, s2))
    dual = _dual_case(ctx, A, b, c, lo, hi, mx, opt)
    if dual is not None:
        cases["dual"] = dual
    yard = dict(ranging_large_at_the_ray_basis=lambda: ctx.bounded_ranging_large(A2, b2, c2, lo2, hi2, s2["basis"],
                                                                                 s2["at_upper"], mx2),
                ranging_large_at_the_optimum=lambda: ctx.bounded_ranging_large(A, b, c, lo, hi, opt["basis"],
                                                                               opt["at_upper"], mx))
    return cases, yard


def _at(cs):
    return cs["A"], cs["b"], cs["c"], cs["lo"], cs["hi"], cs["basis"], cs["at_upper"], cs["maximize"]


def main(path, calls_only=False):
    ctx = capi.Context(0)
    res = {"scenario": "boxed_lp(1, m, n, 'mixed') made infeasible (phase1, dual) or unbounded (ray), solved by "
                       "lp_simplex_bounded_large_ex / lp_simplex_bounded_resolve_large under LP_PIVOT_DEVEX, certified at "
                       f"the basis and flags returned; {ROUNDS} alternated rounds in one session after a warm-up round; "
                       "host wall clock of the whole call; the yardstick is lp_basis_bounded_ranging_large at a "
                       "non-singular basis of the same A (ray) or of the LP before it was changed (optimum); the "
                       "reference is tests/ref/bounded_certificate_ref.c on one core, once"}
    for m, n in SHAPES:
        cases, yard = _workload(ctx, m, n)
        print(f"{m}x{n}: {', '.join(cases)} solved", file=sys.stderr, flush=True)
        calls = {k: (lambda cs=cs: ctx.basis_bounded_certificate_large(*_at(cs))) for k, cs in cases.items()}
        calls.update(yard)
        out = {k: fn() for k, fn in calls.items()}   # warm-up: code objects, the first allocations of this size
        if calls_only:
            continue
        ms = {k: [] for k in calls}
        for _ in range(ROUNDS):
            for k, fn in calls.items():
                out[k], t = _clock(fn)
                ms[k].append(t)
        assert all(out[k]["status"] == OPTIMAL for k in yard)
        entry = dict(shape=f"{m}x{n}", dual_case="missing: none of the first %d basic columns gave an INFEASIBLE re-solve"
                     % DUAL_TRIES if "dual" not in cases else "present")
        for k in yard:
            entry[k] = _stats(ms[k])
        for k, cs in cases.items():
            want, ref_ms = _clock(lambda: CR.certificate(*_at(cs)))
            assert out[k]["status"] == want["status"] == OPTIMAL
            CR.same_bits(out[k], want)
            BC.check(cs, out[k])
            y = "ranging_large_at_the_ray_basis" if k == "ray" else "ranging_large_at_the_optimum"
            entry[k] = dict(_stats(ms[k]), solve_iters=cs["iters"], kind=out[k]["kind"], index=out[k]["index"],
                            value=out[k]["value"], artificials_basic=int((cs["basis"] >= n).sum()),
                            nonzeros=int(np.count_nonzero(out[k]["ray" if out[k]["kind"] == CR.RAY else "farkas"])),
                            over_ranging_large=round(float(np.median(ms[k]) / np.median(ms[y])), 3),
                            reference_one_core_ms=round(ref_ms, 1), equal_to_the_reference_bit_for_bit=True)
        res[f"mixed_{m}x{n}"] = entry
    ctx.close()
    if calls_only:
        return
    res["kernel_source_hash"] = bench.kernel_source_hash()
    text = json.dumps(res)
    with open(path, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--calls-only"]
    main(args[0] if args else os.path.join(ROOT, "profiles", "bounded_certificate_large.json"),
         "--calls-only" in sys.argv)
