"""The bounded-variable re-solve on the GPU (lp_simplex_bounded_resolve, lp_simplex_bounded_resolve_batched): status, x,
obj, basis, at_upper and the three counters equal tests/ref/bounded_resolve_ref.c's bit for bit on several shapes, both
senses and both block sizes, on a 4096-LP batch of 64 x 192 after a change of bounds, on a batch that reaches every
outcome; with lo = 0, hi = inf and no flag the batch equals lp_simplex_resolve_batched; and the refusals (a flag on a
column without an upper bound, a flag that is not 0 or 1, a basis index out of range, a null pointer)."""
import ctypes as C

import numpy as np
import pytest

from simplexmethod_amd import capi
from tests import bounded_ref as B
from tests import bounded_resolve_ref as W
from tests import resolve_ref
from tests.test_gpu_bounded import _bits_equal, _row, _same

pytestmark = pytest.mark.gpu

OPTIMAL, UNBOUNDED, ITER_LIMIT, SINGULAR, INFEASIBLE, BAD_ARG = 0, 1, 2, 3, 4, 5


def _warm_batch(ctx, cases, maximize, kinds):
    """Cold-solves the LPs (A, b, c, lo, hi) on the GPU and perturbs those that were optimal, LP k by kinds[k].  Returns
    the stacked warm starts (A, b', c', lo', hi', basis, at_upper) of the optimal ones and how many there were."""
    A, b, c, lo, hi = (np.stack([cs[i] for cs in cases]) for i in range(5))
    cold = ctx.bounded_batched(A, b, c, lo, hi, maximize)
    keep = np.flatnonzero(cold["status"] == OPTIMAL)
    b2, c2, lo2, hi2 = b.copy(), c.copy(), lo.copy(), hi.copy()
    for k in keep:
        b2[k], c2[k], lo2[k], hi2[k] = W.perturb(int(k), kinds[k], b[k], c[k], lo[k], hi[k], cold["basis"][k],
                                                 cold["x"][k])
    return (A[keep], b2[keep], c2[keep], lo2[keep], hi2[keep], cold["basis"][keep], cold["at_upper"][keep]), len(keep)


def _check_batch(out, warm, maximize, n_orig=None, max_iter=10000):
    for k in range(len(warm[0])):
        r = W.resolve(*(w[k] for w in warm), maximize, n_orig, max_iter=max_iter)
        _same(_row(out, k), r)
        yield r


@pytest.mark.parametrize("m,n", [(4, 12), (8, 20), (16, 48), (32, 96), (48, 120)])
@pytest.mark.parametrize("maximize", [True, False])
def test_shapes_both_senses_and_block_sizes(ctx, m, n, maximize):
    # (m+1)(n+1) <= 4096: four waves ((4, 12), (8, 20), (16, 48)); the others sixteen
    cases = [B.boxed_lp(seed, m, n, maximize)[:5] for seed in range(12)]
    warm, kept = _warm_batch(ctx, cases, maximize, [W.PERTURBATIONS[k % 3] for k in range(12)])
    assert kept >= 9
    out = ctx.bounded_resolve_batched(*warm, maximize, n - m)
    res = list(_check_batch(out, warm, maximize, n - m))
    assert any(r["iters"][0] > 0 for r in res)
    for k in range(0, kept, 3):   # a single LP is a batch of one
        r = res[k]
        if r["status"] == BAD_ARG:
            continue
        _same(ctx.bounded_resolve(*(w[k] for w in warm), maximize, n - m), r)


def test_batch_of_4096_64x192(ctx):
    Bn, m, n = 4096, 64, 192
    cases = [B.boxed_lp(k, m, n, maximize=True, kind="box" if k % 4 == 1 else "mixed")[:5] for k in range(Bn)]
    warm, kept = _warm_batch(ctx, cases, True, ["bound"] * Bn)
    assert kept >= 4000
    out = ctx.bounded_resolve_batched(*warm, True)
    res = list(_check_batch(out, warm, True))
    assert sum(r["status"] == OPTIMAL and r["iters"][0] > 0 for r in res) >= kept // 2
    assert sum(r["status"] == INFEASIBLE for r in res) >= 1


def test_batch_reaches_every_outcome(ctx):
    max_iter = 3
    cases = W.outcome_cases(max_iter=max_iter)
    warm = [np.stack([cs[i] for _, cs, _ in cases]) for i in range(7)]
    out = ctx.bounded_resolve_batched(*warm, True, max_iter=max_iter)
    assert list(out["status"]) == [OPTIMAL, OPTIMAL, INFEASIBLE, INFEASIBLE, UNBOUNDED, ITER_LIMIT, SINGULAR, BAD_ARG]
    assert list(out["status"]) == [st for _, _, st in cases]
    list(_check_batch(out, warm, True, max_iter=max_iter))
    names = [name for name, _, _ in cases]
    for name in ("crossed", "singular", "no_valid_start"):   # the given basis and flags come back
        k = names.index(name)
        assert np.array_equal(out["basis"][k], warm[5][k]) and np.array_equal(out["at_upper"][k], warm[6][k])
        assert not out["iters"][k].any()
    assert np.all(np.isnan(out["x"][2:])) and np.all(np.isnan(out["obj"][2:]))


@pytest.mark.parametrize("m,n", [(8, 20), (32, 96)])
@pytest.mark.parametrize("maximize", [True, False])
def test_identity_anchor_equals_resolve_batched(ctx, m, n, maximize):
    Bn = 64
    A, b, b2, c, slack = resolve_ref.scenario(Bn, m, n)
    if not maximize:
        c = -c
    cold = ctx.resolve_batched(A, b, c, slack, maximize)
    assert np.all(cold["status"] == OPTIMAL)
    basis = cold["basis"].copy()
    basis[::8] = slack[::8]   # some start from the slack identity: no crash, the primal loop
    lo, hi, up = np.zeros((Bn, n)), np.full((Bn, n), np.inf), np.zeros((Bn, n), np.int32)
    g = ctx.bounded_resolve_batched(A, b2, c, lo, hi, basis, up, maximize, n - m)
    t = ctx.resolve_batched(A, b2, c, basis, maximize, n - m)
    assert np.array_equal(g["status"], t["status"])
    assert np.array_equal(g["basis"], t["basis"])
    assert np.array_equal(g["iters"][:, :2], t["iters"])
    assert not g["iters"][:, 2].any() and not g["at_upper"].any()
    assert (t["iters"][:, 0] > 0).any() and (t["iters"][:, 1] > 0).any()
    ok = t["status"] == OPTIMAL
    assert ok.any()
    _bits_equal(g["x"][ok], t["x"][ok])
    _bits_equal(g["obj"][ok], t["obj"][ok])


def test_refusals(ctx):
    A, b, c, lo, hi, mx = B.boxed_lp(1, 6, 16)
    cold = ctx.bounded(A, b, c, lo, hi, mx)
    assert cold["status"] == OPTIMAL
    basis, up = cold["basis"], cold["at_upper"]
    two = lambda v: np.stack([v, v])   # noqa: E731

    def refused(basis2, up2, lo2=lo, hi2=hi):
        assert W.resolve(A, b, c, lo2, hi2, basis2, up2, mx)["status"] == BAD_ARG
        with pytest.raises(capi.LPError) as e:
            ctx.bounded_resolve(A, b, c, lo2, hi2, basis2, up2, mx)
        assert e.value.code == BAD_ARG
        with pytest.raises(capi.LPError) as e:   # a bad start in any LP refuses the whole batch
            ctx.bounded_resolve_batched(two(A), two(b), two(c), np.stack([lo, lo2]), np.stack([hi, hi2]),
                                        np.stack([basis, basis2]), np.stack([up, up2]), mx)
        assert e.value.code == BAD_ARG

    bad = up.copy()
    bad[int(np.flatnonzero(np.isinf(hi))[0])] = 1
    refused(basis, bad)
    bad = up.copy()
    bad[0] = 2
    refused(basis, bad)
    for index in (-1, 16):
        bad = basis.copy()
        bad[3] = index
        refused(bad, up)
    lo2 = lo.copy()
    lo2[2] = -np.inf
    refused(basis, up, lo2=lo2)
    hi2 = hi.copy()
    hi2[2] = np.nan
    refused(basis, np.zeros(16, np.int32), hi2=hi2)
    # a basis that is no valid start: an error for one LP, a status in a batch
    cases = W.outcome_cases(max_iter=3)
    name, cs, st = cases[-1]
    assert name == "no_valid_start" and st == BAD_ARG
    with pytest.raises(capi.LPError) as e:
        ctx.bounded_resolve(*cs, True)
    assert e.value.code == BAD_ARG
    m, n = 160, 320
    assert not ctx.bounded_fits(m, n)
    with pytest.raises(capi.LPError) as e:
        ctx.bounded_resolve(np.eye(m, n), np.ones(m), np.zeros(n), np.zeros(n), np.ones(n), np.arange(m),
                            np.zeros(n, np.int32))
    assert e.value.code == BAD_ARG
    lib = ctx.lib
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    Af = capi.colmajor(A)
    z = np.zeros(64)
    zi = np.zeros(64, np.int32)
    d = lambda a: a.ctypes.data_as(dp)   # noqa: E731
    i = lambda a: a.ctypes.data_as(ip)   # noqa: E731
    basis, up = np.ascontiguousarray(basis, np.int32), np.ascontiguousarray(up, np.int32)
    assert lib.lp_simplex_bounded_resolve(ctx.h, d(Af), 6, 16, d(b), d(c), d(lo), d(hi), None, i(up), int(mx), 16, 1e-9,
                                          100, d(z), i(zi), i(zi), d(z), i(zi)) == BAD_ARG
    assert lib.lp_simplex_bounded_resolve(ctx.h, d(Af), 6, 16, d(b), d(c), d(lo), d(hi), i(basis), None, int(mx), 16,
                                          1e-9, 100, d(z), i(zi), i(zi), d(z), i(zi)) == BAD_ARG
    assert lib.lp_simplex_bounded_resolve(ctx.h, d(Af), 6, 16, d(b), d(c), d(lo), d(hi), i(basis), i(up), int(mx), 16,
                                          -1.0, 100, d(z), i(zi), i(zi), d(z), i(zi)) == BAD_ARG
    assert lib.lp_simplex_bounded_resolve_batched(ctx.h, 1, d(Af), 6, 16, d(b), d(c), d(lo), d(hi), i(basis), i(up),
                                                  int(mx), 16, 1e-9, 100, d(z), i(zi), i(zi), d(z), i(zi),
                                                  None) == BAD_ARG
    assert lib.lp_simplex_bounded_resolve_batched(ctx.h, 0, d(Af), 6, 16, d(b), d(c), d(lo), d(hi), i(basis), i(up),
                                                  int(mx), 16, 1e-9, 100, d(z), i(zi), i(zi), d(z), i(zi),
                                                  i(zi)) == BAD_ARG
    # the context still works after the refusals
    _same(ctx.bounded_resolve(A, b, c, lo, hi, basis, up, mx), W.resolve(A, b, c, lo, hi, basis, up, mx))
