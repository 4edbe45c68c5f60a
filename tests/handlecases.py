"""What the batch-handle tests of the three kinds (test_gpu_batched, test_gpu_batched_two_phase, test_gpu_resolve)
share: one handle run through a tight iteration limit, the default limit and the tight one again, every download
handed back for the module's own oracle comparison, and the check that x and obj of LPs that did not reach the
optimum are left as the caller passed them."""
import numpy as np

from simplexmethod_amd import capi

SENTINEL = -12345.678


def _run(p, max_iter, counters):
    """run + download through the wrapper; with `counters` (phase_iters / resolve_iters) the per-LP counts replace
    the totals after the check that they sum to them."""
    p.run(max_iter=max_iter)
    g = p.download()
    if counters is not None:
        it = counters()
        assert np.array_equal(it.sum(axis=1), g["iters"])
        g["iters"] = it
    return g


def _assert_unwritten(p, g):
    """x and obj of the LPs that are not LP_OPTIMAL: the wrapper's pre-fill (0, NaN) in g, and the sentinel after one
    direct lp_batched_download into sentinel-filled arrays, whose other rows equal g's."""
    bad = g["status"] != capi.OPTIMAL
    assert np.all(g["x"][bad] == 0.0) and np.all(np.isnan(g["obj"][bad]))
    x = np.full((p.batch, p.n_orig), SENTINEL)
    obj = np.full(p.batch, SENTINEL)
    st = np.full(p.batch, -1, dtype=np.int32)
    assert p.ctx.lib.lp_batched_download(p.h, capi._d(x), None, capi._d(obj), None, capi._i(st)) == 0
    assert np.array_equal(st, g["status"])
    assert np.all(x[bad] == SENTINEL) and np.all(obj[bad] == SENTINEL)
    assert np.array_equal(x[~bad], g["x"][~bad]) and np.array_equal(obj[~bad], g["obj"][~bad])


def limit_default_limit(p, limit, counters=None):
    """Three runs of one handle: max_iter = limit, the default, limit again (LPs that were optimal in the second run
    stop at the limit in the third: their x and obj of the second run must not come back).  Returns the three
    downloads."""
    out = []
    for max_iter in (limit, capi.MAX_ITER, limit):
        g = _run(p, max_iter, counters)
        _assert_unwritten(p, g)
        out.append(g)
    for key in ("status", "iters", "basis", "x", "obj"):
        assert np.array_equal(out[0][key], out[2][key], equal_nan=True), key
    return out


def run_twice(p, counters=None):
    """run, download, run, download with the default limit: the two downloads, checked equal."""
    first, second = _run(p, capi.MAX_ITER, counters), _run(p, capi.MAX_ITER, counters)
    for key in ("status", "iters", "basis", "x", "obj"):
        assert np.array_equal(first[key], second[key], equal_nan=True), key
    return first, second
