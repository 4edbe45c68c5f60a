"""GPU parity of every form and thread layout of the batched simplex: the four instantiations of the register-resident
kernel (k_batched_simplex_reg<1024, 4>, <1024, 12>, <512, 44> and <1024, 20>) in the plain and the wave-aligned column
layout, with the reduced costs in registers and in LDS, with each of the three ratio tests, with one row group, with a
row group of padding only and with idle waves behind xB's; and the LDS tableau at m > 256.  One shape per cell
(tests/batched_form_cases.py); tests/test_batched_forms_cpu.py shows on the oracle that the batches pivot in every row
group and on every row-in-group index of each cell.

Every LP against oracle.pyoracle.simplex_tableau (Bland's and the Devex rule: tests/bland_ref.py, tests/devex_ref.py):
status, pivot count, basis, vertex and objective bit for bit."""
import pytest

from oracle import pyoracle as o
from simplexmethod_amd import capi
from tests import batched_form_cases as F
from tests import test_gpu_tolerance_entries as G
from tests.test_gpu_batched import _check

pytestmark = pytest.mark.gpu

IDS = [f"{m}x{n}" for m, n in F.SHAPES]


@pytest.mark.parametrize("shape", F.SHAPES, ids=IDS)
def test_form_matches_oracle(ctx, shape):
    """The whole batch at eps 1e-9 and 0 (the near-tie pairs leave from the other side of their seam), through the
    one-call entry and the handle, which says that it ran one LP per workgroup."""
    m, n = shape
    threads, rpt, aligned, dreg, _ = F.FORMS[shape]
    assert capi.batched_form(m, n) == (True, threads, rpt, aligned, dreg)
    for eps in F.EPS:
        G.check_batched(ctx, m, n, eps, F.batch, F.names(m, n), "dantzig")


@pytest.mark.parametrize("shape", F.SHAPES, ids=IDS)
def test_form_iteration_limit(ctx, shape):
    """A limit that stops some LPs and not others: the scanning wave, the updating waves and xB's wave leave the pivot
    loop together, in the stopped workgroups and in the others; then the default limit on the same handle."""
    m, n = shape
    A, b, c, basis = F.batch(m, n)
    counts = [o.simplex_tableau(A[k], b[k], c[k], basis[k], True, n - m)["iters"] for k in range(len(A))]
    limit = F.iteration_limit(counts)
    p = ctx.batched_problem(A, b, c, basis, True, n - m)
    try:
        assert p.path() == 1
        p.run(max_iter=limit)
        stopped = p.download()
        p.run()
        full = p.download()
    finally:
        p.free()
    assert set(stopped["status"].tolist()) == {o.OPTIMAL, o.ITER_LIMIT}
    _check(stopped, A, b, c, basis, True, n - m, max_iter=limit)
    assert (full["status"] == o.OPTIMAL).all()
    _check(full, A, b, c, basis, True, n - m)


@pytest.mark.parametrize("shape", [(20, 532), (260, 324)], ids=["20x532", "260x324"])
def test_form_minimise(ctx, shape):
    """The minimise rules of the pricing on the negated costs, beside the maximise run of test_form_matches_oracle."""
    m, n = shape
    A, b, c, basis = F.batch(m, n)
    neg = 0.0 - c
    g = ctx.simplex_solve_batched(A, b, neg, basis, False, n - m)
    assert (g["iters"] > 0).all()
    _check(g, A, b, neg, basis, False, n - m)


@pytest.mark.parametrize("rule", ["bland", "devex"])
@pytest.mark.parametrize("shape", [(300, 310), (290, 354)], ids=["300x310", "290x354"])
def test_lds_form_beyond_256_rows(ctx, shape, rule):
    """Under Bland's and the Devex rule every shape runs the LDS tableau, whose ratio test scans the rows in LDS beyond
    m = 256 (check_batched asserts that the Devex weights fit)."""
    m, n = shape
    for eps in F.EPS:
        G.check_batched(ctx, m, n, eps, F.batch, F.names(m, n), rule)
