"""Inputs for the tests of the batched simplex's kernel forms (inputs only, like tests/tolcases.py): one shape per cell
of lp_batched_launch's dispatch and of the register-resident kernel's thread layouts, with the cell it is meant for.

A plain batch under Dantzig's rule runs k_batched_simplex_reg<threads, RPT> or the LDS tableau (threads = 0).  In the
register form nn = n - m non-basic columns and the right-hand side (W = nn + 1 columns) are held by G = (threads - 64)
// W row groups of RPT rows each, padded to mp = G * RPT >= m; the columns are numbered through ("plain") or assigned
wave by wave with a wave of its own for xB ("aligned": RX = ceil(m / 64) rows of xB per lane); wave 0 keeps the reduced
costs in registers for nn <= 256 ("dreg"); its ratio test holds the ratios in two registers per lane (m <= 128), in
four (m <= 256), or scans them in LDS (m > 256).  The table below is written down by hand from that arithmetic;
tests/test_batched_forms_cpu.py compares it with lp_batched_form and checks on the oracle what the inputs reach.

Per shape the batch is (a) capi.gen_lp LPs, (b) tolcases.near_tie_rows LPs whose first ratio test is an ulp near-tie
between two fixed rows on either side of a seam of the cell, (c) one tolcases.exact_ties LP."""
import functools

import numpy as np

from simplexmethod_amd import capi
from tests import tolcases

# (m, n): (threads, RPT, aligned, dreg, what the shape is there for)
FORMS = {
    (56, 120): (1024, 4, True, True, "aligned RX=1, mp = m"),
    (12, 312): (1024, 4, False, False, "plain, reduced costs in LDS"),
    (300, 310): (1024, 4, False, True, "plain, scan ratio test"),
    (160, 224): (1024, 12, True, True, "aligned RX=3, ratio<4>"),
    (24, 344): (1024, 12, True, False, "aligned G=2 CW=5, reduced costs in LDS"),
    (200, 264): (512, 44, True, True, "aligned RX=4, the sixth group is all padding"),
    (256, 320): (512, 44, True, True, "aligned RX=4, m = 256: the last aligned, the last ratio<4>"),
    (260, 324): (512, 44, False, True, "plain, scan ratio test"),
    (80, 272): (512, 44, True, True, "aligned G=2 CW=3"),
    (44, 300): (512, 44, True, True, "aligned G=1, nn = 256: the last dreg, two idle waves"),
    (40, 300): (512, 44, False, False, "plain G=1, reduced costs in LDS"),
    (136, 264): (1024, 20, True, True, "aligned RX=3, mp - m = 4"),
    (140, 268): (1024, 20, True, True, "aligned RX=3, mp = m"),
    (16, 516): (1024, 20, False, False, "plain G=1, reduced costs in LDS"),
    (20, 532): (1024, 20, True, False, "aligned G=1 CW=8, reduced costs in LDS"),
    (270, 334): (1024, 20, False, True, "plain, scan ratio test, mp - m = 10"),
    (280, 344): (1024, 20, False, True, "plain, scan ratio test, mp = m"),
    (290, 354): (0, 0, False, False, "the LDS tableau at m > 256 under Dantzig's rule"),
}
SHAPES = tuple(FORMS)

# Neighbours at which the dispatch flips: ((m, n) -> (threads, RPT)) on either side.  nn = 64: rows per thread 4 | 5,
# 12 | 13 (1024 threads) and 44 | 45, then 20 | 21; nn = 128: 44 | 45 (512 threads); W = n - m + 1 = 960 | 961.
FLIPS = (
    (((56, 120), (1024, 4)), ((57, 121), (1024, 12))),
    (((168, 232), (1024, 12)), ((169, 233), (512, 44))),
    (((264, 328), (512, 44)), ((265, 329), (1024, 20))),
    (((280, 344), (1024, 20)), ((281, 345), (0, 0))),
    (((132, 260), (512, 44)), ((133, 261), (1024, 20))),
    (((4, 963), (1024, 4)), ((4, 964), (0, 0))),
)

# The gen_lp seeds of (a).  With (b) and (c), 0..5 reach every row group and, in the forms of 4, 12 and 20 rows, every
# row-in-group index.  The 44-row forms miss one or two of the 44 indices and take the first further seed that brings
# them; 300 x 310 (75 groups of four rows, ten non-basic columns: half a dozen pivots per LP) takes the seven seeds
# below 4000 that a greedy cover of its groups picked.
SEEDS = {shape: tuple(range(6)) for shape in SHAPES}
SEEDS.update({(200, 264): (*range(6), 6), (256, 320): (*range(6), 19), (260, 324): (*range(6), 13),
              (80, 272): (*range(6), 9), (44, 300): (*range(6), 6),
              (300, 310): (*range(6), 8, 228, 358, 1664, 1882, 1921, 3785)})

EPS = (1e-9, 0.0)


def geometry(m, n):
    """dict(threads, rpt, aligned, dreg, nn, W, G, mp, RX, CW) of a register-form shape by the table; None for the LDS
    form."""
    threads, rpt, aligned, dreg, _ = FORMS[(m, n)]
    if not threads:
        return None
    nn = n - m
    G = (threads - 64) // (nn + 1)
    return dict(threads=threads, rpt=rpt, aligned=aligned, dreg=dreg, nn=nn, W=nn + 1, G=G, mp=G * rpt,
                RX=(m + 63) // 64, CW=nn // 64)


def pairs(m, n):
    """The near-tie row pairs (p, q) of (b), in order and without repeats: q = p + 1 across each seam of the cell."""
    g = geometry(m, n)
    out = []
    if g:
        out.append((g["rpt"] - 1, g["rpt"]))                 # the last row of group 0 | the first of group 1
        if g["aligned"]:
            rx = g["RX"]
            out += [(rx - 1, rx), (64 * rx - 1, 64 * rx)]    # xB's wave: lane 0 | lane 1, the last lane's last row
    if m > 256:
        out += [(63, 64), (255, 256), (m - 2, m - 1)]        # the scan's 64-row steps and its tail
    if g and g["mp"] > m:
        out.append((m - 2, m - 1))                           # the last row in front of the padding
    seen = []
    for p, q in out:
        if 0 <= p and q < m and (p, q) not in seen:
            seen.append((p, q))
    return tuple(seen)


def pair_seed(m, n, k):
    """The seed of the k-th pair's LP."""
    return 7000 + 10 * k


@functools.lru_cache(maxsize=None)
def batch(m, n):
    """(A, b, c, basis) of the whole batch (a) + (b) + (c), stacked; names(m, n) labels the LPs.  Built once per shape
    and shared: do not write into it."""
    lps = [capi.gen_lp(s, m, n) for s in SEEDS[(m, n)]]
    lps += [tolcases.near_tie_rows(pair_seed(m, n, k), m, n, 1, pair=pq) for k, pq in enumerate(pairs(m, n))]
    lps.append(tolcases.exact_ties(1, m, n))
    out = tuple(np.stack([lp[i] for lp in lps]) for i in range(4))
    for a in out:
        a.setflags(write=False)
    return out


def iteration_limit(counts):
    """A max_iter from the LPs' pivot counts that stops about half of the batch (the LPs of `limit` pivots and more)."""
    return sorted(counts)[len(counts) // 2]


def names(m, n):
    return tuple([f"gen{s}" for s in SEEDS[(m, n)]] + [f"pair{p}|{q}" for p, q in pairs(m, n)] + ["ties"])


def pair_slice(m, n):
    """The positions of the (b) LPs in batch(m, n)."""
    k = len(SEEDS[(m, n)])
    return range(k, k + len(pairs(m, n)))
