"""Inputs of the tests of the one-LP-per-workgroup kernels on rows 64 and beyond (inputs only, built on
tests/tolcases.py and tests/tolentries.py).  Wave 0 of those kernels holds the ratios of rows lane, lane + 64,
lane + 128 and lane + 192 in registers; the families of tolcases.py are carried across that seam: near-tie pairs
(p, q = p + off) with p in the first register and q in the second or third (seam_pairs, seam_mixed), and pairs with
both rows beyond the first register (beyond_pairs).  tests/test_rows_beyond_wave_cpu.py checks
on the references that these inputs straddle the seam and depend on eps, tests/test_gpu_rows_beyond_wave.py runs them
on the GPU.

Shapes (every *_fits predicate of the entries below holds at TALL and TALLEST as they stand, except mip_fits at
TALLEST under MIP_LIMITS: the unbounded search runs at TALL alone):
  TALL     100 x 150   m in (64, 128]: the second ratio register is live (wave_ratio_select<2> where the kernel has it)
  TALLEST  130 x 140   m > 128: the third register is live (wave_ratio_select<4>), close to the LDS limit
  BENCH    128 x 256   the benchmark's shape, the plain batched entry only (no other entry fits it)

seam_mixed has EIGHT LPs, one more than tolentries.mixed: near-tie rows at 64, at 65 and at m - 1 are three picks.  The
conditions of the CPU file keep their absolute counts (at least 3 LPs differ, at most 2 cold solves not OPTIMAL ...)."""
import numpy as np

from tests import tolcases as T
from tests import tolentries as E

TALL, TALLEST, BENCH = (100, 150), (130, 140), (128, 256)
TALL_SHAPES = (TALL, TALLEST)
EPS = E.EPS


def seam_offsets(m, n):
    """The partner offsets of a shape: 63, 64, 65 around the first seam; 127, 128, 129 around the second where m > 128;
    127 at BENCH (the last row of the second register)."""
    if m > 128:
        return (63, 64, 65, 127, 128, 129)
    return (63, 64, 65, 127) if (m, n) == BENCH else (63, 64, 65)


# Seeds fixed by the conditions of tests/test_rows_beyond_wave_cpu.py under the rule of tolentries.py: the stated seed
# where it meets them, else the first of 0..31 that does.  The stated seeds are 11 and 12 for the pairs, tolentries'
# MIXED_SEED = 7 for seam_mixed, its boxed form, the parametric inputs and the dual re-solve, and 0 for the MIP batch.
PAIR_SEEDS = (11, 12)                    # condition a: both hold at every shape and offset
MIXED_SEED = {TALL: 7, TALLEST: 7, BENCH: 7}   # condition b (BENCH: no condition, the plain entry's parity alone)
BOUNDED_SEED = {TALL: 7, TALLEST: 19}    # condition c/B.  TALLEST: 19 is the only seed of 0..31 with at most 2 cold
#                                          solves not OPTIMAL at eps = 0.  TALL: no seed of 0..31 has (both subnormal
#                                          pivots end SINGULAR at eps = 0 and huge ends INFEASIBLE or a near-tie LP does):
#                                          the warm re-solve is left out at TALL, the cold solve runs on seed 7
PARAMETRIC_SEED = {TALL: 0, TALLEST: 7}  # condition c/D: at TALL seed 7 misses it
MIP_SEED = {TALL: 0, TALLEST: 1}         # condition c/C: at TALLEST seed 0 misses it
RESOLVE_SEED = {TALL: 7, TALLEST: 7}     # the dual re-solve's condition
WARM_SHAPES = (TALLEST,)                 # the shapes of the warm bounded re-solve (see BOUNDED_SEED)


def seam_pair_list(m, n):
    """[(off, seed)] of seam_pairs, in its order."""
    return [(off, seed) for off in seam_offsets(m, n) for seed in PAIR_SEEDS]


def seam_pairs(m, n):
    """The "many small LPs" form at the seam: one near_tie_rows LP per seam offset and seed, whose first ratio test is
    an ulp near-tie pair (p, q = p + off), q's true quotient the smaller.  (A, b, c, basis) stacked."""
    def make():
        cases = [T.near_tie_rows(seed, m, n, off) for off, seed in seam_pair_list(m, n)]
        return tuple(np.stack(v) for v in zip(*cases))
    return E._memo(("seam_pairs", m, n), make)


# Pairs that lie wholly beyond the first register: 64 <= p < q.  A seam pair's answer at eps > 0 is p < 64, which a
# near-tie replay that reads the first register alone still finds; here the replay has to end in the second or third
# register.  (off, seed): offsets 1 (neighbouring lanes of one register) and 17, the first two seeds of 0..31 with
# p >= 64 each; at m = 130 also 63 with the only such seed (p = 65 in the second register, q = 128 in the third).
BEYOND = {TALL: ((1, 7), (1, 10), (17, 0), (17, 3)),
          TALLEST: ((1, 0), (1, 3), (17, 0), (17, 1), (63, 14)),
          BENCH: ((1, 0), (1, 1), (17, 0), (17, 3))}


def beyond_pairs(m, n):
    """near_tie_rows LPs whose first near-tie pair lies in rows >= 64 (BEYOND): (A, b, c, basis) stacked."""
    def make():
        cases = [T.near_tie_rows(seed, m, n, off) for off, seed in BEYOND[(m, n)]]
        return tuple(np.stack(v) for v in zip(*cases))
    return E._memo(("beyond_pairs", m, n), make)


SEAM_NAMES = ("near_rows@64", "near_rows@65", "near_rows@m-1", "near_cols@17", "ties", "tiny1e-310@64",
              "tiny5e-324@65", "huge")


def seam_mixed(m, n, seed=None):
    """The batch of tolentries.mixed with seam-straddling picks (SEAM_NAMES): (A, b, c, basis) stacked."""
    seed = MIXED_SEED[(m, n)] if seed is None else seed

    def make():
        cases = [T.near_tie_rows(seed, m, n, 64), T.near_tie_rows(seed, m, n, 65), T.near_tie_rows(seed, m, n, m - 1),
                 T.near_tie_cols(seed, m, n, 17), T.exact_ties(seed, m, n), T.tiny_entry(seed, m, n, 1e-310, 64),
                 T.tiny_entry(seed, m, n, 5e-324, 65), T.huge_entries(seed, m, n)]
        return tuple(np.stack(v) for v in zip(*cases))
    return E._memo(("seam_mixed", m, n, seed), make)


def seam_boxed(m, n, seed=None):
    """seam_mixed on the seed of the bounded entries: the batch maker handed to tolentries.bounded_lps and the
    functions built on it."""
    return seam_mixed(m, n, BOUNDED_SEED[(m, n)] if seed is None else seed)


def resolve_start(m, n, eps, seed=None):
    """The dual re-solve's inputs: seam_mixed at the oracle's final bases at `eps`, each right-hand side changed as
    resolve_ref.scenario does (scale_rows), for the LPs whose cold solve is OPTIMAL: (kept indices, (A, b', c, basis)
    stacked)."""
    from tests import resolve_ref
    seed = RESOLVE_SEED[(m, n)] if seed is None else seed

    def make():
        A, b, c, _ = seam_mixed(m, n, seed)
        cold = E.same_eps_start("oracle", m, n, eps, seed, batch=seam_mixed)
        keep = [k for k, r in enumerate(cold) if r["status"] == E.OPTIMAL]
        rows = [(A[k], resolve_ref.scale_rows(10_000 + seed + k, b[k]), c[k], np.asarray(cold[k]["basis"], np.int32))
                for k in keep]
        return keep, tuple(np.stack(v) for v in zip(*rows))
    return E._memo(("dual_resolve", m, n, seed, E.eps_key(eps)), make)
