"""Inputs of tests/test_basis_ties_cpu.py and tests/test_gpu_basis_ties.py: bases at which the basis analyses (duals,
RHS / cost ranging, Farkas and ray certificates, plain and bounded) meet exact ties and eps edges across the seams of
their reductions.  Inputs only; test infrastructure.

Every family but crash_tie is built on integer data whose arithmetic is exact.  B = P_r (I + a subdiagonal of +-1) P_c
is totally unimodular up to signs, so the crash pivots on +-1 and B^-1 has entries 0 and +-1.  alpha itself is designed:
W (m x n, by original column, 0 in the basic columns) is chosen, A_N = B W is exact, and B^-1 A_N = W, xB, y and
d = c_N - c_B W come out as the integers that were put in.  Every ratio is then the correctly rounded quotient of two
small integers, in the C references, in a numpy model and in the kernels alike, so "the first index wins" is the only
thing that decides a reported index.  The basic columns are scattered over [0, n) in non-monotone position order.

Two kinds of column carry a single non-integer entry and stay exact in alpha all the same (B has at most two entries
per row and column, so the chain of such a column has at most two non-zero terms): W[k][j] = 0.5 and W[k][j] = 1e-9,
the latter exactly the default eps.  They make the cost ends move between 0 and 1e-9 and between 1e-9 and
nextafter(1, 0), where integer entries alone cannot; the reduced cost of a 1e-9 column is rounded, its place in a
reduction is not in doubt (its ratio is 5e9)."""
import functools

import numpy as np

EPS_GRID = (0.0, 1e-9, float(np.nextafter(1.0, 0.0)), 1.0, 2.0)   # ranging; the certificates read the first four
CERT_EPS = EPS_GRID[:4]

# 256 threads (m <= 64): two column chunks with a remainder, m % 8 = 4.  512 threads: t and t + 64 in one lane, two
# thread groups.  lp_basis_bounded_fits and lp_basis_bounded_certificate_fits end at n = 192 for m = 100, one column
# chunk, so the bounded per-workgroup forms get the tallest m > 64 with m % 8 = 4 that leaves them a second chunk with
# a remainder: 68 x 270 (n <= 278 there).  HBM_SHAPES lie beyond the plain fits (the tableau in HBM).
WG_SHAPES = {"plain": ((44, 300), (100, 280)), "bounded": ((44, 300), (68, 270))}
HBM_SHAPES = ((150, 600), (257, 1030))
CRASH_WG = (132, 140)      # the tallest m the per-workgroup ranging and certificates hold
CRASH_HBM = (1040, 1060)   # k_crash_select: rows tid and tid + 1024

FORMS = ("plain", "bounded")
_TINY = 1e-9

# (form, seed, m, n) of ranging_ties: per shape the first seed of 1..3 that meets the shares test_basis_ties_cpu.py
# asserts (the signs of B^-1 at the planted positions decide how many rows tie within one lane).  100 x 190 is the
# bounded per-workgroup form with t and t + 64 in 36 lanes: one column chunk, there for its RHS ends.
RANGING = [("plain", 2, 44, 300), ("plain", 2, 100, 280), ("plain", 2, 150, 600), ("plain", 1, 257, 1030),
           ("bounded", 1, 44, 300), ("bounded", 2, 68, 270), ("bounded", 1, 100, 190), ("bounded", 2, 150, 600),
           ("bounded", 1, 257, 1030)]
CERT_SEEDS = (1, 2)


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _frame(rng, m, n, unit_at=()):
    """(B, basis, pr, pc): B = L[pr][:, pc] with L unit lower bidiagonal (+-1 below the diagonal, 0 below the columns in
    `unit_at`, which are unit vectors then, as L's last column always is); basis: m columns of [0, n) in scattered,
    non-monotone position order."""
    sub = rng.choice([-1.0, 1.0], m - 1)
    for k in unit_at:
        sub[k] = 0.0
    L = np.eye(m) + np.diag(sub, -1)
    pr, pc = rng.permutation(m), rng.permutation(m)
    B = L[pr][:, pc]
    cols = np.sort(rng.permutation(n)[:m])
    basis = cols[rng.permutation(m)].astype(np.int32)
    return B, basis, pr, pc


class _Free:
    """Hands out non-basic columns of a range, each once."""

    def __init__(self, rng, n, basis):
        self.rng, self.free = rng, np.ones(n, bool)
        self.free[basis[basis < n]] = False

    def take(self, lo, hi, count=1, first=False):
        idx = np.flatnonzero(self.free[lo:hi]) + lo
        if len(idx) < count:
            raise ValueError("no free column in [%d, %d)" % (lo, hi))
        got = idx[:count] if first else np.sort(self.rng.choice(idx, count, replace=False))
        self.free[got] = False
        return [int(j) for j in got]


def _boxes(rng, n):
    """lo, hi, at_upper as bounded_sens_large_cases.tie draws them."""
    lo = rng.integers(-2, 1, n).astype(float)
    hi = np.where(rng.random(n) < 0.6, lo + rng.integers(2, 5, n), np.inf)
    up = ((rng.random(n) < 0.5) & np.isfinite(hi)).astype(np.int32)
    return lo, hi, up


def _assemble(B, basis, W, n):
    """A with A[:, basis[t]] = B[:, t] (structural positions) and A_N = B W."""
    A = B @ W
    for t, k in enumerate(basis):
        if k < n:
            A[:, k] = B[:, t]
    return A


def _held(lo, hi, up, basis, n):
    v = np.where(up == 1, hi, lo)
    v[basis[basis < n]] = 0.0
    return v


def _cost(rng, m, n, basis, W, d):
    """c with c_B small integers and c_N = c_B W + d."""
    cB = rng.integers(-3, 4, m).astype(float)
    cB[basis >= n] = 0.0
    c = cB @ W + d
    c[basis[basis < n]] = cB[basis < n]
    return c


# ---------------------------------------------------------------------------------------------------- ranging_ties
@functools.lru_cache(maxsize=None)
def ranging_ties(form, seed, m, n):
    """plain: (A, b, c, basis); bounded: (A, b, c, lo, hi, basis, at_upper).  xB lies 0 to 2 above its lower bound and
    B^-1's columns are +-1 down a long run, so most rows' RHS ends tie over many positions.  Three columns J with
    d = +6 and three columns K with d = -6 (every other |d| <= 5) sit in two waves of the first 256-column chunk and in
    the second chunk; about half the rows t have W[t][J] = W[t][K] = 1, so their winning cost ratio (6 over 1 when
    maximising, -6 over 1 when minimising) is attained at all three.  Four columns hold one entry 0.5 or 1e-9 each."""
    rng = np.random.default_rng([seed, m, n, FORMS.index(form), 11])
    B, basis, _, _ = _frame(rng, m, n)
    free = _Free(rng, n, basis)
    W = rng.integers(-3, 4, (m, n)).astype(float)
    W[:, basis] = 0.0
    d = rng.integers(-5, 6, n).astype(float)
    J = free.take(0, 64) + free.take(128, min(192, n)) + (free.take(256, n) if n > 256 else [])
    K = free.take(64, 128) + free.take(min(192, n - 1) - 32, min(256, n)) + (free.take(256, n) if n > 256 else [])
    rows = rng.random(m) < 0.5
    W[np.ix_(rows, J + K)] = 1.0
    d[J], d[K] = 6.0, -6.0
    F = free.take(0, n, 4)
    kF = rng.choice(m, 4, replace=False)
    W[:, F] = 0.0
    for j, k, a, dj in zip(F, kF, (0.5, 0.5, _TINY, _TINY), (5.0, -5.0, 5.0, -5.0)):
        W[k, j], d[j] = a, dj
    c = _cost(rng, m, n, basis, W, d)
    A = _assemble(B, basis, W, n)
    off = rng.integers(0, 3, m).astype(float)   # xB above its lower bound
    off[:6] = 0.0
    off[64:70] = 0.0   # positions t and t + 64 of six lanes tie at 0, the best ratio of a lower end
    if form == "plain":
        b = B @ off
        return _ro(A, b, c, basis)
    lo, hi, up = _boxes(rng, n)
    up[J + K + F] = 0
    lo[F] = 0.0   # held at 0.0: b' stays exact
    b = B @ (lo[basis] + off) + A @ _held(lo, hi, up, basis, n)
    return _ro(A, b, c, lo, hi, basis, up)


def special_columns(form, seed, m, n):
    """(fractional columns, 1e-9 columns) of ranging_ties: those whose alpha holds one non-integer entry."""
    at = ranging_ties(form, seed, m, n)
    A, basis = at[0], at[-1] if form == "plain" else at[5]
    Binv = np.rint(np.linalg.inv(A[:, basis]))
    alpha = Binv @ A
    frac = np.flatnonzero((alpha != np.rint(alpha)).any(axis=0))
    return frac, frac[np.abs(alpha[:, frac]).max(axis=0) < 0.25]


# ------------------------------------------------------------------------------------------------------- cert_dual
N_CAND = 14          # violated positions
FIRST_PASSING = 9    # the 10th candidate is the first whose row passes: the second pass of 8
ALSO_PASSING = 11    # and one later in that pass
EDGE_CAND = 4        # its only failing entry is exactly -1: it passes at eps = 1.0
UNIT_CAND = 2        # violated by exactly 1: no candidate at eps = 1.0


@functools.lru_cache(maxsize=None)
def cert_dual(form, seed, m, n):
    """The dual-simplex case.  N_CAND positions are violated (by 2 or 3, UNIT_CAND by exactly 1; bounded: alternately
    below L_t and above H_t), half of them at positions 64 and beyond when m > 64 (all four such positions at m = 68).  With sigma_t = -1 above, tau_j = -1 for a
    flagged column, candidate rows are alpha[t][j] = sigma_t tau_j G[t][j] with G >= 0 except one failing entry -2
    (EDGE_CAND: -1) per candidate, in the first, the second or the last 256-column chunk by turns; candidates
    FIRST_PASSING and ALSO_PASSING have none.  So eps < 1 reports candidate 9 and eps = 1.0 candidate 4."""
    rng = np.random.default_rng([seed, m, n, FORMS.index(form), 12])
    B, basis, _, _ = _frame(rng, m, n)
    free = _Free(rng, n, basis)
    if m > 64:
        beyond = min(N_CAND // 2, m - 64)
        cand = np.sort(np.concatenate([rng.choice(64, N_CAND - beyond, replace=False),
                                       64 + rng.choice(m - 64, beyond, replace=False)]))
    else:
        cand = np.sort(rng.choice(m, N_CAND, replace=False))
    bounded = form == "bounded"
    lo, hi, up = _boxes(rng, n) if bounded else (np.zeros(n), np.full(n, np.inf), np.zeros(n, np.int32))
    above = np.zeros(m, bool)
    if bounded:
        above[cand[1::2]] = True
        hi[basis[above]] = lo[basis[above]] + 3.0
    nonbasic = np.ones(n, bool)
    nonbasic[basis] = False
    tau = np.where((up == 1) & nonbasic, -1.0, 1.0)
    W = rng.integers(-3, 4, (m, n)).astype(float)
    G = rng.integers(0, 4, (N_CAND, n)).astype(float)
    last = 256 * ((n - 1) // 256)
    chunks = ((0, 256), (256, min(512, n)), (last, n))
    fails = {}
    for k in range(N_CAND):
        if k in (FIRST_PASSING, ALSO_PASSING):
            continue
        j = free.take(*chunks[k % 3])[0]
        G[k, j] = -1.0 if k == EDGE_CAND else -2.0
        fails[k] = j
    sigma = np.where(above[cand], -1.0, 1.0)
    W[cand] = sigma[:, None] * tau[None, :] * G
    W[:, basis] = 0.0
    L, H = lo[basis], hi[basis]
    xB = L + rng.integers(0, 3, m)
    depth = rng.integers(2, 4, N_CAND).astype(float)
    depth[UNIT_CAND] = 1.0
    xB[cand] = np.where(above[cand], H[cand] + depth, L[cand] - depth)
    c = _cost(rng, m, n, basis, W, rng.integers(-3, 4, n).astype(float))
    A = _assemble(B, basis, W, n)
    b = B @ xB + A @ _held(lo, hi, up, basis, n)
    info = dict(cand=cand, fails=fails, above=above)
    return (_ro(A, b, c, lo, hi, basis, up) if bounded else _ro(A, b, c, basis)), info


# -------------------------------------------------------------------------------------------------------- cert_ray
@functools.lru_cache(maxsize=None)
def cert_ray(form, seed, m, n, maximize):
    """The ray case: xB within its bounds.  With s = +1 (max) or -1 (min), an ordinary column holds an entry 2 somewhere
    and never qualifies.  Six columns of the first chunk improve and have alpha <= 0 except one spoiling entry.  Four have
    s d = 2 and the entry 2: in the last remainder of 8 positions for two of them, at t >= 64 (m > 64) for two.  The
    entry of `edge` and of `threshold` < `edge` is exactly 1, with s d = 2 and s d = 1.  j1 >= 256 has alpha <= 0 and
    s d = 1, the improvement threshold; j2 later in its chunk and j3 in the next chunk (n > 512) qualify with s d = 2
    and 3.  So eps < 1 reports j1 and eps = 1.0 `edge`: j1 and `threshold` improve by exactly eps then, which is not
    enough.
    bounded: the qualifying columns are unflagged with hi = +inf and negative only where H_t = +inf; three columns in
    front of j1 would qualify but for a flag, a finite hi, or a negative entry at a position with finite H_t."""
    rng = np.random.default_rng([seed, m, n, FORMS.index(form), int(maximize), 13])
    s = 1.0 if maximize else -1.0
    B, basis, _, _ = _frame(rng, m, n)
    free = _Free(rng, n, basis)
    bounded = form == "bounded"
    lo, hi, up = _boxes(rng, n) if bounded else (np.zeros(n), np.full(n, np.inf), np.zeros(n, np.int32))
    L, H = lo[basis], hi[basis]
    if bounded:
        assert np.isfinite(H).sum() >= 4 and np.isinf(H).sum() >= 4
    W = rng.integers(-3, 4, (m, n)).astype(float)
    W[rng.integers(0, m, n), np.arange(n)] = 2.0   # every ordinary column is spoiled by a 2
    d = rng.integers(-3, 4, n).astype(float)

    def clean(j, sd):
        """alpha <= 0, and 0 where H_t is finite; s d = sd; unflagged, hi = +inf"""
        W[:, j] = np.where(np.isinf(H), -rng.integers(0, 4, m).astype(float), 0.0)
        d[j] = s * sd
        up[j], hi[j] = 0, np.inf

    rem = m - (m % 8 or 8)
    spoil_at = [int(rng.integers(rem, m)), int(rng.integers(rem, m))]
    far = (64, m) if m > 64 else (8, rem)
    spoil_at += [int(rng.integers(*far)), int(rng.integers(*far))]
    spoiled = free.take(0, 256, 6)
    threshold, edge = spoiled[1], spoiled[3]
    hard = iter(spoil_at)
    for j in spoiled:
        clean(j, 1.0 if j == threshold else 2.0)
        if j in (threshold, edge):
            W[int(rng.integers(0, m)), j] = 1.0
        else:
            W[next(hard), j] = 2.0
    second = min(512, n)
    j1 = free.take(256, 256 + (second - 256) // 2)[0]
    excluded = []
    if bounded:
        excluded = free.take(0, j1, 3)
        for j in excluded:
            clean(j, 2.0)
        hi[excluded[0]] = lo[excluded[0]] + 2.0
        up[excluded[0]] = 1
        hi[excluded[1]] = lo[excluded[1]] + 2.0
        W[int(rng.choice(np.flatnonzero(np.isfinite(H)))), excluded[2]] = -2.0
    j2 = free.take(j1 + 1, second)[0]
    clean(j1, 1.0)
    clean(j2, 2.0)
    j3 = None
    if n > 512:
        j3 = free.take(512, min(768, n))[0]
        clean(j3, 3.0)
    W[:, basis] = 0.0
    xB = L + rng.integers(0, 3, m)
    c = _cost(rng, m, n, basis, W, d)
    A = _assemble(B, basis, W, n)
    b = B @ xB + A @ _held(lo, hi, up, basis, n)
    info = dict(spoiled=spoiled, spoil_at=spoil_at, edge=edge, threshold=threshold, j1=j1, j2=j2, j3=j3, excluded=excluded)
    return (_ro(A, b, c, lo, hi, basis, up) if bounded else _ro(A, b, c, basis)), info


# ----------------------------------------------------------------------------------------------------- cert_phase1
PHASE1_VARIANTS = ("none", "farkas", "edge")


@functools.lru_cache(maxsize=None)
def cert_phase1(form, seed, m, n, variant, arts):
    """The phase-I case: `arts` (1 or 2) artificials n+i are basic with value 2 each, at the positions of B's unit
    columns.  With tau_j = -1 for a flagged column their alpha rows are -tau_j G, G >= 0, so g = A^T f passes
    everywhere ("farkas"), but for one column of the last chunk at which the first artificial's row holds tau_j 2
    ("none": g fails by 2) or tau_j 1 ("edge": g = -1 exactly, decided by eps).  The rows of the basic artificials have
    b0_i >= 0 or b0_i <= -2, so the artificial columns' signs do not move with eps <= 1."""
    rng = np.random.default_rng([seed, m, n, FORMS.index(form), PHASE1_VARIANTS.index(variant), arts, 14])
    k0 = m // 2
    bounded = form == "bounded"
    B, basis, pr, pc = _frame(rng, m, n, unit_at=(k0,) if arts == 2 else ())
    basis = basis.copy()
    art_pos = []
    for k in ((m - 1, k0) if arts == 2 else (m - 1,)):
        t, r = int(np.flatnonzero(pc == k)[0]), int(np.flatnonzero(pr == k)[0])
        assert B[r, t] == 1.0 and np.count_nonzero(B[:, t]) == 1
        basis[t] = n + r
        art_pos.append(t)
    free = _Free(rng, n, basis)
    lo, hi, up = _boxes(rng, n) if bounded else (np.zeros(n), np.full(n, np.inf), np.zeros(n, np.int32))
    nonbasic = np.ones(n, bool)
    nonbasic[basis[basis < n]] = False
    tau = np.where((up == 1) & nonbasic, -1.0, 1.0)
    W = rng.integers(-3, 4, (m, n)).astype(float)
    W[art_pos] = -tau[None, :] * rng.integers(0, 4, (arts, n))
    jf = free.take(256 * ((n - 1) // 256), n)[0]
    if variant != "farkas":
        W[art_pos, jf] = 0.0
        W[art_pos[0], jf] = tau[jf] * (2.0 if variant == "none" else 1.0)
    W[:, basis[basis < n]] = 0.0
    structural = basis < n
    xB = np.full(m, 2.0)
    xB[structural] = lo[basis[structural]] + rng.integers(0, 3, int(structural.sum()))
    c = _cost(rng, m, n, basis, W, rng.integers(-3, 4, n).astype(float))
    for _ in range(4):   # the sign of an artificial column follows b0 of its row, which follows the column
        A = _assemble(B, basis, W, n)
        b = B @ xB + A @ _held(lo, hi, up, basis, n)
        b0 = b - A @ lo
        want = np.array([-1.0 if b0[basis[t] - n] < 0 else 1.0 for t in art_pos])
        have = np.array([B[basis[t] - n, t] for t in art_pos])
        if np.array_equal(want, have):
            break
        B = B.copy()
        for t, w in zip(art_pos, want):
            B[basis[t] - n, t] = w
    else:
        raise ValueError("the artificial columns' signs do not settle")
    rows = [int(basis[t] - n) for t in art_pos]
    if np.any((b0[rows] < 0) & (b0[rows] > -2)):
        raise ValueError("an artificial column's sign would move with eps")
    info = dict(art_pos=art_pos, jf=jf, b0=b0[rows])
    return (_ro(A, b, c, lo, hi, basis, up) if bounded else _ro(A, b, c, basis)), info


# ------------------------------------------------------------------------------------------------------- crash_tie
CRASH_PAIRS_WG = ((3, 67), (66, 130), (10, 75))   # one lane across row 64; one lane beyond it; two lanes across it
CRASH_PAIRS_HBM = ((5, 1029), (1030, 1035))


@functools.lru_cache(maxsize=None)
def crash_tie(m, n, p, q, seed=1):
    """(A, b, c, basis) of real-valued random data, not exact.  The column that pivots at step 0 of the crash on
    [B | I | b] (position 0) holds 1.5 in row p and -1.5 in row q, every other entry below 1; so does row 0 of B at
    positions p and q, which is the column the crash on [B^T | c_B] (the duals) scans at its step 0.  The first maximum
    is p.  Only that step is designed: a crash that took q goes on from a pivot of the other sign, and its results
    differ from the reference's through rounding."""
    rng = np.random.default_rng([seed, m, n, p, q, 15])
    A = rng.random((m, n))
    basis = rng.permutation(n)[:m].astype(np.int32)
    A[p, basis[0]], A[q, basis[0]] = 1.5, -1.5
    A[0, basis[p]], A[0, basis[q]] = 1.5, -1.5
    b = (1.0 + rng.random(m)) * (n * 0.25)
    c = rng.random(n)
    return _ro(A, b, c, basis)


# --------------------------------------------------------------------------------------------------------- batches
def stack(cases, singular_at):
    """Cases of one form and shape stacked along a batch axis; LP `singular_at` gets a repeated basis index."""
    out = [np.stack([np.asarray(case[k]) for case in cases]) for k in range(len(cases[0]))]
    basis = out[3] if len(out) == 4 else out[5]
    basis[singular_at, 1] = basis[singular_at, 0]
    return tuple(out)


def as_bounded(at):
    """A plain case in the bounded entries' arguments: lo = 0, hi = +inf, no flag."""
    A, b, c, basis = at
    n = A.shape[1]
    return A, b, c, np.zeros(n), np.full(n, np.inf), basis, np.zeros(n, np.int32)
