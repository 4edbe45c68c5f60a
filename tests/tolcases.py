"""Problem families for the tolerance tests (inputs only, like tests/lpcases.py): LPs whose pivot choices depend on the
last bits of a ratio or a reduced cost, or whose operands leave the range in which the kernels' fast reciprocals hold.

Every family is seeded and cheap.  Interesting rows and columns are placed across the kernels' boundaries: partner
offsets of 1, 63, 64, 65 (same and neighbouring 64-row waves), 255, 256 (the near-tie replay's 256-row tiles, the
chip-resident kernel's slices) and 511, 512 (its 8 / 16 slices), clipped to m - 1; column partners straddle the 16- and
32-column workgroups of the chip-resident kernel.  An offset reaches what it is meant for only where m > off: at
m <= 64 the offsets 64 and 65 are clipped to 63 and no pair reaches the batched kernels' rows l and l + 64 (the second
ratio register of wave 0).  tests/rowcases.py places the families there, at shapes of m > 64.

All LPs are in slack form [A_orig | I] with the slack basis and maximise (capi.gen_lp), so that the first pricing
sees d = c and the first ratio test the column A[:, e] against xB = b."""
import numpy as np

from simplexmethod_amd import capi

ROW_OFFSETS = (1, 63, 64, 65, 255, 256, 511, 512)
COL_OFFSETS = (1, 15, 16, 17, 31, 32, 33, 64, 255)
SCALES = (3.0, 5.0, 7.0, 0.3, 0.7, 1.1)
TINY = (1e-12, 1e-200, 1e-310, 5e-324)             # 1e-200 < 2^-500; 1e-310 and 5e-324 are subnormal
POW2 = ((300, 300), (-300, -300), (300, -600), (-300, 600), (600, -300), (-600, 300))   # (kb, kc)


def _rng(*key):
    return np.random.default_rng([0x70C, *[int(k) & 0xFFFFFFFF for k in key]])


def _clip_pair(rng, m, off):
    """Rows (p, q = p + off) inside [0, m): off is clipped to m - 1."""
    off = min(off, m - 1)
    p = int(rng.integers(0, m - off))
    return p, p + off


def _force_entering(A, c, n_orig, e):
    """Column e enters first on every eps below 1: its cost beats every other cost by more than 1."""
    c[e] = float(np.max(c[:n_orig])) + 1.5
    A[:, e] = np.maximum(A[:, e], 0.05)    # every row eligible (u >= 0.05)


def _twin_scale(a, bp, start):
    """The first scale of SCALES (in rotation from `start`) whose twin (s * a, s * bp) has a quotient strictly
    below a / bp's — so that the exact chain at eps = 0 takes the row BEHIND; None if no scale does."""
    qp = bp / a
    for t in range(len(SCALES)):
        s = SCALES[(start + t) % len(SCALES)]
        if (s * bp) / (s * a) < qp:
            return s
    return None


def near_tie_rows(seed, m, n, off, pair=None):
    """ulp near-tie rows at the first ratio test.  Row p gets the smallest ratio by a margin; row q = p + off (behind
    it) becomes its twin fl(s * row_p), b_q = fl(s * b_p) with the scale s chosen so that q's true quotient is a few
    ulp SMALLER than p's.  The reference chain takes q at eps = 0 and p at eps >= 1e-15; a ranking by approximate
    quotients may keep p.  The other rows are paired the same way at random offsets (more near-ties later on).
    pair = (p, q) fixes the two rows (off is then part of the seed alone)."""
    A, b, c, basis = capi.gen_lp(seed, m, n)
    no = n - m
    rng = _rng(1, seed, m, n, off)
    e = int(rng.integers(0, no))
    _force_entering(A, c, no, e)
    start = int(rng.integers(0, len(SCALES)))
    bmin = 0.5 * float((b / A[:, e]).min())
    for t in range(256):   # (another pair, or b_p an ulp lower, until a scale of SCALES qualifies)
        if t % 8 == 0:
            p, q = _clip_pair(rng, m, off) if pair is None else pair
            b0 = b[p]
            b[p] = bmin * A[p, e]
        s = _twin_scale(A[p, e], b[p], start)
        if s is not None:
            break
        b[p] = np.nextafter(b[p], 0.0)
        if t % 8 == 7:   # (and u_p an ulp higher)
            b[p] = b0
            A[p, e] = np.nextafter(A[p, e], np.inf)
    else:
        raise AssertionError("no twin scale found")
    A[q, :no] = s * A[p, :no]
    b[q] = s * b[p]
    # more twins among the remaining rows, so that later ratio tests meet near-ties too
    for i in rng.permutation([i for i in range(m) if i not in (p, q)])[: max(0, m // 4)]:
        j = int(i) + int(rng.choice(ROW_OFFSETS))
        if j >= m or j in (p, q):
            continue
        t = float(rng.choice(SCALES))
        A[j, :no] = t * A[i, :no]
        b[j] = t * b[i]
    return A, b, c, basis


def first_pivot_pairs(seed, count, m=64, n=96):
    """The "many small LPs" form: `count` LPs of m x n whose first ratio test is an ulp near-tie pair (p, q = p + off)
    with q's true quotient smaller (see near_tie_rows; offsets cycle through ROW_OFFSETS clipped to m).  Returns
    (A, b, c, basis) stacked along a batch axis."""
    out = [near_tie_rows(seed * 100003 + k, m, n, ROW_OFFSETS[k % len(ROW_OFFSETS)]) for k in range(count)]
    A, b, c, basis = zip(*out)
    return np.stack(A), np.stack(b), np.stack(c), np.stack(basis)


def near_tie_cols(seed, m, n, off, cols=None):
    """ulp near-tie columns: column e2 = e + off is column e with every entry and the cost moved one ulp up
    (nextafter); e has the largest cost, so at the first pricing d_e2 exceeds d_e by one ulp: the chain takes e2 at
    eps = 0 and e at eps >= 1e-15.  The pair straddles the kernels' column workgroups for the larger offsets.
    cols = (e, e2) fixes the two columns (off is then part of the seed alone)."""
    A, b, c, basis = capi.gen_lp(seed, m, n)
    no = n - m
    rng = _rng(2, seed, m, n, off)
    off = min(off, no - 1)
    e = int(rng.integers(0, no - off))
    e, e2 = (e, e + off) if cols is None else cols
    _force_entering(A, c, no, e)
    A[:, e2] = np.nextafter(A[:, e], np.inf)
    c[e2] = np.nextafter(c[e], np.inf)
    # and a few more near-duplicate column pairs at the other offsets (ties later on)
    for d in COL_OFFSETS:
        j0 = int(rng.integers(0, no))
        j1 = j0 + d
        if j1 >= no or {j0, j1} & {e, e2}:
            continue
        A[:, j1] = np.nextafter(A[:, j0], np.inf if d & 1 else -np.inf)
        c[j1] = np.nextafter(c[j0], np.inf)
    return A, b, c, basis


def exact_ties(seed, m, n):
    """Small-integer data with ties everywhere: A_orig in {0..3}, b in {0..4} (a quarter of the rows zero), c in
    {0..3}: equal ratios, equal reduced costs and degenerate pivots from the first iteration on."""
    rng = _rng(3, seed, m, n)
    no = n - m
    A = np.zeros((m, n))
    A[:, :no] = rng.integers(0, 4, size=(m, no))
    A[:, no:] = np.eye(m)
    b = rng.integers(1, 5, size=m).astype(np.float64)
    b[rng.permutation(m)[: max(1, m // 4)]] = 0.0
    c = np.zeros(n)
    c[:no] = rng.integers(0, 4, size=no)
    return A, b, c, np.arange(no, n, dtype=np.int32)


def tiny_entry(seed, m, n, u, off, pair=None):
    """A degenerate row q = p + off (b_q = 0) whose entry in the first entering column is u (TINY).  Row p holds the
    smallest positive ratio.  At eps = 0 row q is eligible with ratio 0 and leaves first (a pivot on u); at eps > u it
    is not.  Pivoting on a subnormal u fills the tableau with inf and NaN: the paths must agree on where.
    pair = (p, q) fixes the two rows (off is then part of the seed alone)."""
    A, b, c, basis = capi.gen_lp(seed, m, n)
    no = n - m
    rng = _rng(4, seed, m, n, off)
    e = int(rng.integers(0, no))
    _force_entering(A, c, no, e)
    p, q = _clip_pair(rng, m, off) if pair is None else pair
    b[p] = 0.5 * float((b / A[:, e]).min()) * A[p, e]
    A[q, e] = u
    b[q] = 0.0
    return A, b, c, basis


def huge_entries(seed, m, n):
    """Operands outside [2^-500, 2^501): rows of xB = 2^600 and 2^-600, and column entries of 2^520 (every one of
    them eligible, several of them ratio-test winners over the solve)."""
    A, b, c, basis = capi.gen_lp(seed, m, n)
    no = n - m
    rng = _rng(5, seed, m, n)
    rows = rng.permutation(m)
    k = max(1, m // 8)
    b[rows[:k]] *= 2.0 ** 600
    b[rows[k:2 * k]] *= 2.0 ** -600
    big = rows[2 * k:3 * k]
    cols = rng.integers(0, no, size=big.size)
    A[big, cols] = 2.0 ** 520
    return A, b, c, basis


def pow2_scaled(A, b, c, kb, kc):
    """b * 2^kb, c * 2^kc: at eps = 0 the pivot sequence is invariant, x scales by 2^kb and obj by 2^(kb + kc)."""
    return A, b * 2.0 ** kb, c * 2.0 ** kc


FAMILIES = ("near_rows", "near_cols", "ties", "tiny", "huge")


def family_case(family, seed, m, n, idx=0):
    """One case of a family by index (idx picks the partner offset, the scale or the tiny value)."""
    if family == "near_rows":
        return near_tie_rows(seed, m, n, ROW_OFFSETS[idx % len(ROW_OFFSETS)])
    if family == "near_cols":
        return near_tie_cols(seed, m, n, COL_OFFSETS[idx % len(COL_OFFSETS)])
    if family == "ties":
        return exact_ties(seed, m, n)
    if family == "tiny":
        return tiny_entry(seed, m, n, TINY[idx % len(TINY)], ROW_OFFSETS[(idx // len(TINY)) % len(ROW_OFFSETS)])
    if family == "huge":
        return huge_entries(seed, m, n)
    raise ValueError(family)


# ---- the single-LP grid of the tolerance tests ------------------------------------------------------------------
SHAPES = ((8, 24), (64, 160), (200, 600), (512, 1024), (768, 1536))
EPS_ALL = (0.0, -0.0, 2.0 ** -60, 1e-300, 1e-12, 1e-6, 1e-2, float("inf"))
LARGE_EPS = 1e-2
# (family, index) per shape; the offsets / tiny values they select are family_case's
_PICKS = (("near_rows", 0), ("near_rows", 2), ("near_rows", 6), ("near_cols", 0), ("near_cols", 5), ("ties", 0),
          ("tiny", 0), ("tiny", 1), ("tiny", 2), ("tiny", 23), ("huge", 0))

# the cases whose oracle trace at LARGE_EPS differs from the one at 1e-9 (they also run at LARGE_EPS)
_LARGE = {"near_rows6-8x24", "near_cols0-8x24", "huge0-64x160", "near_rows0-200x600",
          "near_rows2-512x1024", "near_rows6-512x1024", "near_rows0-768x1536", "near_rows2-768x1536",
          "near_rows6-768x1536"}


def single_cases():
    """(family, seed, m, n, idx, max_iter, large): every family at every shape.  Up to 200 x 600 every case runs to
    the end; at 512 x 1024 and 768 x 1536 the near-tie-row cases run to the end and the others stop after the first
    pivot (max_iter = 1), which pins the eps-dependent choice and keeps the oracle cheap.  `large`: the case also
    runs at LARGE_EPS (only where its oracle trace there differs from the one at 1e-9, tests/test_tolerance_cpu.py)."""
    out = []
    for si, (m, n) in enumerate(SHAPES):
        for fam, idx in _PICKS:
            full = m <= 200 or fam == "near_rows"
            large = f"{fam}{idx}-{m}x{n}" in _LARGE
            out.append((fam, 11 + si, m, n, idx, capi.MAX_ITER if full else 1, large))
    return out


def case_id(case):
    fam, seed, m, n, idx, max_iter, _ = case
    return f"{fam}{idx}-{m}x{n}-it{max_iter}"
