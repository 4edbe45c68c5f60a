"""The inputs of tests/test_gpu_basis_ties.py (tests/tiecases.py) are not vacuous, shown without a GPU: the integer
bases are exact, the C references (tests/ref/ranging_ref.c, bounded_sens_ref.c, certificate_ref.c,
bounded_certificate_ref.c, duals_ref.c) agree with an independent numpy model that takes the first index among the
exact winners, every condition tiecases.py claims for a family holds (asserted with counts), and the eps grid moves a
reported index or end where exact data can move one.

What exact data cannot do: a basis of integers reads the same at eps = 0, 1e-9 and nextafter(1, 0), since no |beta| or
|alpha| lies in (0, 1).  The cost ends move at those steps through the four columns that hold one entry 0.5 or 1e-9;
the RHS ends (beta is +-1 or 0) and the integer certificate cases move at 1.0 alone, and the tests say so."""
import numpy as np
import pytest

from simplexmethod_amd import capi
from tests import bounded_certificate_ref as BC
from tests import bounded_sens_ref as S
from tests import certificate_ref as PC
from tests import duals_ref as PD
from tests import ranging_ref as PR
from tests import tiecases as T

OPTIMAL = 0
NONE, FARKAS, RAY = 0, 1, 2
NEXT_BELOW_1 = T.EPS_GRID[2]


# ------------------------------------------------------------------------------------------------------- the model
class Model:
    """The exact quantities of a case given in the bounded entries' arguments (T.as_bounded for a plain one)."""

    def __init__(self, at, eps=0.0):
        A, b, c, lo, hi, basis, up = at
        self.m, self.n = m, n = A.shape
        self.at, self.basis = at, basis
        self.structural = basis < n
        self.nonbasic = np.ones(n, bool)
        self.nonbasic[basis[self.structural]] = False
        self.flag = (up == 1) & self.nonbasic
        self.v = np.where(self.nonbasic, np.where(up == 1, hi, lo), 0.0)
        bp, b0 = b - A @ self.v, b - A @ lo
        Bm = np.zeros((m, m))
        for t, k in enumerate(basis):
            if k < n:
                Bm[:, t] = A[:, k]
            else:
                Bm[k - n, t] = -1.0 if b0[k - n] < -eps else 1.0
        self.Binv = np.rint(np.linalg.inv(Bm))
        assert np.array_equal(self.Binv @ Bm, np.eye(m))   # exactness: the rounded inverse is the inverse
        assert set(np.unique(self.Binv).tolist()) <= {-1.0, 0.0, 1.0}
        self.xB = self.Binv @ bp
        self.alpha = self.Binv @ A
        self.L = np.where(self.structural, lo[np.minimum(basis, n - 1)], 0.0)
        self.H = np.where(self.structural, hi[np.minimum(basis, n - 1)], np.inf)
        cB = np.where(self.structural, c[np.minimum(basis, n - 1)], 0.0)
        self.y = self.Binv.T @ cB
        self.d = np.where(self.nonbasic, c - self.alpha.T @ cB, 0.0)
        self.x = self.v.copy()
        self.x[basis[self.structural]] = self.xB[self.structural]


def _winners(values, ok, want_max):
    """Indices of `ok` whose value is the extreme one (exact ties), ascending; empty without a candidate."""
    idx = np.flatnonzero(ok)
    if len(idx) == 0:
        return idx
    best = values[idx].max() if want_max else values[idx].min()
    return idx[values[idx] == best]


def rhs_winners(M, i, end, eps):
    """The winning basis positions of row i's lower (0) or upper (1) RHS end with their sides, ascending by 2t + side."""
    beta = M.Binv[:, i]
    use_L = (beta > eps) if end == 0 else (beta < -eps)
    use_H = ((beta < -eps) if end == 0 else (beta > eps)) & np.isfinite(M.H)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(use_L, (M.L - M.xB) / beta, (M.H - M.xB) / beta)
    return _winners(ratio, use_L | use_H, end == 0), use_H


def cost_winners(M, t, end, maximize, eps):
    """The winning columns of basic position t's lower (0) or upper (1) cost end, ascending."""
    a = M.alpha[t]
    live = M.nonbasic & (np.abs(a) > eps)
    sense = maximize != M.flag
    lower = live & ((a > eps) == sense)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = M.d / a
    return _winners(ratio, lower if end == 0 else live & ~lower, end == 0)


def model_ranging(M, maximize, eps):
    m, n = M.m, M.n
    leave, side, enter = np.full((m, 2), -1), np.full((m, 2), -1), np.full((n, 2), -1)
    for i in range(m):
        for end in (0, 1):
            win, use_H = rhs_winners(M, i, end, eps)
            if len(win):
                leave[i, end], side[i, end] = M.basis[win[0]], int(use_H[win[0]])
    for j in np.flatnonzero(M.nonbasic):
        enter[j, 1 if (maximize != M.flag[j]) else 0] = j
    for t in range(m):
        for end in (0, 1):
            win = cost_winners(M, t, end, maximize, eps)
            if len(win):
                enter[M.basis[t], end] = win[0]
    return leave, side, enter


def sign_ok(M, g, eps):
    """Step 3 of bounded_certificate_ref.c over the non-basic columns."""
    return np.where(M.flag, g <= eps, g >= -eps) | ~M.nonbasic


def dual_candidates(M, eps):
    """(position, above) of the violated positions, ascending."""
    below = M.xB < M.L - eps
    above = np.isfinite(M.H) & (M.xB > M.H + eps)
    return [(int(t), bool(above[t])) for t in np.flatnonzero(below | above)]


def ray_ok(M, j, maximize, eps):
    a = M.alpha[:, j]
    if not M.nonbasic[j] or M.flag[j] or M.at[4][j] != np.inf:
        return False
    if not np.all(a <= eps) or np.any((a < -eps) & np.isfinite(M.H)):
        return False
    return M.d[j] > eps if maximize else M.d[j] < -eps


def model_certificate(at, maximize, eps):
    """(kind, index) as bounded_certificate_ref.c decides them, on exact quantities."""
    M = Model(at, eps)
    if not M.structural.all():
        f = -M.Binv[~M.structural].sum(axis=0)
        ok = M.xB[~M.structural].sum() > eps and sign_ok(M, M.at[0].T @ f, eps).all()
        return (FARKAS if ok else NONE), -1
    cand = dual_candidates(M, eps)
    if cand:
        for t, above in cand:
            if sign_ok(M, -M.alpha[t] if above else M.alpha[t], eps).all():
                return FARKAS, t
        return NONE, -1
    for j in range(M.n):
        if ray_ok(M, j, maximize, eps):
            return RAY, j
    return NONE, -1


# ------------------------------------------------------------------------------------------------ references, once
_cache = {}


def ref_ranging(case, maximize, eps):
    k = ("r", case, maximize, eps)
    if k not in _cache:
        at = T.ranging_ties(*case)
        _cache[k] = (PR.ranging if case[0] == "plain" else S.ranging)(*at, maximize, eps)
    return _cache[k]


def ref_certificate(form, at, maximize, eps):
    return (PC.certificate if form == "plain" else BC.certificate)(*at, maximize, eps)


def bounded_args(form, at):
    return T.as_bounded(at) if form == "plain" else at


def cert_shapes(form):
    """The bounded certificates have no path beyond their fit."""
    return T.WG_SHAPES[form] + (T.HBM_SHAPES if form == "plain" else ())


# ---------------------------------------------------------------------------------------------------------- shapes
def test_the_shapes_lie_where_the_table_says():
    lib = capi.load()
    plain = (lib.lp_basis_ranging_fits, lib.lp_basis_certificate_fits)
    bounded = (lib.lp_basis_bounded_fits, lib.lp_basis_bounded_certificate_fits)
    for m, n in T.WG_SHAPES["plain"] + (T.CRASH_WG,):
        assert all(f(m, n) for f in plain), (m, n)
    for m, n in T.WG_SHAPES["bounded"]:
        assert all(f(m, n) for f in plain + bounded), (m, n)
    assert not any(f(100, 257) for f in bounded) and not any(f(76, 257) for f in bounded)   # why 68 x 270
    assert not any(f(T.CRASH_WG[0] + 1, T.CRASH_WG[0] + 1) for f in plain)                # why 132 rows
    for m, n in T.HBM_SHAPES + (T.CRASH_HBM,):
        assert not any(f(m, n) for f in plain + bounded), (m, n)
    assert lib.lp_basis_duals_fits(T.CRASH_WG[0]) and not lib.lp_basis_duals_fits(T.CRASH_HBM[0])
    for shapes in T.WG_SHAPES.values():
        assert shapes[0][0] <= 64 < shapes[1][0]   # the 256-thread and the 512-thread instantiation
        assert [m % 8 for m, _ in shapes] == [4, 4] and all(256 < n < 512 and n % 256 for _, n in shapes)


# --------------------------------------------------------------------------------------------------------- ranging
@pytest.mark.parametrize("form,seed,m,n", T.RANGING)
def test_ranging_reference_is_the_model(form, seed, m, n):
    """x, y, d and every reported index, both senses, over the eps grid."""
    at = T.ranging_ties(form, seed, m, n)
    M = Model(bounded_args(form, at))
    frac, tiny = T.special_columns(form, seed, m, n)
    assert len(frac) == 4 and len(tiny) == 2
    whole = np.ones(n, bool)
    whole[frac] = False
    assert np.array_equal(M.alpha[:, whole], np.rint(M.alpha[:, whole])) and np.abs(M.alpha).max() <= 3
    assert sorted(np.abs(M.alpha[:, frac]).max(axis=0).tolist()) == [1e-9, 1e-9, 0.5, 0.5]
    assert {1.0, 2.0, 3.0} <= set(np.unique(np.abs(M.alpha)).tolist())
    assert np.all((M.xB - M.L >= 0) & (M.xB - M.L <= 2))
    exact = np.ones(n, bool)
    exact[tiny] = False
    if form == "plain":
        g = PD.duals(*at)
    else:
        g = S.duals(*at)
        assert np.array_equal(g["x"], M.x)
    assert g["status"] == OPTIMAL and np.array_equal(g["y"], M.y)
    assert np.array_equal(g["d"][exact], M.d[exact]) and np.allclose(g["d"][tiny], M.d[tiny], rtol=0, atol=1e-6)
    for maximize in (False, True):
        for eps in T.EPS_GRID:
            q = ref_ranging((form, seed, m, n), maximize, eps)
            assert q["status"] == OPTIMAL
            leave, side, enter = model_ranging(M, maximize, eps)
            assert np.array_equal(q["b_leave"], leave) and np.array_equal(q["c_enter"], enter), (maximize, eps)
            if form == "bounded":
                assert np.array_equal(q["b_side"], side)


@pytest.mark.parametrize("form,seed,m,n", T.RANGING)
def test_ranging_ties_cross_the_seams(form, seed, m, n):
    M = Model(bounded_args(form, T.ranging_ties(form, seed, m, n)))
    eps = 1e-9
    # ---- RHS: the lower end of most rows is tied across lanes, for m > 64 also 64 positions or more apart
    tied = lanes = far = first_not_smallest = same_lane = 0
    for i in range(m):
        win, _ = rhs_winners(M, i, 0, eps)
        if len(win) < 2:
            continue
        tied += 1
        lanes += len(set((win % 64).tolist())) > 1
        far += int(win[-1] - win[0] >= 64)
        same_lane += bool(np.any((win[1:] - win[0]) % 64 == 0))
        first_not_smallest += int(M.basis[win[0]] != M.basis[win].min())
    assert 4 * lanes >= 3 * m, (tied, lanes)                            # three quarters of the rows or more
    assert 3 * first_not_smallest >= tied, (tied, first_not_smallest)   # a third of the ties or more
    if m > 64:
        # the first winner t ties with a t + 64k of its own lane in five rows or more; the winners lie 64 positions or
        # more apart in most rows (68 rows: a quarter, only four positions lie beyond 64)
        assert same_lane >= 5 and (2 * far > m or (m == 68 and 4 * far >= m)), (far, same_lane)
    # ---- cost: per remainder of 8 positions (and in the second thread group of the 512-thread form) a basic column
    # whose winning ratio is attained in two 256-column chunks and in two waves of one chunk
    for maximize in (False, True):
        hit, second_group = set(), 0
        for t in range(m):
            for end in (0, 1):
                win = cost_winners(M, t, end, maximize, eps)
                chunk, wave = win // 256, (win % 256) // 64
                waves_of_one_chunk = max((len(set(wave[chunk == k].tolist())) for k in set(chunk.tolist())), default=0)
                if (len(set(chunk.tolist())) > 1 or n <= 256) and waves_of_one_chunk > 1:
                    hit.add(t % 8)
                    second_group += (t // 8) % 2
        assert hit == set(range(8)), (maximize, hit)
        assert second_group >= 4, (maximize, second_group)


@pytest.mark.parametrize("form,seed,m,n", T.RANGING)
def test_ranging_moves_at_every_step_of_the_eps_grid(form, seed, m, n):
    """Some cost end or entering column differs between adjacent eps values in both senses; |beta| = 1 is a candidate
    below eps = 1.0 only, so the RHS ends move at that step and no other."""
    for maximize in (False, True):
        q = [ref_ranging((form, seed, m, n), maximize, eps) for eps in T.EPS_GRID]
        for a, b in zip(q, q[1:]):
            cost_same = all(np.array_equal(S.bits(a[k]), S.bits(b[k])) for k in ("c_lo", "c_hi")) and \
                np.array_equal(a["c_enter"], b["c_enter"])
            assert not cost_same
        rhs_moves = [not np.array_equal(a["b_leave"], b["b_leave"]) for a, b in zip(q, q[1:])]
        assert rhs_moves == [False, False, True, False]
        assert 2 * (q[2]["b_leave"][:, 0] >= 0).sum() > m and (q[3]["b_leave"] == -1).all()


# ---------------------------------------------------------------------------------------------- certificates: dual
@pytest.mark.parametrize("form", T.FORMS)
@pytest.mark.parametrize("seed", T.CERT_SEEDS)
def test_cert_dual(form, seed):
    for m, n in cert_shapes(form):
        at, info = T.cert_dual(form, seed, m, n)
        bat = bounded_args(form, at)
        M = Model(bat)
        cand = dual_candidates(M, 1e-9)
        pos = [t for t, _ in cand]
        assert pos == info["cand"].tolist() and len(cand) == T.N_CAND >= 12
        if m > 64:
            assert sum(t < 64 for t in pos) >= 7 and sum(t >= 64 for t in pos) >= 4
        if form == "bounded":
            assert sum(a for _, a in cand) == 7   # seven above H_t, seven below L_t
        passing, chunks = [], []
        for k, (t, above) in enumerate(cand):
            bad = np.flatnonzero(~sign_ok(M, -M.alpha[t] if above else M.alpha[t], 1e-9))
            if len(bad) == 0:
                passing.append(k)
            else:
                assert bad.tolist() == [info["fails"][k]]   # exactly one failing column
                chunks.append(int(bad[0]) // 256)
                entry = (-1.0 if above else 1.0) * (-1.0 if M.flag[bad[0]] else 1.0) * M.alpha[t, bad[0]]
                assert entry == (-1.0 if k == T.EDGE_CAND else -2.0)
        assert passing == [T.FIRST_PASSING, T.ALSO_PASSING] and T.FIRST_PASSING // 8 == T.ALSO_PASSING // 8 == 1
        earlier = chunks[:T.FIRST_PASSING]
        assert earlier.count(0) == 3 and earlier.count(1) >= 3 and earlier.count((n - 1) // 256) >= 3
        got = {}
        for eps in T.CERT_EPS:
            for maximize in (False, True):
                r = ref_certificate(form, at, maximize, eps)
                assert r["status"] == OPTIMAL and (r["kind"], r["index"]) == model_certificate(bat, maximize, eps)
            got[eps] = r["index"]
        assert got[0.0] == got[1e-9] == got[NEXT_BELOW_1] == pos[T.FIRST_PASSING]
        assert got[1.0] == pos[T.EDGE_CAND]   # the reported index moves with eps
        assert len(dual_candidates(M, 1.0)) == T.N_CAND - 1   # the position violated by exactly 1 is none at eps = 1


# ----------------------------------------------------------------------------------------------- certificates: ray
@pytest.mark.parametrize("form", T.FORMS)
@pytest.mark.parametrize("seed", T.CERT_SEEDS)
@pytest.mark.parametrize("maximize", (False, True))
def test_cert_ray(form, seed, maximize):
    s = 1.0 if maximize else -1.0
    for m, n in cert_shapes(form):
        at, info = T.cert_ray(form, seed, m, n, maximize)
        bat = bounded_args(form, at)
        M = Model(bat)
        assert np.all((M.xB >= M.L) & (M.xB <= M.H)) and not dual_candidates(M, 0.0)
        rem = m - (m % 8 or 8)
        assert len(info["spoiled"]) == 6 and max(info["spoiled"]) < 256 and info["threshold"] < info["edge"]
        spoil = []
        for j in info["spoiled"]:
            unit = j in (info["edge"], info["threshold"])
            assert s * M.d[j] == (1.0 if j == info["threshold"] else 2.0)
            t = np.flatnonzero(M.alpha[:, j] > 0)
            assert len(t) == 1 and M.alpha[t[0], j] == (1.0 if unit else 2.0)   # spoiled at one position
            if not unit:
                spoil.append(int(t[0]))
        assert sum(t >= rem for t in spoil) >= 2 and (m <= 64 or sum(t >= 64 for t in spoil) >= 2)
        j1, j2, j3 = info["j1"], info["j2"], info["j3"]
        qualifying = [j for j in range(n) if ray_ok(M, j, maximize, 1e-9)]
        assert qualifying == [j for j in (j1, j2, j3) if j is not None]
        assert j1 >= 256 and j1 // 256 == j2 // 256 and (n <= 512) == (j3 is None) and (j3 is None or j3 // 256 == 2)
        assert s * M.d[j1] == 1.0   # at the improvement threshold
        if form == "bounded":
            A, b, c, lo, hi, basis, up = at
            e = info["excluded"]
            assert max(e) < j1 and up[e[0]] == 1 and up[e[1]] == 0 and np.isfinite(hi[e[1]]) and hi[e[2]] == np.inf
            assert np.any((M.alpha[:, e[2]] < 0) & np.isfinite(M.H))
            for j in e:   # each qualifies in the plain sense
                assert np.all(M.alpha[:, j] <= 0) and s * M.d[j] == 2.0
        got = {}
        for eps in T.CERT_EPS:
            r = ref_certificate(form, at, maximize, eps)
            assert r["status"] == OPTIMAL and (r["kind"], r["index"]) == model_certificate(bat, maximize, eps)
            got[eps] = (r["kind"], r["index"], r["value"])
        assert got[0.0] == got[1e-9] == got[NEXT_BELOW_1] == (RAY, j1, s)
        assert got[1.0] == (RAY, info["edge"], 2.0 * s)   # j1 stops improving, the entry 1 stops spoiling


# ------------------------------------------------------------------------------------------- certificates: phase I
@pytest.mark.parametrize("form", T.FORMS)
@pytest.mark.parametrize("seed", T.CERT_SEEDS)
@pytest.mark.parametrize("arts", (1, 2))
def test_cert_phase1(form, seed, arts):
    for m, n in cert_shapes(form):
        for variant in T.PHASE1_VARIANTS:
            at, info = T.cert_phase1(form, seed, m, n, variant, arts)
            bat = bounded_args(form, at)
            M = Model(bat)
            basis = bat[5]
            assert (basis >= n).sum() == arts and M.xB[basis >= n].tolist() == [2.0] * arts   # a positive sum
            assert np.all((info["b0"] >= 0) | (info["b0"] <= -2))
            g = bat[0].T @ -M.Binv[basis >= n].sum(axis=0)
            bad = np.flatnonzero(~sign_ok(M, g, 1e-9))
            if variant == "farkas":
                assert len(bad) == 0
            else:
                assert bad.tolist() == [info["jf"]] and info["jf"] // 256 == (n - 1) // 256   # one column, last chunk
                assert abs(g[bad[0]]) == (2.0 if variant == "none" else 1.0)
            kinds = []
            for eps in T.CERT_EPS:
                r = ref_certificate(form, at, False, eps)
                assert r["status"] == OPTIMAL and r["index"] == -1
                assert (r["kind"], -1) == model_certificate(bat, False, eps)
                kinds.append(r["kind"])
            assert kinds == {"none": [NONE] * 4, "farkas": [FARKAS] * 4, "edge": [NONE] * 3 + [FARKAS]}[variant]


# ------------------------------------------------------------------------------------------------------- crash_tie
@pytest.mark.parametrize("shape,pairs,seam", [(T.CRASH_WG, T.CRASH_PAIRS_WG, 64), (T.CRASH_HBM, T.CRASH_PAIRS_HBM, 1024)])
def test_crash_tie(shape, pairs, seam):
    m, n = shape
    kinds = set()
    for p, q in pairs:
        A, b, c, basis = T.crash_tie(m, n, p, q)
        B = A[:, basis]
        for line in (B[:, 0], B[0, :]):   # step 0 of the crash on [B | I | b], and of the one on [B^T | c_B]
            mag = np.abs(line)
            assert mag[p].tobytes() == mag[q].tobytes() and line[p] == -line[q] > 0
            assert np.flatnonzero(mag == mag.max()).tolist() == [p, q] and p < q < m
        kinds.add("straddles" if p < seam <= q else "beyond" if p >= seam else "lane")
        # p and q differ in their lane, or share it on either side of the seam: both are asked for
        kinds.add("same lane" if (q - p) % 64 == 0 else "lanes")
    assert {"straddles", "beyond", "same lane", "lanes"} <= kinds
    if m < 200:
        A, b, c, basis = T.crash_tie(m, n, *pairs[0])
        st, binv, xb = PR.crash(A, b, basis, 0)
        assert st == OPTIMAL and np.allclose(binv @ A[:, basis], np.eye(m), atol=1e-8)


def test_batches_differ_from_their_neighbours():
    for m, n in T.WG_SHAPES["plain"]:
        cases = [T.ranging_ties("plain", 1, m, n), T.cert_dual("plain", 1, m, n)[0],
                 T.cert_ray("plain", 1, m, n, True)[0]]
        A, b, c, basis = T.stack(cases, 1)
        assert A.shape == (3, m, n) and basis[1, 0] == basis[1, 1] and basis[0, 0] != basis[0, 1]
        assert PR.ranging(A[1], b[1], c[1], basis[1])["status"] == 3   # SINGULAR
