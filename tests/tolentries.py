"""Inputs of the tolerance tests of the entries added after tests/tolcases.py (inputs only): Devex pricing, the
bounded-variable re-solve, branch-and-bound over bounds, the parametric right-hand side and the parametric cost.
Everything is built on tolcases.family_case; tests/test_tolerance_entries_cpu.py checks on the references that these
inputs depend on eps, tests/test_gpu_tolerance_entries.py runs them on the GPU.

Two shapes: 16 x 48 (a tableau of at most 4096 doubles: the four-wave instantiation of the one-LP-per-workgroup
kernels) and a sixteen-wave shape with m <= 64, 64 x 160 unless a condition of the CPU file needs 32 x 96.

A composite entry starts from a result of another solve.  That solve is run by the cold reference at the SAME eps
as the entry (same_eps_start): a basis that is optimal at 1e-9 is often no valid start at eps = 0."""
import numpy as np

from oracle import pyoracle as o
from tests import bounded_ref, mip_bounded_ref, parametric_cost_ref, parametric_ref
from tests import bounded_resolve_ref as W
from tests import tolcases as T

OPTIMAL = 0
SMALL, LARGE = (16, 48), (64, 160)
SHAPES = (SMALL, LARGE)
EPS = (0.0, 1e-12, 1e-2)               # the grid of every composite entry
EPS_SMALL_ONLY = (-0.0, float("inf"))   # added at 16 x 48
EPS_DEFAULT = 1e-9
BAD_EPS = (-1e-9, -np.inf, np.nan)

PICKS = (("near_rows", 0), ("near_rows", 6), ("near_cols", 5), ("ties", 0), ("tiny", 1), ("tiny", 3), ("huge", 0))
NAMES = tuple(f"{f}{i}" for f, i in PICKS)
MIXED_SEED = 7

# Seeds fixed by the conditions of tests/test_tolerance_entries_cpu.py: the stated seed where it meets them, else the
# first of 0..31 that does.
PARAMETRIC_SEED = {SMALL: 7, LARGE: 5}   # group D: at 64 x 160 seed 7 leaves no LP with a path at eps = 0
MIP_SEED = {SMALL: 1, LARGE: 0}          # group C: at 16 x 48 seed 0 has no LP whose stats differ at 1e-2
MIP_LIMITS = dict(max_depth=12, max_nodes=300)

_CACHE = {}


def eps_grid(shape):
    return EPS + (EPS_SMALL_ONLY if tuple(shape) == SMALL else ())


def eps_key(eps):
    return np.float64(eps).tobytes()


def _memo(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def mixed(m, n, seed=MIXED_SEED):
    """The seven picks of test_gpu_tolerance._mixed, stacked: (A, b, c, basis)."""
    def make():
        cases = [T.family_case(f, seed, m, n, i) for f, i in PICKS]
        return tuple(np.stack(v) for v in zip(*cases))
    return _memo(("mixed", m, n, seed), make)


def two_phase_form(A, b, c):
    """The family LPs without their basis, some rows negated (b < 0: the two-phase row flip)."""
    A, b = A.copy(), b.copy()
    A[..., ::5, :] *= -1.0
    b[..., ::5] *= -1.0
    return A, b, c


def boxes(shape, m, seed=5):
    """The box recipe of test_gpu_tolerance.test_bounded_batched: lo = 0, each hi +inf or U(0.5, 4) with equal
    chance, the m slacks unbounded.  shape = c.shape."""
    rng = np.random.default_rng(seed)
    lo = np.zeros(shape)
    hi = np.where(rng.random(shape) < 0.5, np.inf, rng.uniform(0.5, 4.0, shape))
    hi[..., shape[-1] - m:] = np.inf
    return lo, hi


# ---- Devex ----------------------------------------------------------------------------------------------------------
SCALED = (("near_cols", 3, 5), ("ties", 3, 0))   # (family, seed, idx) at 64 x 160, eps = 0
SCALED_DIFFERENT, SCALED_SAME = (600, -600), (300, -300)   # c * 2^k: the squared scores leave fp64 / stay inside


def scaled_cost_case(fam, seed, idx, k, m=64, n=160):
    A, b, c, basis = T.family_case(fam, seed, m, n, idx)
    return A, b, c * 2.0 ** k, basis


# ---- the start of a composite entry ---------------------------------------------------------------------------------
def bounded_lps(m, n, batch=mixed):
    """The LPs of batch(m, n) with the box recipe: (A, b, c, lo, hi), stacked."""
    A, b, c, _ = batch(m, n)
    lo, hi = boxes(c.shape, m)
    return A, b, c, lo, hi


def start_eps(eps):
    """The eps of the cold bounded solve behind an entry run at `eps`: eps itself, except +inf, at which the bounded
    two-phase flow ends SINGULAR on every LP (no pivot element exceeds +inf) and no start exists; the entry is then run
    at +inf from the start of the default eps."""
    return EPS_DEFAULT if eps == np.inf else eps


def same_eps_start(kind, m, n, eps, seed=MIXED_SEED, batch=mixed):
    """The cold reference solves of a batch at `eps`, once per (kind, batch maker, shape, eps bits):
      "oracle"   batch(m, n, seed) from the slack basis by the oracle: a list of its result dicts;
      "bounded"  bounded_lps(m, n, batch) by bounded_ref.bounded at start_eps(eps) with the full vertex (n_orig = n).
    batch: the maker of the LPs, mixed or another of its signature (tests/rowcases.py)."""
    def make():
        if kind == "oracle":
            A, b, c, basis = batch(m, n, seed)
            return [o.simplex_tableau(A[k], b[k], c[k], basis[k], True, n - m, eps=eps) for k in range(len(A))]
        if kind == "bounded":
            A, b, c, lo, hi = bounded_lps(m, n, batch)
            return [bounded_ref.bounded(A[k], b[k], c[k], lo[k], hi[k], True, n, eps=start_eps(eps))
                    for k in range(len(A))]
        raise ValueError(kind)
    return _memo(("start", kind, batch.__name__, m, n, seed, eps_key(eps)), make)


# ---- bounded re-solve -----------------------------------------------------------------------------------------------
PERTURB_SEED = {"bound": 3, "rhs": 3, "cost": 5}   # (cost: seeds 0..4 give no bound flip at some shape and eps)


def resolve_batch(m, n, eps, kind, batch=mixed):
    """The warm starts of the LPs whose cold solve at start_eps(eps) is OPTIMAL, perturbed by
    bounded_resolve_ref.perturb(PERTURB_SEED[kind], kind): (kept indices, (A, b', c', lo', hi', basis, at_upper)
    stacked)."""
    def make():
        A, b, c, lo, hi = bounded_lps(m, n, batch)
        cold = same_eps_start("bounded", m, n, eps, batch=batch)
        keep = [k for k, r in enumerate(cold) if r["status"] == OPTIMAL]
        rows = []
        for k in keep:
            r = cold[k]
            b2, c2, lo2, hi2 = W.perturb(PERTURB_SEED[kind], kind, b[k], c[k], lo[k], hi[k], r["basis"], r["x"])
            rows.append((A[k], b2, c2, lo2, hi2, r["basis"], r["at_upper"]))
        return keep, tuple(np.stack(v) for v in zip(*rows))
    return _memo(("resolve", batch.__name__, m, n, eps_key(eps), kind), make)


def resolve_ref(m, n, eps, kind, batch=mixed):
    """bounded_resolve_ref.resolve on every LP of resolve_batch at `eps` (sense max, n_orig = n - m)."""
    def make():
        _, warm = resolve_batch(m, n, eps, kind, batch)
        return [W.resolve(*(w[k] for w in warm), True, n - m, eps=eps) for k in range(len(warm[0]))]
    return _memo(("resolve_ref", batch.__name__, m, n, eps_key(eps), kind), make)


# ---- bounded MIP ----------------------------------------------------------------------------------------------------
MIP_TIES = 5   # the first five LPs of a batch come from exact_ties, the last two from near_tie_rows


def boxed_mip_ties(m, n, seed):
    """Seven tolerance-family LPs with the box recipe, every other structural column integer and the marked columns'
    bounds rounded outward as mip_bounded_ref.boxed_mip does.  Sense max.  The first MIP_TIES are exact_ties (seeds
    7 seed .. 7 seed + 4) with b + 0.5: still small-integer ratios and costs with ties everywhere, but no row of
    b = 0 and fractional vertices, so that the search branches (with b itself every LP is solved at its root).  The
    last two are near_tie_rows (offsets 1 and 255 clipped).  Returns (A, b, c, lo, hi) stacked and the mask (n)."""
    def make():
        cases = [T.exact_ties(7 * seed + k, m, n)[:3] for k in range(MIP_TIES)]
        cases = [(A, b + 0.5, c) for A, b, c in cases]
        cases += [T.family_case("near_rows", seed, m, n, i)[:3] for i in (0, 6)]
        A, b, c = (np.stack(v) for v in zip(*cases))
        lo, hi = boxes(c.shape, m, seed=100 + seed)
        mask = np.zeros(n, dtype=np.int32)
        mask[0:n - m:2] = 1
        for j in np.flatnonzero(mask):
            lo[:, j] = np.floor(lo[:, j])
            hi[:, j] = np.where(np.isfinite(hi[:, j]), np.ceil(hi[:, j]), hi[:, j])
        return A, b, c, lo, hi, mask
    return _memo(("mip", m, n, seed), make)


def mip_ref(m, n, eps, seed=None):
    """Per LP of boxed_mip_ties: the root by bounded_ref.bounded at start_eps(eps), and mip_bounded_ref.mip from it under
    MIP_LIMITS (None where the root is not OPTIMAL).  A list of (root, result)."""
    seed = MIP_SEED[(m, n)] if seed is None else seed

    def make():
        A, b, c, lo, hi, mask = boxed_mip_ties(m, n, seed)
        out = []
        for k in range(len(A)):
            root = bounded_ref.bounded(A[k], b[k], c[k], lo[k], hi[k], True, n - m, eps=start_eps(eps))
            r = None
            if root["status"] == OPTIMAL:
                r = mip_bounded_ref.mip(A[k], b[k], c[k], lo[k], hi[k], root["basis"], root["at_upper"], mask, True,
                                        n - m, eps=eps, **MIP_LIMITS)
            out.append((root, r))
        return out
    return _memo(("mip_ref", m, n, seed, eps_key(eps)), make)


# ---- parametric right-hand side and cost ----------------------------------------------------------------------------
MAX_BREAKS = 64


def parametric_inputs(m, n, eps, seed=None, batch=mixed):
    """batch(m, n, seed) at the oracle's final bases at `eps`: (A, b, c, basis, d, g, run_status) with
    d = parametric_ref.direction(1, b), g = parametric_cost_ref.direction(1, c) per LP."""
    seed = PARAMETRIC_SEED[(m, n)] if seed is None else seed

    def make():
        A, b, c, _ = batch(m, n, seed)
        cold = same_eps_start("oracle", m, n, eps, seed, batch)
        basis = np.stack([np.asarray(r["basis"], np.int32) for r in cold])
        status = np.array([r["status"] for r in cold], np.int32)
        d = np.stack([parametric_ref.direction(1, bk) for bk in b])
        g = np.stack([parametric_cost_ref.direction(1, ck) for ck in c])
        return A, b, c, basis, d, g, status
    return _memo(("parametric", batch.__name__, m, n, seed, eps_key(eps)), make)


def parametric_refs(m, n, eps, which, seed=None, handle=False, batch=mixed):
    """parametric_ref.parametric_batched ("rhs") or parametric_cost_ref.parametric_cost_batched ("cost") on
    parametric_inputs.  handle: the form after a batched run, in which an LP whose cold solve is not OPTIMAL keeps that
    status; otherwise every basis is given to the reference as it is."""
    seed = PARAMETRIC_SEED[(m, n)] if seed is None else seed

    def make():
        A, b, c, basis, d, g, status = parametric_inputs(m, n, eps, seed, batch)
        rs = status if handle else None
        if which == "rhs":
            return parametric_ref.parametric_batched(A, b, c, basis, d, np.inf, True, eps, MAX_BREAKS, rs)
        return parametric_cost_ref.parametric_cost_batched(A, b, c, basis, g, np.inf, True, eps, MAX_BREAKS, rs)
    return _memo(("parametric_ref", which, batch.__name__, m, n, seed, eps_key(eps), handle), make)
