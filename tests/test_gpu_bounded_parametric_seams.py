"""lp_basis_bounded_parametric_large and lp_basis_bounded_parametric_cost_large at near-ties across the places where
their selectors cut the work: the tau gather on 1024 threads whose wave 15 leaves early, the entering chain over row r
and the bounded ratio test over column e through block_chain_select on 960 threads (thread t holds entries t, t + 960,
t + 1920) with wave 0's replay over tiles of 1024, the staging and the in-selector bound flip with a stride of 960, and
the chain wave's held columns 256 at a time.  Every case of tests/bounded_parametric_seam_cases.py (what each one pins
is asserted on the reference alone in tests/test_bounded_parametric_seams_cpu.py) over eps in (0, 1e-12, 1e-2) and
max_breaks in (0, 1, 8), through the C ABI with every output pre-filled, against tests/ref/bounded_parametric_ref.c bit
for bit: the status, NaN and -1 fills, signed zeros, side, basis and at_upper.  max_breaks = 0 pins the blocking row or
column that leaves no trace."""
import pytest

from tests import bounded_parametric_seam_cases as S
from tests.test_gpu_bounded_parametric_large import _case, _same

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,epss", S.GRID_PARAMS, ids=S.GRID_IDS)
def test_case_equals_the_reference_over_the_grid(ctx, name, epss):
    cs = S.CASES[name]
    case = cs.make()
    for eps in epss:
        for mb in S.BREAKS:
            want = S.ref(name, case, eps, mb)
            got = _case(ctx, cs.path, case, eps=eps, max_breaks=mb)
            try:
                _same(got, want)
            except AssertionError as err:
                raise AssertionError("%s eps=%r max_breaks=%d: %s (enter %s / %s, leave %s / %s, side %s / %s)" % (
                    name, eps, mb, err, got["enter"], want["enter"], got["leave"], want["leave"], got["side"],
                    want["side"])) from err
            if mb == 0:
                if cs.path == "rhs":
                    assert got["leave"][0] >= 0 and got["side"][0] in (0, 1) and got["enter"][0] == -1
                else:
                    assert got["enter"][0] >= 0 and got["leave"][0] == -1 and got["side"][0] == -1
            elif eps in cs.first:
                assert (got["enter"][0], got["leave"][0], got["side"][0]) == cs.first[eps]


@pytest.mark.parametrize("path", sorted(S.EDGE_CASE))
def test_t_max_and_eps_edges_on_a_beyond_case(ctx, path):
    """t_max at, just above and below the first breakpoint, and eps at and just below |delta_r| (RHS) or |g_e| (cost),
    where the pinned candidate stops being one."""
    name = S.EDGE_CASE[path]
    case = S.CASES[name].make()
    ends = []
    for t_max in S.EDGE_TMAX:
        want = S.ref(name, case, 0.0, S.EDGE_BREAKS, t_max=t_max)
        _same(_case(ctx, path, case, eps=0.0, max_breaks=S.EDGE_BREAKS, t_max=t_max), want)
        ends.append(want["nseg"])
    assert ends[0] == ends[1] == 1 and ends[2] > 1
    firsts = []
    for eps in S.EDGE_EPS[path]:
        want = S.ref(name, case, eps, S.EDGE_BREAKS)
        _same(_case(ctx, path, case, eps=eps, max_breaks=S.EDGE_BREAKS), want)
        firsts.append(want["t"][1])
    assert firsts[0] == S.TAU and firsts[1] != S.TAU
