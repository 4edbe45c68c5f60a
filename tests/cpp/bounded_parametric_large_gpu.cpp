// GPU tests of Solver::boundedParametricRhsLarge and Solver::boundedParametricCostLarge: after
// Solver::boundedSimplexLarge on 160 x 320 boxed LPs (beyond lp_basis_bounded_parametric_fits) both paths equal the C
// entries lp_basis_bounded_parametric_large / _cost_large bit for bit and tests/ref/bounded_parametric_ref.c's (the
// library named by LP_BOUNDED_PARAMETRIC_REF, loaded at run time), while the LDS methods refuse the shape; at a shape
// that fits they equal Solver::boundedParametricRhs / boundedParametricCost; a result that is not optimal keeps its
// status without segments, a repeated basis index is singular, crossed bounds are infeasible without segments, and a bad
// flag, index or direction size throws std::invalid_argument.  (No test_ prefix:
// tests/test_bounded_parametric_large_cpp.py runs this program.)
#include <cmath>
#include <cstdint>
#include <limits>

#include "check.h"
#include "fixtures.h"
#include "Canonical.h"
#include "SimplexSolover.h"

using lpla::MatrixXd;
using lpla::VectorXd;

static const double INF = std::numeric_limits<double>::infinity();
static const int MB = Solver::MAX_BREAKS;

// fixtures.h's boxed_problem with seeded directions of mixed signs: d (m) scaled by b, g (n)
static Canonical problem(uint64_t seed, int m, int k, bool maximize, MatrixXd* A, VectorXd* b, VectorXd* c,
                         std::vector<double>* lo, std::vector<double>* hi, VectorXd* d, VectorXd* g) {
    Canonical can = boxed_problem(seed, m, k, maximize, A, b, c, lo, hi, /*a_offset=*/0.05, /*b_scale=*/0.125);
    uint64_t s = seed * 104729 + 7;
    *d = VectorXd::Zero(m);
    *g = VectorXd::Zero(k + m);
    for (int i = 0; i < m; ++i) (*d)[i] = (2.0 * u01(s) - 1.0) * (*b)[i];
    for (int j = 0; j < k + m; ++j) (*g)[j] = 2.0 * u01(s) - 1.0;
    return can;
}

typedef int (*Entry)(lp_context*, const double*, int, int, const double*, const double*, const double*, const double*,
                     const int*, const int*, int, const double*, double, double, int, int*, double*, double*, double*,
                     int*, int*, int*, int*, int*);
typedef int (*RefEntry)(const double*, int, int, const double*, const double*, const double*, const double*, const int*,
                        const int*, int, const double*, double, double, int, int*, double*, double*, double*, int*,
                        int*, int*, int*, int*);

// One path in the padded layout of the C entries
struct Padded {
    int status = -1, nseg = -7;
    std::vector<double> t, obj, slope;
    std::vector<int> enter, leave, side, basis, up;
    Padded(int m, int n) : t(MB + 2), obj(MB + 2), slope(MB + 1), enter(MB + 1), leave(MB + 1), side(MB + 1),
                           basis((size_t)m), up((size_t)n) {}
};

static void same_padded(const Padded& a, const Padded& w) {
    CHECK(a.status == w.status && a.nseg == w.nseg);
    for (size_t k = 0; k < w.t.size(); ++k) CHECK(same_bits(a.t[k], w.t[k]) && same_bits(a.obj[k], w.obj[k]));
    for (size_t k = 0; k < w.slope.size(); ++k) CHECK(same_bits(a.slope[k], w.slope[k]));
    CHECK(a.enter == w.enter && a.leave == w.leave && a.side == w.side && a.basis == w.basis && a.up == w.up);
}

// the mirror's path against a padded one; returns the breakpoints whose leaving variable stops at its upper bound
static int compare(const Solver::BoundedParametric& g, const Padded& w) {
    CHECK(g.status == w.status);
    const int ns = w.nseg;
    CHECK((int)g.slope.size() == ns && (int)g.t.size() == (ns ? ns + 1 : 0) && (int)g.obj.size() == (ns ? ns + 1 : 0));
    CHECK((int)g.enter.size() == ns && (int)g.leave.size() == ns && (int)g.side.size() == ns);
    if ((int)g.slope.size() != ns || (int)g.side.size() != ns) return 0;
    int upper = 0;
    for (int k = 0; k < ns; ++k) {
        CHECK(same_bits(g.t[k], w.t[(size_t)k]) && same_bits(g.obj[k], w.obj[(size_t)k]));
        CHECK(same_bits(g.slope[k], w.slope[(size_t)k]));
        CHECK(g.enter[(size_t)k] == w.enter[(size_t)k] && g.leave[(size_t)k] == w.leave[(size_t)k]);
        CHECK(g.side[(size_t)k] == w.side[(size_t)k]);
        upper += g.side[(size_t)k] == 1;
    }
    if (ns) CHECK(same_bits(g.t[ns], w.t[(size_t)ns]) && same_bits(g.obj[ns], w.obj[(size_t)ns]));
    CHECK(g.basis == w.basis && g.atUpper == w.up);
    return upper;
}

static void same_paths(const Solver::BoundedParametric& a, const Solver::BoundedParametric& w) {
    CHECK(a.status == w.status && a.t.size() == w.t.size() && a.slope.size() == w.slope.size());
    if (a.t.size() != w.t.size() || a.slope.size() != w.slope.size()) return;
    for (int k = 0; k < (int)w.t.size(); ++k) CHECK(same_bits(a.t[k], w.t[k]) && same_bits(a.obj[k], w.obj[k]));
    for (int k = 0; k < (int)w.slope.size(); ++k) CHECK(same_bits(a.slope[k], w.slope[k]));
    CHECK(a.enter == w.enter && a.leave == w.leave && a.side == w.side && a.basis == w.basis && a.atUpper == w.atUpper);
}

TEST(BoundedParametricLarge_MatchesTheCEntryAndTheRef) {
    const RefLib lib("LP_BOUNDED_PARAMETRIC_REF");
    const RefEntry refs[2] = {lib.symbol<RefEntry>("ref_bounded_parametric"),
                              lib.symbol<RefEntry>("ref_bounded_parametric_cost")};
    const Entry entries[2] = {lp_basis_bounded_parametric_large, lp_basis_bounded_parametric_cost_large};
    const int M = 160, K = 160, N = M + K;
    CHECK(lp_basis_bounded_parametric_fits(M, N) == 0 && lp_basis_bounded_parametric_cost_fits(M, N) == 0);
    lp_context* ctx = lpgpu::context(0);
    int paths = 0, breaks = 0, upper = 0;
    for (uint64_t seed = 1; seed <= 2; ++seed) {
        const bool maximize = seed % 2 == 0;
        MatrixXd A;
        VectorXd b, c, d, g;
        std::vector<double> lo, hi;
        Solver s(problem(seed, M, K, maximize, &A, &b, &c, &lo, &hi, &d, &g));
        const Solver::BoundedResult r = s.boundedSimplexLarge(lo, hi, /*throw_on_failure=*/false);
        CHECK(r.status == LP_OPTIMAL);
        if (r.status != LP_OPTIMAL) continue;
        for (int cost = 0; cost < 2; ++cost) {
            const VectorXd& dir = cost ? g : d;
            for (double tMax : {INF, 0.05}) {
                const Solver::BoundedParametric got =
                    cost ? s.boundedParametricCostLarge(lo, hi, r, dir, tMax) : s.boundedParametricRhsLarge(lo, hi, r, dir, tMax);
                Padded viaC(M, N), want(M, N);
                viaC.status = entries[cost](ctx, A.data(), M, N, b.data(), c.data(), lo.data(), hi.data(), r.basis.data(),
                                            r.atUpper.data(), maximize ? 1 : 0, dir.data(), tMax, Solver::EPS, MB,
                                            &viaC.nseg, viaC.t.data(), viaC.obj.data(), viaC.slope.data(),
                                            viaC.enter.data(), viaC.leave.data(), viaC.side.data(), viaC.basis.data(),
                                            viaC.up.data());
                want.status = refs[cost](A.data(), M, N, b.data(), c.data(), lo.data(), hi.data(), r.basis.data(),
                                         r.atUpper.data(), maximize ? 1 : 0, dir.data(), tMax, Solver::EPS, MB, &want.nseg,
                                         want.t.data(), want.obj.data(), want.slope.data(), want.enter.data(),
                                         want.leave.data(), want.side.data(), want.basis.data(), want.up.data());
                same_padded(viaC, want);
                upper += compare(got, viaC);
                ++paths;
                breaks += (int)got.slope.size() - 1;
            }
            // the LDS methods refuse this shape
            if (cost) CHECK_THROWS(s.boundedParametricCost(lo, hi, r, dir, INF), std::invalid_argument);
            else CHECK_THROWS(s.boundedParametricRhs(lo, hi, r, dir, INF), std::invalid_argument);
        }
    }
    std::printf("  %d paths, %d breakpoints, %d at an upper bound\n", paths, breaks, upper);
    CHECK(paths == 8 && breaks >= 60 && upper >= 5);
}

TEST(BoundedParametricLarge_EqualsTheLdsMethodsWhereBothRun) {
    const int M = 9, K = 14, N = M + K;
    CHECK(lp_basis_bounded_parametric_fits(M, N) == 1 && lp_basis_bounded_parametric_cost_fits(M, N) == 1);
    int paths = 0;
    for (uint64_t seed = 0; seed < 6; ++seed) {
        const bool maximize = seed % 2 == 0;
        MatrixXd A;
        VectorXd b, c, d, g;
        std::vector<double> lo, hi;
        Solver s(problem(seed, M, K, maximize, &A, &b, &c, &lo, &hi, &d, &g));
        const Solver::BoundedResult r = s.boundedSimplex(lo, hi, /*throw_on_failure=*/false);
        if (r.status != LP_OPTIMAL) continue;
        for (double tMax : {INF, 0.4}) {
            same_paths(s.boundedParametricRhsLarge(lo, hi, r, d, tMax), s.boundedParametricRhs(lo, hi, r, d, tMax));
            same_paths(s.boundedParametricCostLarge(lo, hi, r, g, tMax), s.boundedParametricCost(lo, hi, r, g, tMax));
            paths += 2;
        }
    }
    CHECK(paths >= 12);
}

TEST(BoundedParametricLarge_StatusesAndExceptions) {
    const int M = 160, K = 160, N = M + K;
    MatrixXd A;
    VectorXd b, c, d, g;
    std::vector<double> lo, hi;
    Solver s(problem(2, M, K, true, &A, &b, &c, &lo, &hi, &d, &g));
    const Solver::BoundedResult r = s.boundedSimplexLarge(lo, hi, /*throw_on_failure=*/false);
    CHECK(r.status == LP_OPTIMAL);
    const Solver::BoundedParametric good = s.boundedParametricRhsLarge(lo, hi, r, d, INF);
    CHECK(good.slope.size() >= 1);
    Solver::BoundedResult failed = r;
    failed.status = LP_INFEASIBLE;   // a result that is not optimal keeps its status and gets no segments
    const Solver::BoundedParametric none = s.boundedParametricCostLarge(lo, hi, failed, g, INF);
    CHECK(none.status == LP_INFEASIBLE && none.slope.size() == 0 && none.t.size() == 0 && none.basis == r.basis);
    Solver::BoundedResult rep = r;
    rep.basis[1] = rep.basis[0];     // repeated index: singular
    const Solver::BoundedParametric e = s.boundedParametricRhsLarge(lo, hi, rep, d, INF);
    CHECK(e.status == LP_SINGULAR && e.slope.size() == 0 && e.basis == rep.basis && e.atUpper == rep.atUpper);
    std::vector<double> crossed = hi;
    crossed[3] = lo[3] - 1.0;        // crossed bounds: infeasible without segments, also with the repeat
    const Solver::BoundedParametric x = s.boundedParametricCostLarge(lo, crossed, r, g, INF);
    CHECK(x.status == LP_INFEASIBLE && x.slope.size() == 0 && x.basis == r.basis);
    CHECK(s.boundedParametricRhsLarge(lo, crossed, rep, d, INF).status == LP_INFEASIBLE);
    Solver::BoundedResult bad = r;
    bad.basis[1] = N;                // out of range
    CHECK_THROWS(s.boundedParametricRhsLarge(lo, hi, bad, d, INF), std::invalid_argument);
    bad = r;
    bad.atUpper[0] = 1;              // column 0 has no upper bound
    CHECK(hi[0] == INF);
    CHECK_THROWS(s.boundedParametricCostLarge(lo, hi, bad, g, INF), std::invalid_argument);
    CHECK_THROWS(s.boundedParametricRhsLarge(lo, hi, r, g, INF), std::invalid_argument);    // g has n entries
    CHECK_THROWS(s.boundedParametricCostLarge(lo, hi, r, d, INF), std::invalid_argument);   // d has m entries
    CHECK_THROWS(s.boundedParametricRhsLarge(lo, hi, r, d, -1.0), std::invalid_argument);
    // and a good call afterwards
    same_paths(s.boundedParametricRhsLarge(lo, hi, r, d, INF), good);
}

int main(int argc, char** argv) { return run_all(argc > 1 ? argv[1] : nullptr); }
