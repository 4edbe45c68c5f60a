// GPU tests of Solver::boundedDualsLarge and Solver::boundedRangingLarge: at an optimal Solver::boundedSimplexLarge
// result on a 160 x 320 boxed LP (beyond lp_basis_bounded_fits) they equal tests/ref/bounded_sens_ref.c's bit for bit
// (the library named by LP_BOUNDED_SENS_REF, loaded at run time) and the dual objective is the primal one; the LDS
// methods still refuse the shape; a result that is not optimal keeps its status with NaN, crossed bounds are
// infeasible, a repeated basis index is singular, and a bad flag or index throws std::invalid_argument.
// (No test_ prefix: tests/test_bounded_sens_large_cpp.py runs this program.)
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

typedef int (*RefBoundedDuals)(const double*, int, int, const double*, const double*, const double*, const double*,
                               const int*, const int*, double*, double*, double*, double*);
typedef int (*RefBoundedRanging)(const double*, int, int, const double*, const double*, const double*, const double*,
                                 const int*, const int*, int, double, double*, int*, int*, double*, int*);

static const int M = 160, K = 160, N = M + K;

// tests/cpp/test_bounded_large_gpu.cpp's problem: fixtures.h's boxed problem with b_i in 0.125 k [1, 2)
static Canonical large_problem(uint64_t seed, bool maximize, MatrixXd* A, VectorXd* b, VectorXd* c,
                               std::vector<double>* lo, std::vector<double>* hi) {
    return boxed_problem(seed, M, K, maximize, A, b, c, lo, hi, /*a_offset=*/0.0, /*b_scale=*/0.125);
}

TEST(BoundedSensLarge_MatchesTheRef) {
    const RefLib lib("LP_BOUNDED_SENS_REF");
    RefBoundedDuals ref_d = lib.symbol<RefBoundedDuals>("ref_bounded_duals");
    RefBoundedRanging ref_r = lib.symbol<RefBoundedRanging>("ref_bounded_ranging");
    CHECK(lp_basis_bounded_fits(M, N) == 0);
    int checked = 0, at_upper = 0, upper_sides = 0;
    for (uint64_t seed = 1; ref_d && ref_r && seed <= 4; ++seed) {
        const bool maximize = seed % 2 == 0;
        MatrixXd A;
        VectorXd b, c;
        std::vector<double> lo, hi;
        Solver s(large_problem(seed, maximize, &A, &b, &c, &lo, &hi));
        const Solver::BoundedResult sol = s.boundedSimplexLarge(lo, hi, /*throw_on_failure=*/false);
        if (sol.status != LP_OPTIMAL) continue;
        ++checked;
        for (int j = 0; j < N; ++j) at_upper += sol.atUpper[(size_t)j];
        const Solver::BoundedDuals g = s.boundedDualsLarge(lo, hi, sol);
        const Solver::BoundedRanging q = s.boundedRangingLarge(lo, hi, sol);
        std::vector<double> x((size_t)N), y((size_t)M), d((size_t)N), rhs(2 * (size_t)M), cost(2 * (size_t)N);
        std::vector<int> rv(2 * (size_t)M), rs(2 * (size_t)M), cv(2 * (size_t)N);
        double w = 0.0;
        int st = ref_d(A.data(), M, N, b.data(), c.data(), lo.data(), hi.data(), sol.basis.data(), sol.atUpper.data(),
                       x.data(), y.data(), d.data(), &w);
        CHECK(st == g.status && st == LP_OPTIMAL);
        CHECK(same_bits(g.objective, w));
        CHECK(std::fabs(g.objective - sol.objective) <= 1e-7 * (1 + std::fabs(sol.objective)));
        for (int j = 0; j < N; ++j) CHECK(same_bits(g.x[j], x[(size_t)j]) && same_bits(g.d[j], d[(size_t)j]));
        for (int i = 0; i < M; ++i) CHECK(same_bits(g.y[i], y[(size_t)i]));
        st = ref_r(A.data(), M, N, b.data(), c.data(), lo.data(), hi.data(), sol.basis.data(), sol.atUpper.data(),
                   maximize ? 1 : 0, Solver::EPS, rhs.data(), rv.data(), rs.data(), cost.data(), cv.data());
        CHECK(st == q.status && st == LP_OPTIMAL);
        for (int i = 0; i < M; ++i) {
            const size_t a = 2 * (size_t)i;
            CHECK(same_bits(q.b_lo[i], rhs[a]) && same_bits(q.b_hi[i], rhs[a + 1]));
            CHECK(q.b_leave_lo[(size_t)i] == rv[a] && q.b_leave_hi[(size_t)i] == rv[a + 1]);
            CHECK(q.b_side_lo[(size_t)i] == rs[a] && q.b_side_hi[(size_t)i] == rs[a + 1]);
            upper_sides += (rs[a] == 1) + (rs[a + 1] == 1);
        }
        for (int j = 0; j < N; ++j) {
            const size_t a = 2 * (size_t)j;
            CHECK(same_bits(q.c_lo[j], cost[a]) && same_bits(q.c_hi[j], cost[a + 1]));
            CHECK(q.c_enter_lo[(size_t)j] == cv[a] && q.c_enter_hi[(size_t)j] == cv[a + 1]);
        }
        // the LDS methods still refuse this shape
        CHECK_THROWS(s.boundedDuals(lo, hi, sol), std::invalid_argument);
        CHECK_THROWS(s.boundedRanging(lo, hi, sol), std::invalid_argument);
    }
    std::printf("  %d optimal, %d columns at upper, %d ends leave at an upper bound\n", checked, at_upper, upper_sides);
    CHECK(checked >= 2 && at_upper >= 4 && upper_sides >= 1);
}

TEST(BoundedSensLarge_StatusesAndExceptions) {
    std::vector<double> lo, hi;
    Solver s(large_problem(2, true, nullptr, nullptr, nullptr, &lo, &hi));
    Solver::BoundedResult r = s.boundedSimplexLarge(lo, hi, /*throw_on_failure=*/false);
    CHECK(r.status == LP_OPTIMAL);
    r.status = LP_UNBOUNDED;   // a result that is not optimal keeps its status
    const Solver::BoundedDuals g = s.boundedDualsLarge(lo, hi, r);
    const Solver::BoundedRanging q = s.boundedRangingLarge(lo, hi, r);
    CHECK(g.status == LP_UNBOUNDED && std::isnan(g.x[0]) && std::isnan(g.y[0]) && std::isnan(g.objective));
    CHECK(q.status == LP_UNBOUNDED && std::isnan(q.b_lo[0]) && q.b_side_hi[0] == -1 && q.c_enter_lo[0] == -1);
    r.status = LP_OPTIMAL;
    Solver::BoundedResult rep = r;
    rep.basis[1] = rep.basis[0];   // repeated index: singular
    const Solver::BoundedDuals gs = s.boundedDualsLarge(lo, hi, rep);
    CHECK(gs.status == LP_SINGULAR && std::isnan(gs.x[0]) && std::isnan(gs.objective));
    const Solver::BoundedRanging e = s.boundedRangingLarge(lo, hi, rep);
    CHECK(e.status == LP_SINGULAR && std::isnan(e.b_hi[0]) && e.b_leave_lo[0] == -1 && e.b_side_lo[0] == -1);
    std::vector<double> crossed = hi;
    crossed[1] = lo[1] - 1.0;      // crossed bounds: infeasible, nothing thrown
    CHECK(s.boundedDualsLarge(lo, crossed, r).status == LP_INFEASIBLE);
    CHECK(s.boundedRangingLarge(lo, crossed, r).status == LP_INFEASIBLE);
    Solver::BoundedResult bad = r;
    bad.basis[1] = N;              // out of range
    CHECK_THROWS(s.boundedDualsLarge(lo, hi, bad), std::invalid_argument);
    CHECK_THROWS(s.boundedRangingLarge(lo, hi, bad), std::invalid_argument);
    bad = r;
    int free = 0;
    while (hi[(size_t)free] != INF) ++free;
    bad.atUpper[(size_t)free] = 1;   // a column without an upper bound
    CHECK_THROWS(s.boundedDualsLarge(lo, hi, bad), std::invalid_argument);
    CHECK_THROWS(s.boundedRangingLarge(lo, hi, bad), std::invalid_argument);
    // and a good call afterwards
    CHECK(s.boundedDualsLarge(lo, hi, r).status == LP_OPTIMAL);
    CHECK(s.boundedRangingLarge(lo, hi, r).status == LP_OPTIMAL);
}

int main(int argc, char** argv) { return run_all(argc > 1 ? argv[1] : nullptr); }
