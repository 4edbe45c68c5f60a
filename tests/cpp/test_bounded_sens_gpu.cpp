// GPU tests of Solver::boundedDuals and Solver::boundedRanging: at an optimal Solver::boundedSimplex result they equal
// tests/ref/bounded_sens_ref.c's bit for bit (the library named by LP_BOUNDED_SENS_REF, loaded at run time), the dual
// objective is the primal one, a result that is not optimal keeps its status with NaN, a repeated basis index is
// singular, and a bad flag or index throws std::invalid_argument.
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

TEST(BoundedSens_MatchesTheRef) {
    const RefLib lib("LP_BOUNDED_SENS_REF");
    RefBoundedDuals ref_d = lib.symbol<RefBoundedDuals>("ref_bounded_duals");
    RefBoundedRanging ref_r = lib.symbol<RefBoundedRanging>("ref_bounded_ranging");
    int checked = 0, at_upper = 0;
    for (uint64_t seed = 0; ref_d && ref_r && seed < 16; ++seed) {
        const int m = 3 + (int)(seed % 5), k = 5 + (int)(seed % 7), n = k + m;
        const bool maximize = seed % 2 == 0;
        MatrixXd A;
        VectorXd b, c;
        std::vector<double> lo, hi;
        Canonical p = boxed_problem(seed, m, k, maximize, &A, &b, &c, &lo, &hi);
        Solver s(p);
        const Solver::BoundedResult sol = s.boundedSimplex(lo, hi, /*throw_on_failure=*/false);
        if (sol.status != LP_OPTIMAL) continue;
        ++checked;
        for (int j = 0; j < n; ++j) at_upper += sol.atUpper[(size_t)j];
        const Solver::BoundedDuals g = s.boundedDuals(lo, hi, sol);
        const Solver::BoundedRanging q = s.boundedRanging(lo, hi, sol);
        std::vector<double> x((size_t)n), y((size_t)m), d((size_t)n), rhs(2 * (size_t)m), cost(2 * (size_t)n);
        std::vector<int> rv(2 * (size_t)m), rs(2 * (size_t)m), cv(2 * (size_t)n);
        double w = 0.0;
        int st = ref_d(A.data(), m, n, b.data(), c.data(), lo.data(), hi.data(), sol.basis.data(), sol.atUpper.data(),
                       x.data(), y.data(), d.data(), &w);
        CHECK(st == g.status && st == LP_OPTIMAL);
        CHECK(same_bits(g.objective, w));
        CHECK(std::fabs(g.objective - sol.objective) <= 1e-7 * (1 + std::fabs(sol.objective)));
        for (int j = 0; j < n; ++j) CHECK(same_bits(g.x[j], x[(size_t)j]) && same_bits(g.d[j], d[(size_t)j]));
        for (int i = 0; i < m; ++i) CHECK(same_bits(g.y[i], y[(size_t)i]));
        st = ref_r(A.data(), m, n, b.data(), c.data(), lo.data(), hi.data(), sol.basis.data(), sol.atUpper.data(),
                   maximize ? 1 : 0, Solver::EPS, rhs.data(), rv.data(), rs.data(), cost.data(), cv.data());
        CHECK(st == q.status && st == LP_OPTIMAL);
        for (int i = 0; i < m; ++i) {
            const size_t a = 2 * (size_t)i;
            CHECK(same_bits(q.b_lo[i], rhs[a]) && same_bits(q.b_hi[i], rhs[a + 1]));
            CHECK(q.b_leave_lo[(size_t)i] == rv[a] && q.b_leave_hi[(size_t)i] == rv[a + 1]);
            CHECK(q.b_side_lo[(size_t)i] == rs[a] && q.b_side_hi[(size_t)i] == rs[a + 1]);
            CHECK(q.b_lo[i] <= b[i] + 1e-9 && b[i] <= q.b_hi[i] + 1e-9);
        }
        for (int j = 0; j < n; ++j) {
            const size_t a = 2 * (size_t)j;
            CHECK(same_bits(q.c_lo[j], cost[a]) && same_bits(q.c_hi[j], cost[a + 1]));
            CHECK(q.c_enter_lo[(size_t)j] == cv[a] && q.c_enter_hi[(size_t)j] == cv[a + 1]);
            CHECK(q.c_lo[j] <= c[j] + 1e-9 && c[j] <= q.c_hi[j] + 1e-9);
        }
    }
    CHECK(checked >= 12 && at_upper >= 4);
}

TEST(BoundedSens_StatusesAndExceptions) {
    MatrixXd A;
    VectorXd b, c;
    std::vector<double> lo, hi;
    Canonical p = boxed_problem(2, 4, 7, true, &A, &b, &c, &lo, &hi);
    const int n = 11;
    Solver s(p);
    Solver::BoundedResult r = s.boundedSimplex(lo, hi, /*throw_on_failure=*/false);
    CHECK(r.status == LP_OPTIMAL);
    r.status = LP_UNBOUNDED;   // a result that is not optimal keeps its status
    const Solver::BoundedDuals g = s.boundedDuals(lo, hi, r);
    const Solver::BoundedRanging q = s.boundedRanging(lo, hi, r);
    CHECK(g.status == LP_UNBOUNDED && std::isnan(g.x[0]) && std::isnan(g.y[0]) && std::isnan(g.objective));
    CHECK(q.status == LP_UNBOUNDED && std::isnan(q.b_lo[0]) && q.b_side_hi[0] == -1 && q.c_enter_lo[0] == -1);
    r.status = LP_OPTIMAL;
    Solver::BoundedResult rep = r;
    rep.basis[1] = rep.basis[0];   // repeated index: singular
    CHECK(s.boundedDuals(lo, hi, rep).status == LP_SINGULAR);
    const Solver::BoundedRanging e = s.boundedRanging(lo, hi, rep);
    CHECK(e.status == LP_SINGULAR && std::isnan(e.b_hi[0]) && e.b_leave_lo[0] == -1 && e.b_side_lo[0] == -1);
    std::vector<double> crossed = hi;
    crossed[1] = lo[1] - 1.0;      // crossed bounds: infeasible, nothing thrown
    CHECK(s.boundedDuals(lo, crossed, r).status == LP_INFEASIBLE);
    CHECK(s.boundedRanging(lo, crossed, r).status == LP_INFEASIBLE);
    Solver::BoundedResult bad = r;
    bad.basis[1] = 1000;           // out of range
    CHECK_THROWS(s.boundedDuals(lo, hi, bad), std::invalid_argument);
    CHECK_THROWS(s.boundedRanging(lo, hi, bad), std::invalid_argument);
    bad = r;
    bad.atUpper[0] = 1;            // column 0 has no upper bound
    CHECK(hi[0] == INF);
    CHECK_THROWS(s.boundedDuals(lo, hi, bad), std::invalid_argument);
    CHECK_THROWS(s.boundedRanging(lo, hi, bad), std::invalid_argument);
    std::vector<double> few(lo.begin(), lo.begin() + n - 1);
    CHECK_THROWS(s.boundedDuals(few, hi, r), std::invalid_argument);
    CHECK_THROWS(s.boundedRanging(few, hi, r), std::invalid_argument);
}

int main(int argc, char** argv) { return run_all(argc > 1 ? argv[1] : nullptr); }
