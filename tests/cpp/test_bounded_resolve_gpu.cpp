// GPU tests of Solver::boundedResolve: an optimal Solver::boundedSimplex result is fed back after one bound of a basic
// column was tightened, and the result equals tests/ref/bounded_resolve_ref.c's bit for bit (the library named by
// LP_BOUNDED_RESOLVE_REF, loaded at run time); fed back unchanged it is optimal again; crossed bounds throw unless
// asked not to, and a bad start throws std::invalid_argument.
#include <cmath>
#include <cstdint>

#include "check.h"
#include "fixtures.h"
#include "Canonical.h"
#include "SimplexSolover.h"

using lpla::MatrixXd;
using lpla::VectorXd;

typedef int (*RefBoundedResolve)(const double*, int, int, const double*, const double*, const double*, const double*,
                                 const int*, const int*, int, int, double, int, double*, int*, int*, double*, int*);

TEST(BoundedResolve_MatchesTheRef) {
    const RefLib lib("LP_BOUNDED_RESOLVE_REF");
    RefBoundedResolve ref = lib.symbol<RefBoundedResolve>("ref_bounded_resolve");
    int warm = 0, dual = 0;
    for (uint64_t seed = 0; ref && seed < 24; ++seed) {
        const int m = 3 + (int)(seed % 5), k = 5 + (int)(seed % 7), n = k + m;
        const bool maximize = seed % 2 == 0;
        MatrixXd A;
        VectorXd b, c;
        std::vector<double> lo, hi;
        Canonical p = boxed_problem(seed, m, k, maximize, &A, &b, &c, &lo, &hi);
        Solver s(p);
        const Solver::BoundedResult cold = s.boundedSimplex(lo, hi, /*throw_on_failure=*/false);
        if (cold.status != LP_OPTIMAL) continue;
        ++warm;
        // fed back unchanged: optimal again, nothing thrown
        const Solver::BoundedResult again = s.boundedResolve(lo, hi, cold);
        CHECK(again.status == LP_OPTIMAL);
        CHECK(std::fabs(again.objective - cold.objective) <= 1e-9 * std::fmax(1.0, std::fabs(cold.objective)));
        // a branch on the basic column of position seed % m: its upper bound pulled below its value, or its lower
        // bound pushed above it
        const int kb = cold.basis[(size_t)(seed % (uint64_t)m)];
        const double xk = cold.x[kb];
        if (seed % 4 < 2) hi[(size_t)kb] = lo[(size_t)kb] + 0.5 * (xk - lo[(size_t)kb]);
        else lo[(size_t)kb] = xk + 0.25;
        const Solver::BoundedResult g = s.boundedResolve(lo, hi, cold, /*throw_on_failure=*/false);
        std::vector<double> x((size_t)n, std::nan(""));
        std::vector<int> basis((size_t)m), up((size_t)n);
        double obj = std::nan("");
        int it[3];
        const int st = ref(A.data(), m, n, b.data(), c.data(), lo.data(), hi.data(), cold.basis.data(),
                           cold.atUpper.data(), maximize ? 1 : 0, n, Solver::EPS, Solver::MAX_ITER, x.data(),
                           basis.data(), up.data(), &obj, it);
        CHECK(st == g.status);
        CHECK(same_value(obj, g.objective));
        for (int j = 0; j < n; ++j) CHECK(same_value(x[(size_t)j], g.x[j]) && up[(size_t)j] == g.atUpper[(size_t)j]);
        CHECK(basis == g.basis);
        for (int q = 0; q < 3; ++q) CHECK(it[q] == g.iterations[q]);
        CHECK(g.iterations[3] == 0);
        if (it[0] > 0) ++dual;
    }
    CHECK(warm > 12);
    CHECK(dual > 6);
}

TEST(BoundedResolve_FailuresAndBadStarts) {
    MatrixXd A;
    VectorXd b, c;
    std::vector<double> lo, hi;
    Canonical p = boxed_problem(5, 4, 6, true, &A, &b, &c, &lo, &hi);
    Solver s(p);
    const Solver::BoundedResult cold = s.boundedSimplex(lo, hi);
    std::vector<double> crossed = hi;
    crossed[0] = lo[0] - 1.0;
    const Solver::BoundedResult g = s.boundedResolve(lo, crossed, cold, false);
    CHECK(g.status == LP_INFEASIBLE && std::isnan(g.objective));
    CHECK(g.basis == cold.basis && g.atUpper == cold.atUpper);
    for (int q = 0; q < 4; ++q) CHECK(g.iterations[q] == 0);
    CHECK_THROWS(s.boundedResolve(lo, crossed, cold), std::runtime_error);
    Solver::BoundedResult bad = cold;
    bad.atUpper[0] = 1;   // column 0 has no upper bound
    CHECK_THROWS(s.boundedResolve(lo, hi, bad, false), std::invalid_argument);
    bad = cold;
    bad.basis[1] = 10;
    CHECK_THROWS(s.boundedResolve(lo, hi, bad, false), std::invalid_argument);
    bad = cold;
    bad.basis[1] = bad.basis[0];   // a repeated column: singular
    CHECK(s.boundedResolve(lo, hi, bad, false).status == LP_SINGULAR);
    bad = cold;
    bad.basis.pop_back();
    CHECK_THROWS(s.boundedResolve(lo, hi, bad), std::invalid_argument);
    CHECK_THROWS(s.boundedResolve(std::vector<double>(3, 0.0), hi, cold), std::invalid_argument);
}

int main(int argc, char** argv) { return run_all(argc > 1 ? argv[1] : nullptr); }
