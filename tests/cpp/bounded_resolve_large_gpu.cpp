// GPU tests of Solver::boundedResolveLarge: an optimal Solver::boundedSimplexLarge result on a 160 x 320 boxed LP (beyond
// lp_simplex_bounded_fits) is fed back after one bound of a basic column was tightened, and the result equals
// tests/ref/bounded_resolve_ref.c's bit for bit (the library named by LP_BOUNDED_RESOLVE_REF, loaded at run time); fed
// back unchanged it is optimal again; crossed bounds throw unless asked not to, and a bad start throws
// std::invalid_argument.  (No test_ prefix: tests/test_bounded_resolve_large_cpp.py runs this program.)
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

static const int M = 160, K = 160, N = M + K;

// tests/cpp/test_bounded_large_gpu.cpp's problem: fixtures.h's boxed problem with b_i in 0.125 k [1, 2)
static Canonical large_problem(uint64_t seed, bool maximize, MatrixXd* A, VectorXd* b, VectorXd* c,
                               std::vector<double>* lo, std::vector<double>* hi) {
    return boxed_problem(seed, M, K, maximize, A, b, c, lo, hi, /*a_offset=*/0.0, /*b_scale=*/0.125);
}

TEST(BoundedResolveLarge_MatchesTheRef) {
    const RefLib lib("LP_BOUNDED_RESOLVE_REF");
    RefBoundedResolve ref = lib.symbol<RefBoundedResolve>("ref_bounded_resolve");
    CHECK(lp_simplex_bounded_fits(M, N) == 0);
    int warm = 0, dual = 0;
    for (uint64_t seed = 1; ref && seed <= 4; ++seed) {
        const bool maximize = seed % 2 == 0;
        MatrixXd A;
        VectorXd b, c;
        std::vector<double> lo, hi;
        Solver s(large_problem(seed, maximize, &A, &b, &c, &lo, &hi));
        const Solver::BoundedResult cold = s.boundedSimplexLarge(lo, hi, /*throw_on_failure=*/false);
        if (cold.status != LP_OPTIMAL) continue;
        ++warm;
        // fed back unchanged: optimal again, nothing thrown
        const Solver::BoundedResult again = s.boundedResolveLarge(lo, hi, cold);
        CHECK(again.status == LP_OPTIMAL);
        CHECK(std::fabs(again.objective - cold.objective) <= 1e-9 * std::fmax(1.0, std::fabs(cold.objective)));
        // a branch on the basic column of position 7 seed: its upper bound pulled below its value, or its lower bound
        // pushed above it
        const int kb = cold.basis[(size_t)(7 * seed % (uint64_t)M)];
        const double xk = cold.x[kb];
        if (seed % 4 < 2) hi[(size_t)kb] = lo[(size_t)kb] + 0.5 * (xk - lo[(size_t)kb]);
        else lo[(size_t)kb] = xk + 0.25;
        const Solver::BoundedResult g = s.boundedResolveLarge(lo, hi, cold, /*throw_on_failure=*/false);
        std::vector<double> x((size_t)N, std::nan(""));
        std::vector<int> basis((size_t)M), up((size_t)N);
        double obj = std::nan("");
        int it[3];
        const int st = ref(A.data(), M, N, b.data(), c.data(), lo.data(), hi.data(), cold.basis.data(),
                           cold.atUpper.data(), maximize ? 1 : 0, N, Solver::EPS, Solver::MAX_ITER, x.data(),
                           basis.data(), up.data(), &obj, it);
        std::printf("  seed %d: status %d, iterations %d + %d, %d flips\n", (int)seed, g.status, g.iterations[0],
                    g.iterations[1], g.iterations[2]);
        CHECK(st == g.status);
        CHECK(same_value(obj, g.objective));
        for (int j = 0; j < N; ++j) CHECK(same_value(x[(size_t)j], g.x[j]) && up[(size_t)j] == g.atUpper[(size_t)j]);
        CHECK(basis == g.basis);
        for (int q = 0; q < 3; ++q) CHECK(it[q] == g.iterations[q]);
        CHECK(g.iterations[3] == 0);
        if (it[0] > 0) ++dual;
        // the LDS entry still refuses this shape
        CHECK_THROWS(s.boundedResolve(lo, hi, cold, false), std::invalid_argument);
    }
    CHECK(warm >= 2);
    CHECK(dual >= 2);
}

TEST(BoundedResolveLarge_FailuresAndBadStarts) {
    std::vector<double> lo, hi;
    Solver s(large_problem(2, true, nullptr, nullptr, nullptr, &lo, &hi));
    const Solver::BoundedResult cold = s.boundedSimplexLarge(lo, hi);
    std::vector<double> crossed = hi;
    crossed[0] = lo[0] - 1.0;
    const Solver::BoundedResult g = s.boundedResolveLarge(lo, crossed, cold, false);
    CHECK(g.status == LP_INFEASIBLE && std::isnan(g.objective));
    CHECK(g.basis == cold.basis && g.atUpper == cold.atUpper);
    for (int q = 0; q < 4; ++q) CHECK(g.iterations[q] == 0);
    CHECK_THROWS(s.boundedResolveLarge(lo, crossed, cold), std::runtime_error);
    Solver::BoundedResult bad = cold;
    bad.atUpper[0] = 1;   // column 0 has no upper bound
    CHECK_THROWS(s.boundedResolveLarge(lo, hi, bad, false), std::invalid_argument);
    bad = cold;
    bad.basis[1] = N;
    CHECK_THROWS(s.boundedResolveLarge(lo, hi, bad, false), std::invalid_argument);
    bad = cold;
    bad.basis[1] = bad.basis[0];   // a repeated column: singular
    const Solver::BoundedResult sing = s.boundedResolveLarge(lo, hi, bad, false);
    CHECK(sing.status == LP_SINGULAR && sing.basis == bad.basis && sing.atUpper == bad.atUpper);
}

int main(int argc, char** argv) { return run_all(argc > 1 ? argv[1] : nullptr); }
