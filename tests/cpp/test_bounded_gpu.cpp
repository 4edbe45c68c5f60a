// GPU tests of Solver::boundedSimplex: on boxed problems of both senses (fixed, negative-lo and infinite-hi columns)
// the result equals tests/ref/bounded_ref.c's bit for bit (the library named by LP_BOUNDED_REF, loaded at run time);
// an infeasible box throws unless asked not to, and bad bounds throw std::invalid_argument.
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

typedef int (*RefBounded)(const double*, int, int, const double*, const double*, const double*, const double*, int, int,
                          double, int, double*, int*, int*, double*, int*);

TEST(BoundedSimplex_MatchesTheRef) {
    const RefLib lib("LP_BOUNDED_REF");
    RefBounded ref = lib.symbol<RefBounded>("ref_bounded");
    int optimal = 0, flipped = 0;
    for (uint64_t seed = 0; ref && seed < 24; ++seed) {
        const int m = 3 + (int)(seed % 5), k = 5 + (int)(seed % 7), n = k + m;
        const bool maximize = seed % 2 == 0;
        MatrixXd A;
        VectorXd b, c;
        std::vector<double> lo, hi;
        Canonical p = boxed_problem(seed, m, k, maximize, &A, &b, &c, &lo, &hi);
        Solver s(p);
        const Solver::BoundedResult g = s.boundedSimplex(lo, hi, /*throw_on_failure=*/false);
        std::vector<double> x((size_t)n, std::nan(""));
        std::vector<int> basis((size_t)m), up((size_t)n);
        double obj = std::nan("");
        int it[4];
        const int st = ref(A.data(), m, n, b.data(), c.data(), lo.data(), hi.data(), maximize ? 1 : 0, n, Solver::EPS,
                           Solver::MAX_ITER, x.data(), basis.data(), up.data(), &obj, it);
        CHECK(st == g.status);
        CHECK(same_value(obj, g.objective));
        for (int j = 0; j < n; ++j) CHECK(same_value(x[(size_t)j], g.x[j]) && up[(size_t)j] == g.atUpper[(size_t)j]);
        CHECK(basis == g.basis);
        for (int q = 0; q < 4; ++q) CHECK(it[q] == g.iterations[q]);
        if (st == LP_OPTIMAL) {
            ++optimal;
            if (it[3] > 0) ++flipped;
            (void)s.boundedSimplex(lo, hi);   // throws nothing when optimal
        }
    }
    CHECK(optimal > 12);
    CHECK(flipped > 0);
}

TEST(BoundedSimplex_FailuresAndBadBounds) {
    MatrixXd A;
    VectorXd b, c;
    std::vector<double> lo, hi;
    Canonical p = boxed_problem(5, 4, 6, true, &A, &b, &c, &lo, &hi);
    Solver s(p);
    std::vector<double> crossed = hi;
    crossed[0] = lo[0] - 1.0;
    const Solver::BoundedResult g = s.boundedSimplex(lo, crossed, false);
    CHECK(g.status == LP_INFEASIBLE && std::isnan(g.objective));
    for (int q = 0; q < 4; ++q) CHECK(g.iterations[q] == 0);
    CHECK_THROWS(s.boundedSimplex(lo, crossed), std::runtime_error);
    std::vector<double> free_lo = lo;
    free_lo[1] = -INF;
    CHECK_THROWS(s.boundedSimplex(free_lo, hi, false), std::invalid_argument);
    CHECK_THROWS(s.boundedSimplex(std::vector<double>(3, 0.0), hi), std::invalid_argument);
}

int main(int argc, char** argv) { return run_all(argc > 1 ? argv[1] : nullptr); }
