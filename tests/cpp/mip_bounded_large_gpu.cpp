// GPU tests of Solver::boundedBranchAndBoundLarge: on a 160 x 320 boxed problem (beyond lp_mip_bounded_fits at any
// depth) with every other structural column integer, the search from an optimal Solver::boundedSimplexLarge result
// equals tests/ref/mip_bounded_ref.c's bit for bit (the library named by LP_MIP_BOUNDED_REF, loaded at run time); the
// form that solves the relaxation itself agrees; the LDS form still refuses the shape; bad arguments throw
// std::invalid_argument.  (No test_ prefix: tests/test_mip_bounded_large_cpp.py runs this program.)
#include <cmath>
#include <cstdint>

#include "check.h"
#include "fixtures.h"
#include "Canonical.h"
#include "SimplexSolover.h"

using lpla::MatrixXd;
using lpla::VectorXd;

typedef int (*RefMipBounded)(const double*, int, int, const double*, const double*, const double*, const double*,
                             const int*, const int*, int, int, const int*, double, double, double, int, int, int, double*,
                             double*, double*, int*, int*);

static const int M = 160, K = 160, N = M + K;

// tests/cpp/test_bounded_large_gpu.cpp's problem with the columns j < K, j even, integer: their bounds rounded outward
static Canonical mixed_problem(uint64_t seed, bool maximize, MatrixXd* A, VectorXd* b, VectorXd* c,
                               std::vector<double>* lo, std::vector<double>* hi, std::vector<bool>* mask) {
    Canonical can = boxed_problem(seed, M, K, maximize, A, b, c, lo, hi, /*a_offset=*/0.0, /*b_scale=*/0.125);
    mask->assign((size_t)N, false);
    for (int j = 0; j < K; j += 2) {
        (*mask)[(size_t)j] = true;
        (*lo)[(size_t)j] = std::floor((*lo)[(size_t)j]);
        if (std::isfinite((*hi)[(size_t)j])) (*hi)[(size_t)j] = std::ceil((*hi)[(size_t)j]);
    }
    return can;
}

TEST(BoundedBranchAndBoundLarge_MatchesTheRef) {
    const RefLib lib("LP_MIP_BOUNDED_REF");
    RefMipBounded ref = lib.symbol<RefMipBounded>("ref_mip_bounded");
    CHECK(lp_mip_bounded_fits(M, N, 0) == 0);
    const int depth = 64, nodes = 40;
    int searched = 0;
    for (uint64_t seed = 1; ref && seed <= 4; ++seed) {
        const bool maximize = seed % 2 == 0;
        MatrixXd A;
        VectorXd b, c;
        std::vector<double> lo, hi;
        std::vector<bool> mask;
        Solver s(mixed_problem(seed, maximize, &A, &b, &c, &lo, &hi, &mask));
        const Solver::BoundedResult cold = s.boundedSimplexLarge(lo, hi, /*throw_on_failure=*/false);
        if (cold.status != LP_OPTIMAL) continue;
        const Solver::IntegerResult g = s.boundedBranchAndBoundLarge(mask, lo, hi, cold, depth, nodes);
        const std::vector<int> imask(mask.begin(), mask.end());
        std::vector<double> x((size_t)N, std::nan(""));
        double obj = std::nan(""), bound = std::nan("");
        int found = 0, stats[5];
        const int st = ref(A.data(), M, N, b.data(), c.data(), lo.data(), hi.data(), cold.basis.data(),
                           cold.atUpper.data(), maximize ? 1 : 0, N, imask.data(), Solver::EPS, Solver::INT_TOL,
                           Solver::MIP_GAP, depth, nodes, Solver::MAX_ITER, x.data(), &obj, &bound, &found, stats);
        std::printf("  seed %d: status %d, %d nodes, found %d, deepest level %d\n", (int)seed, g.status, g.nodes,
                    (int)g.found, stats[4]);
        CHECK(st == g.status);
        CHECK((found != 0) == g.found && stats[0] == g.nodes);
        CHECK(same_value(obj, g.objective) && same_value(bound, g.bound));
        for (int j = 0; j < N; ++j) CHECK(same_value(x[(size_t)j], g.x[j]));
        if (stats[0] > 1) ++searched;
        // the form that solves the relaxation first
        const Solver::IntegerResult own = s.boundedBranchAndBoundLarge(mask, lo, hi, depth, nodes);
        CHECK(own.status == g.status && own.nodes == g.nodes && same_value(own.objective, g.objective));
        // the LDS entry still refuses this shape
        CHECK_THROWS(s.boundedBranchAndBound(mask, lo, hi, cold, depth, nodes), std::invalid_argument);
    }
    CHECK(searched >= 2);
}

TEST(BoundedBranchAndBoundLarge_BadArguments) {
    std::vector<double> lo, hi;
    std::vector<bool> mask;
    Solver s(mixed_problem(2, true, nullptr, nullptr, nullptr, &lo, &hi, &mask));
    const Solver::BoundedResult cold = s.boundedSimplexLarge(lo, hi);
    CHECK_THROWS(s.boundedBranchAndBoundLarge(std::vector<bool>(3, true), lo, hi, cold), std::invalid_argument);
    CHECK_THROWS(s.boundedBranchAndBoundLarge(mask, lo, hi, cold, 1025), std::invalid_argument);
    CHECK_THROWS(s.boundedBranchAndBoundLarge(mask, lo, hi, cold, 64, 0), std::invalid_argument);
    std::vector<double> frac = hi;
    frac[0] = lo[0] + 2.5;
    CHECK_THROWS(s.boundedBranchAndBoundLarge(mask, lo, frac, cold), std::invalid_argument);
    Solver::BoundedResult bad = cold;
    bad.basis[1] = N;
    CHECK_THROWS(s.boundedBranchAndBoundLarge(mask, lo, hi, bad), std::invalid_argument);
    // the context still solves
    const Solver::IntegerResult g = s.boundedBranchAndBoundLarge(mask, lo, hi, cold, 64, 5);
    CHECK(g.nodes >= 1 && g.nodes <= 5);
}

int main(int argc, char** argv) { return run_all(argc > 1 ? argv[1] : nullptr); }
