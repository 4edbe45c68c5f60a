// GPU tests of Solver::boundedResolve and Solver::boundedResolveLarge under a dual ratio test: an optimal cold result on
// a boxed LP is fed back after one bound of a basic column was tightened, under DualRatio::LongStep, both DualRules and
// every PivotRule, and the result equals tests/ref/bounded_resolve_long_step_ref.c's bit for bit (the library named by
// LP_BOUNDED_RESOLVE_LONG_STEP_REF, loaded at run time): at 32 x 96 through both entries, which must agree, and at
// 160 x 320 (beyond lp_simplex_bounded_fits) through boundedResolveLarge.  DualRatio::Textbook is the overload without
// a ratio test bit for bit.  (No test_ prefix: tests/test_bounded_resolve_long_step_cpp.py runs this program.)
#include <cmath>
#include <cstdint>

#include "check.h"
#include "fixtures.h"
#include "Canonical.h"
#include "SimplexSolover.h"

using lpla::MatrixXd;
using lpla::VectorXd;

typedef int (*RefBoundedResolveLong)(const double*, int, int, const double*, const double*, const double*,
                                     const double*, const int*, const int*, int, int, double, int, double*, int*, int*,
                                     double*, int*, int, int, int);

static bool same_result(const Solver::BoundedResult& a, const Solver::BoundedResult& b) {
    bool ok = a.status == b.status && a.basis == b.basis && a.atUpper == b.atUpper && same_value(a.objective, b.objective);
    for (int q = 0; q < 4; ++q) ok = ok && a.iterations[q] == b.iterations[q];
    for (int j = 0; ok && j < (int)a.x.size(); ++j) ok = same_value(a.x[j], b.x[j]);
    return ok;
}

// One shape: cold solves, a branch on a basic column, the re-solve under (rule, dual, LongStep) against the reference
static void run_shape(RefBoundedResolveLong ref, int M, int K, bool lds, int* warm, int* flipped) {
    const int N = M + K;
    for (uint64_t seed = 1; ref && seed <= 4; ++seed) {
        const bool maximize = seed % 2 == 0;
        MatrixXd A;
        VectorXd b, c;
        std::vector<double> lo, hi;
        Solver s(boxed_problem(seed, M, K, maximize, &A, &b, &c, &lo, &hi, /*a_offset=*/0.0, /*b_scale=*/0.125));
        const Solver::BoundedResult cold = s.boundedSimplexLarge(lo, hi, /*throw_on_failure=*/false);
        if (cold.status != LP_OPTIMAL) continue;
        ++*warm;
        const int kb = cold.basis[(size_t)(7 * seed % (uint64_t)M)];
        const double xk = cold.x[kb];
        if (seed % 4 < 2) hi[(size_t)kb] = lo[(size_t)kb] + 0.5 * (xk - lo[(size_t)kb]);
        else lo[(size_t)kb] = xk + 0.25;
        for (int rule = 0; rule < 3; ++rule) {
            for (int dual = 0; dual < 2; ++dual) {
                const Solver::PivotRule pr = (Solver::PivotRule)rule;
                const Solver::DualRule dr = (Solver::DualRule)dual;
                const Solver::BoundedResult g = s.boundedResolveLarge(lo, hi, cold, pr, dr, Solver::DualRatio::LongStep, false);
                std::vector<double> x((size_t)N, std::nan(""));
                std::vector<int> basis((size_t)M), up((size_t)N);
                double obj = std::nan("");
                int it[3];
                const int st = ref(A.data(), M, N, b.data(), c.data(), lo.data(), hi.data(), cold.basis.data(),
                                   cold.atUpper.data(), maximize ? 1 : 0, N, Solver::EPS, Solver::MAX_ITER, x.data(),
                                   basis.data(), up.data(), &obj, it, rule, dual, LP_DUAL_RATIO_LONG_STEP);
                if (rule == 0)
                    std::printf("  %d x %d seed %d dual rule %d: status %d, iterations %d + %d, %d flips\n", M, N, (int)seed,
                                dual, g.status, g.iterations[0], g.iterations[1], g.iterations[2]);
                CHECK(st == g.status);
                CHECK(same_value(obj, g.objective));
                for (int j = 0; j < N; ++j) CHECK(same_value(x[(size_t)j], g.x[j]) && up[(size_t)j] == g.atUpper[(size_t)j]);
                CHECK(basis == g.basis);
                for (int q = 0; q < 3; ++q) CHECK(it[q] == g.iterations[q]);
                CHECK(g.iterations[3] == 0);
                if (rule == 0 && it[0] > 0 && it[2] > 0) ++*flipped;
                // the textbook ratio test is the overload without one
                CHECK(same_result(s.boundedResolveLarge(lo, hi, cold, pr, dr, Solver::DualRatio::Textbook, false),
                                  s.boundedResolveLarge(lo, hi, cold, pr, dr, false)));
                if (lds) {
                    CHECK(same_result(s.boundedResolve(lo, hi, cold, pr, dr, Solver::DualRatio::LongStep, false), g));
                    CHECK(same_result(s.boundedResolve(lo, hi, cold, pr, dr, Solver::DualRatio::Textbook, false),
                                      s.boundedResolve(lo, hi, cold, pr, dr, false)));
                } else {
                    CHECK_THROWS(s.boundedResolve(lo, hi, cold, pr, dr, Solver::DualRatio::LongStep, false), std::invalid_argument);
                }
            }
        }
    }
}

TEST(BoundedResolveLongStep_LdsShape) {
    const RefLib lib("LP_BOUNDED_RESOLVE_LONG_STEP_REF");
    RefBoundedResolveLong ref = lib.symbol<RefBoundedResolveLong>("ref_bounded_resolve_long_step");
    int warm = 0, flipped = 0;
    run_shape(ref, 32, 64, true, &warm, &flipped);
    CHECK(warm >= 2);
    CHECK(flipped >= 1);
}

TEST(BoundedResolveLongStep_BeyondLds) {
    const RefLib lib("LP_BOUNDED_RESOLVE_LONG_STEP_REF");
    RefBoundedResolveLong ref = lib.symbol<RefBoundedResolveLong>("ref_bounded_resolve_long_step");
    int warm = 0, flipped = 0;
    run_shape(ref, 160, 160, false, &warm, &flipped);
    CHECK(warm >= 2);
    CHECK(flipped >= 1);
}

TEST(BoundedResolveLongStep_UnknownRatio) {
    std::vector<double> lo, hi;
    Solver s(boxed_problem(2, 32, 64, true, nullptr, nullptr, nullptr, &lo, &hi, 0.0, 0.125));
    const Solver::BoundedResult cold = s.boundedSimplexLarge(lo, hi);
    CHECK_THROWS(s.boundedResolve(lo, hi, cold, Solver::PivotRule::Dantzig, Solver::DualRule::Dantzig, (Solver::DualRatio)2, false),
                 std::invalid_argument);
    CHECK_THROWS(s.boundedResolveLarge(lo, hi, cold, Solver::PivotRule::Dantzig, Solver::DualRule::Devex, (Solver::DualRatio)-1, false),
                 std::invalid_argument);
    CHECK(s.boundedResolve(lo, hi, cold, Solver::PivotRule::Dantzig, Solver::DualRule::Dantzig, Solver::DualRatio::LongStep).status == LP_OPTIMAL);
}

int main(int argc, char** argv) { return run_all(argc > 1 ? argv[1] : nullptr); }
