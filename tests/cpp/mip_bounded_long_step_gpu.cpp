// GPU tests of Solver::boundedBranchAndBound and Solver::boundedBranchAndBoundLarge under a dual ratio test: on 8 x 20
// boxed problems with every structural column integer and on 67 x 201 ones with every other, the search from an optimal
// Solver::boundedSimplexLarge result under DualRatio::LongStep equals tests/ref/mip_bounded_long_step_ref.c's bit for bit
// (the library named by LP_MIP_BOUNDED_LONG_STEP_REF, loaded at run time), with 0 and 3 snapshots in HBM and through the
// LDS form, which must agree with the HBM form without snapshots; DualRatio::Textbook is the overload
// without a ratio test; an unknown ratio throws std::invalid_argument.  (No test_ prefix:
// tests/test_mip_bounded_long_step_cpp.py runs this program.)
#include <cmath>
#include <cstdint>

#include "check.h"
#include "fixtures.h"
#include "Canonical.h"
#include "SimplexSolover.h"

using lpla::MatrixXd;
using lpla::VectorXd;

typedef int (*RefMipBoundedLongStep)(const double*, int, int, const double*, const double*, const double*,
                                     const double*, const int*, const int*, int, int, const int*, double, double,
                                     double, int, int, int, double*, double*, double*, int*, int*, int, int*, int);

// boxed_problem with the columns j < K, j a multiple of `every`, integer: their bounds rounded outward
static Canonical mixed_problem(uint64_t seed, int M, int K, int every, bool maximize, MatrixXd* A, VectorXd* b,
                               VectorXd* c, std::vector<double>* lo, std::vector<double>* hi, std::vector<bool>* mask) {
    Canonical can = boxed_problem(seed, M, K, maximize, A, b, c, lo, hi, /*a_offset=*/0.0, /*b_scale=*/0.125);
    mask->assign((size_t)(M + K), false);
    for (int j = 0; j < K; j += every) {
        (*mask)[(size_t)j] = true;
        (*lo)[(size_t)j] = std::floor((*lo)[(size_t)j]);
        if (std::isfinite((*hi)[(size_t)j])) (*hi)[(size_t)j] = std::ceil((*hi)[(size_t)j]);
    }
    return can;
}

static bool same_search(const Solver::IntegerResult& a, const Solver::IntegerResult& b) {
    bool ok = a.status == b.status && a.found == b.found && a.nodes == b.nodes && a.restored == b.restored &&
              a.rebuilt == b.rebuilt && same_value(a.objective, b.objective) && same_value(a.bound, b.bound);
    for (int j = 0; ok && j < (int)a.x.size(); ++j) ok = same_value(a.x[j], b.x[j]);
    return ok;
}

// One shape: seeds 1 .. seeds under DualRatio::LongStep against the reference; *flips sums the reference's flip counts
static void run_shape(RefMipBoundedLongStep ref, int M, int K, int every, int seeds, int depth, int nodes, bool lds,
                      int* searched, int* flips) {
    const int N = M + K;
    for (uint64_t seed = 1; ref && seed <= (uint64_t)seeds; ++seed) {
        const bool maximize = seed % 2 == 0;
        MatrixXd A;
        VectorXd b, c;
        std::vector<double> lo, hi;
        std::vector<bool> mask;
        Solver s(mixed_problem(seed, M, K, every, maximize, &A, &b, &c, &lo, &hi, &mask));
        const Solver::BoundedResult cold = s.boundedSimplexLarge(lo, hi, /*throw_on_failure=*/false);
        if (cold.status != LP_OPTIMAL) continue;
        const std::vector<int> imask(mask.begin(), mask.end());
        const int ks[2] = {0, 3};
        for (int q = 0; q < 2; ++q) {
            const Solver::IntegerResult g =
                s.boundedBranchAndBoundLarge(mask, lo, hi, cold, depth, nodes, ks[q], Solver::DualRatio::LongStep);
            std::vector<double> x((size_t)N, std::nan(""));
            double obj = std::nan(""), bound = std::nan("");
            int found = 0, stats[7];
            const int st = ref(A.data(), M, N, b.data(), c.data(), lo.data(), hi.data(), cold.basis.data(),
                               cold.atUpper.data(), maximize ? 1 : 0, N, imask.data(), Solver::EPS, Solver::INT_TOL,
                               Solver::MIP_GAP, depth, nodes, Solver::MAX_ITER, x.data(), &obj, &bound, &found, stats,
                               ks[q], nullptr, LP_DUAL_RATIO_LONG_STEP);
            std::printf("  %d x %d seed %d, %d snapshots: status %d, %d nodes, %d restored, %d rebuilt, %d flips\n", M,
                        N, (int)seed, ks[q], g.status, g.nodes, g.restored, g.rebuilt, stats[3]);
            CHECK(st == g.status);
            CHECK((found != 0) == g.found && stats[0] == g.nodes);
            CHECK(stats[5] == g.restored && stats[6] == g.rebuilt);
            CHECK(same_value(obj, g.objective) && same_value(bound, g.bound));
            for (int j = 0; j < N; ++j) CHECK(same_value(x[(size_t)j], g.x[j]));
            if (stats[0] > 1) ++*searched;
            *flips += stats[3];
            // the textbook ratio test is the overload without one
            CHECK(same_search(s.boundedBranchAndBoundLarge(mask, lo, hi, cold, depth, nodes, ks[q],
                                                           Solver::DualRatio::Textbook),
                              s.boundedBranchAndBoundLarge(mask, lo, hi, cold, depth, nodes, ks[q])));
            if (q == 0 && lds) {   // the LDS form: the same search (it does not count the second children by kind)
                Solver::IntegerResult l = s.boundedBranchAndBound(mask, lo, hi, cold, depth, nodes, Solver::DualRatio::LongStep);
                CHECK(l.restored == 0 && l.rebuilt == 0);
                l.rebuilt = g.rebuilt;
                CHECK(same_search(l, g));
                CHECK(same_search(s.boundedBranchAndBound(mask, lo, hi, cold, depth, nodes, Solver::DualRatio::Textbook),
                                  s.boundedBranchAndBound(mask, lo, hi, cold, depth, nodes)));
            }
        }
    }
}

TEST(BoundedBranchAndBoundLongStep_8x20) {
    const RefLib lib("LP_MIP_BOUNDED_LONG_STEP_REF");
    RefMipBoundedLongStep ref = lib.symbol<RefMipBoundedLongStep>("ref_mip_bounded_long_step");
    CHECK(lp_mip_bounded_fits(8, 20, 32) == 1);
    int searched = 0, flips = 0;
    run_shape(ref, 8, 12, 1, 8, 32, 200, true, &searched, &flips);
    CHECK(searched >= 4);
    CHECK(flips >= 1);
}

TEST(BoundedBranchAndBoundLongStep_67x201) {
    const RefLib lib("LP_MIP_BOUNDED_LONG_STEP_REF");
    RefMipBoundedLongStep ref = lib.symbol<RefMipBoundedLongStep>("ref_mip_bounded_long_step");
    CHECK(lp_mip_bounded_fits(67, 201, 64) == 1);   // (an odd row length: 202 columns padded to 208 in HBM)
    int searched = 0, flips = 0;
    run_shape(ref, 67, 134, 2, 4, 64, 40, true, &searched, &flips);
    CHECK(searched >= 2);
    CHECK(flips >= 1);
}

TEST(BoundedBranchAndBoundLongStep_UnknownRatio) {
    std::vector<double> lo, hi;
    std::vector<bool> mask;
    Solver s(mixed_problem(2, 8, 12, 1, true, nullptr, nullptr, nullptr, &lo, &hi, &mask));
    const Solver::BoundedResult cold = s.boundedSimplexLarge(lo, hi);
    CHECK_THROWS(s.boundedBranchAndBound(mask, lo, hi, cold, 32, 100, (Solver::DualRatio)2), std::invalid_argument);
    CHECK_THROWS(s.boundedBranchAndBoundLarge(mask, lo, hi, cold, 32, 100, 3, (Solver::DualRatio)-1), std::invalid_argument);
    CHECK_THROWS(s.boundedBranchAndBoundLarge(mask, lo, hi, cold, 32, 100, -1, Solver::DualRatio::LongStep), std::invalid_argument);
    // the context still solves
    const Solver::IntegerResult g = s.boundedBranchAndBound(mask, lo, hi, cold, 32, 5, Solver::DualRatio::LongStep);
    CHECK(g.nodes >= 1 && g.nodes <= 5);
}

int main(int argc, char** argv) { return run_all(argc > 1 ? argv[1] : nullptr); }
