// GPU tests of Solver::boundedBranchAndBoundLarge with snapshots: on 4 x 14 boxed problems with every structural column
// integer and on a 160 x 320 one with every other, the search from an optimal Solver::boundedSimplexLarge result with 0,
// 3 and maxDepth snapshots equals tests/ref/mip_bounded_snapshots_ref.c's bit for bit, the restored and rebuilt counts
// included (the library named by LP_MIP_BOUNDED_SNAPSHOTS_REF, loaded at run time); 0 snapshots is the form without
// the argument; the form that solves the relaxation itself agrees; a snapshot count outside [0, 1024] throws
// std::invalid_argument.  (No test_ prefix: tests/test_mip_bounded_snapshots_cpp.py runs this program.)
#include <cmath>
#include <cstdint>

#include "check.h"
#include "fixtures.h"
#include "Canonical.h"
#include "SimplexSolover.h"

using lpla::MatrixXd;
using lpla::VectorXd;

typedef int (*RefMipBoundedSnapshots)(const double*, int, int, const double*, const double*, const double*,
                                      const double*, const int*, const int*, int, int, const int*, double, double,
                                      double, int, int, int, double*, double*, double*, int*, int*, int, int*);

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

// One shape: seeds 1 .. seeds, each with 0, 3 and depth snapshots against the reference; counts what was reached
static void run_shape(RefMipBoundedSnapshots ref, int M, int K, int every, int seeds, int depth, int nodes,
                      int* restored, int* rebuilt) {
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
        const int ks[3] = {0, 3, depth};
        for (int q = 0; q < 3; ++q) {
            const Solver::IntegerResult g = s.boundedBranchAndBoundLarge(mask, lo, hi, cold, depth, nodes, ks[q]);
            std::vector<double> x((size_t)N, std::nan(""));
            double obj = std::nan(""), bound = std::nan("");
            int found = 0, stats[7];
            const int st = ref(A.data(), M, N, b.data(), c.data(), lo.data(), hi.data(), cold.basis.data(),
                               cold.atUpper.data(), maximize ? 1 : 0, N, imask.data(), Solver::EPS, Solver::INT_TOL,
                               Solver::MIP_GAP, depth, nodes, Solver::MAX_ITER, x.data(), &obj, &bound, &found, stats,
                               ks[q], nullptr);
            std::printf("  %d x %d seed %d, %d snapshots: status %d, %d nodes, %d restored, %d rebuilt\n", M, N,
                        (int)seed, ks[q], g.status, g.nodes, g.restored, g.rebuilt);
            CHECK(st == g.status);
            CHECK((found != 0) == g.found && stats[0] == g.nodes);
            CHECK(stats[5] == g.restored && stats[6] == g.rebuilt);
            CHECK(same_value(obj, g.objective) && same_value(bound, g.bound));
            for (int j = 0; j < N; ++j) CHECK(same_value(x[(size_t)j], g.x[j]));
            if (ks[q] == 0) {   // the form without the argument
                const Solver::IntegerResult old = s.boundedBranchAndBoundLarge(mask, lo, hi, cold, depth, nodes);
                CHECK(old.status == g.status && old.nodes == g.nodes && old.found == g.found);
                CHECK(same_value(old.objective, g.objective) && same_value(old.bound, g.bound));
                for (int j = 0; j < N; ++j) CHECK(same_value(old.x[j], g.x[j]));
                CHECK(old.restored == 0 && old.rebuilt == 0 && g.restored == 0);
            }
            if (ks[q] == depth) CHECK(g.rebuilt == 0);
            if (ks[q] == 3) {
                *restored += g.restored;
                *rebuilt += g.rebuilt;
                // the form that solves the relaxation first
                const Solver::IntegerResult own = s.boundedBranchAndBoundLarge(mask, lo, hi, depth, nodes, 3);
                CHECK(own.status == g.status && own.nodes == g.nodes && own.restored == g.restored);
                CHECK(same_value(own.objective, g.objective));
            }
        }
    }
}

TEST(BoundedBranchAndBoundLargeSnapshots_4x14) {
    const RefLib lib("LP_MIP_BOUNDED_SNAPSHOTS_REF");
    RefMipBoundedSnapshots ref = lib.symbol<RefMipBoundedSnapshots>("ref_mip_bounded_snapshots");
    int restored = 0, rebuilt = 0;
    run_shape(ref, 4, 10, 1, 8, 24, 400, &restored, &rebuilt);
    CHECK(restored >= 4);
    CHECK(rebuilt >= 1);
}

TEST(BoundedBranchAndBoundLargeSnapshots_160x320) {
    const RefLib lib("LP_MIP_BOUNDED_SNAPSHOTS_REF");
    RefMipBoundedSnapshots ref = lib.symbol<RefMipBoundedSnapshots>("ref_mip_bounded_snapshots");
    CHECK(lp_mip_bounded_fits(160, 320, 0) == 0);
    int restored = 0, rebuilt = 0;
    run_shape(ref, 160, 160, 2, 4, 64, 40, &restored, &rebuilt);
    CHECK(restored >= 2);
}

TEST(BoundedBranchAndBoundLargeSnapshots_BadArguments) {
    std::vector<double> lo, hi;
    std::vector<bool> mask;
    Solver s(mixed_problem(2, 4, 10, 1, true, nullptr, nullptr, nullptr, &lo, &hi, &mask));
    const Solver::BoundedResult cold = s.boundedSimplexLarge(lo, hi);
    CHECK_THROWS(s.boundedBranchAndBoundLarge(mask, lo, hi, cold, 24, 100, 1025), std::invalid_argument);
    CHECK_THROWS(s.boundedBranchAndBoundLarge(mask, lo, hi, cold, 1025, 100, 3), std::invalid_argument);
    CHECK_THROWS(s.boundedBranchAndBoundLarge(mask, lo, hi, cold, 24, 0, 3), std::invalid_argument);
    unsigned long long bytes = 0;
    CHECK(lp_mip_bounded_snapshot_bytes(4, 14, 3, &bytes) == LP_OPTIMAL && bytes == 3ull * 8 * (5 * 16 + 2 * 14));
    CHECK(lp_mip_bounded_snapshot_bytes(4, 14, 3, nullptr) == LP_BAD_ARG);
    // the context still solves
    const Solver::IntegerResult g = s.boundedBranchAndBoundLarge(mask, lo, hi, cold, 24, 5, 3);
    CHECK(g.nodes >= 1 && g.nodes <= 5);
}

int main(int argc, char** argv) { return run_all(argc > 1 ? argv[1] : nullptr); }
