// GPU tests of Solver::branchAndBound: after twoPhaseSimplex_ex() on MIN canonical problems the search from the final
// basis equals tests/ref/mip_ref.c's bit for bit (the library named by LP_MIP_REF, loaded at run time), and the form
// that starts from the problem's own basis agrees with the reference from that basis.
#include <cmath>
#include <cstdint>

#include "check.h"
#include "fixtures.h"
#include "Canonical.h"
#include "SimplexSolover.h"

using lpla::MatrixXd;
using lpla::VectorXd;

typedef int (*RefMip)(const double*, int, int, const double*, const double*, const int*, int, int, const int*, double,
                      double, double, int, int, int, double*, double*, double*, int*, int*);

static void check_against(RefMip ref, const MatrixXd& A, const VectorXd& b, const VectorXd& c,
                          const std::vector<int>& basis, const std::vector<bool>& integer,
                          const Solver::IntegerResult& g, int* branched) {
    const int m = (int)A.rows(), n = (int)A.cols();
    std::vector<int> mask((size_t)n);
    for (int j = 0; j < n; ++j) mask[(size_t)j] = integer[(size_t)j] ? 1 : 0;
    std::vector<double> x((size_t)n);
    double obj = 0, bound = 0;
    int found = 0, stats[4] = {0, 0, 0, 0};
    const int st = ref(A.data(), m, n, b.data(), c.data(), basis.data(), /*maximize=*/0, n, mask.data(), Solver::EPS,
                       Solver::INT_TOL, Solver::MIP_GAP, 32, 100000, Solver::MAX_ITER, x.data(), &obj, &bound, &found,
                       stats);
    CHECK(st == g.status);
    CHECK((found != 0) == g.found);
    CHECK(stats[0] == g.nodes);
    CHECK(same_value(obj, g.objective) && same_value(bound, g.bound));
    CHECK((long)g.x.size() == n);
    for (int j = 0; j < n && j < (long)g.x.size(); ++j) CHECK(same_value(g.x[j], x[(size_t)j]));
    if (stats[0] > 1) ++*branched;
}

TEST(BranchAndBound_MatchesTheRef) {
    const RefLib lib("LP_MIP_REF");
    RefMip ref = lib.symbol<RefMip>("ref_mip");
    int branched = 0, optimal = 0;
    for (uint64_t seed = 0; ref && seed < 16; ++seed) {
        const int m = 3 + (int)(seed % 4), k = 4 + (int)(seed % 5), n = k + m;
        MatrixXd A;
        VectorXd b, c;
        Canonical primal = min_problem(500 + seed, m, k, &A, &b, &c, /*b_spread=*/3.0);
        Solver s(primal);
        std::vector<bool> integer((size_t)n, false);
        for (int j = 0; j < k; ++j) integer[(size_t)j] = seed % 3 != 1 || j % 2 == 0;   // some mixed masks
        const Solver::Result r = s.twoPhaseSimplex_ex();
        CHECK(r.status == LP_OPTIMAL);
        const Solver::IntegerResult g = s.branchAndBound(integer, r);
        check_against(ref, A, b, c, r.basis, integer, g, &branched);
        const Solver::IntegerResult own = s.branchAndBound(integer);
        check_against(ref, A, b, c, primal.GetBasisIndices(), integer, own, &branched);
        if (g.status == LP_OPTIMAL) {
            ++optimal;
            CHECK(g.objective == g.bound);
            for (int j = 0; j < k; ++j)
                if (integer[(size_t)j]) CHECK(std::fabs(g.x[j] - std::round(g.x[j])) <= Solver::INT_TOL);
        }
    }
    CHECK(branched > 0);
    CHECK(optimal > 0);
}

TEST(BranchAndBound_NotOptimalAndBadMask) {
    MatrixXd A;
    VectorXd b, c;
    Canonical primal = min_problem(3, 4, 5, &A, &b, &c, /*b_spread=*/3.0);
    Solver s(primal);
    Solver::Result r = s.twoPhaseSimplex_ex();
    std::vector<bool> integer(9, true);
    r.status = LP_INFEASIBLE;
    const Solver::IntegerResult g = s.branchAndBound(integer, r);
    CHECK(g.status == LP_INFEASIBLE && !g.found && std::isnan(g.objective) && g.nodes == 0);
    r.status = LP_OPTIMAL;
    CHECK_THROWS(s.branchAndBound(std::vector<bool>(3, true), r), std::invalid_argument);
}

int main(int argc, char** argv) { return run_all(argc > 1 ? argv[1] : nullptr); }
