// GPU tests of Solver::boundedBranchAndBound: on MIN canonical problems with integer boxes the search from a
// boundedSimplex result equals tests/ref/mip_bounded_ref.c's bit for bit (the library named by LP_MIP_BOUNDED_REF,
// loaded at run time), the form without a start solves the relaxation itself and gives the same result, and the
// refusals throw.
#include <cmath>
#include <cstdint>
#include <limits>

#include "check.h"
#include "fixtures.h"
#include "Canonical.h"
#include "SimplexSolover.h"

using lpla::MatrixXd;
using lpla::VectorXd;

// min c.x, A0 x >= b as [A0 | -I] with k originals in integer boxes [0 or 1, 3 .. 6] and m surplus columns in [0, inf).
// Not fixtures.h's min_problem (b_spread 3): the boxes are drawn from the same stream after the costs.
static Canonical min_problem(uint64_t seed, int m, int k, MatrixXd* Aout, VectorXd* bout, VectorXd* cout,
                             std::vector<double>* lo, std::vector<double>* hi) {
    uint64_t s = seed * 7919 + 17;
    MatrixXd A = MatrixXd::Zero(m, k + m);
    VectorXd b(m), c = VectorXd::Zero(k + m);
    for (int i = 0; i < m; ++i) {
        for (int j = 0; j < k; ++j) A(i, j) = u01(s);
        A(i, k + i) = -1.0;
        b[i] = 1.0 + 3.0 * u01(s);
    }
    for (int j = 0; j < k; ++j) c[j] = 0.1 + u01(s);
    lo->assign((size_t)(k + m), 0.0);
    hi->assign((size_t)(k + m), std::numeric_limits<double>::infinity());
    for (int j = 0; j < k; ++j) {
        (*lo)[(size_t)j] = u01(s) < 0.25 ? 1.0 : 0.0;
        (*hi)[(size_t)j] = 3.0 + std::floor(4.0 * u01(s));
    }
    std::vector<int> basis((size_t)m);
    for (int i = 0; i < m; ++i) basis[(size_t)i] = k + i;
    *Aout = A;
    *bout = b;
    *cout = c;
    Canonical can(A, b, c, basis, /*minimize=*/true);
    can.SetOriginalVariablesCount(k + m);
    return can;
}

typedef int (*RefMipBounded)(const double*, int, int, const double*, const double*, const double*, const double*,
                             const int*, const int*, int, int, const int*, double, double, double, int, int, int,
                             double*, double*, double*, int*, int*);

static void check_against(RefMipBounded ref, const MatrixXd& A, const VectorXd& b, const VectorXd& c,
                          const std::vector<double>& lo, const std::vector<double>& hi,
                          const Solver::BoundedResult& from, const std::vector<bool>& integer, int max_depth,
                          const Solver::IntegerResult& g, int* branched) {
    const int m = (int)A.rows(), n = (int)A.cols();
    std::vector<int> mask((size_t)n);
    for (int j = 0; j < n; ++j) mask[(size_t)j] = integer[(size_t)j] ? 1 : 0;
    std::vector<double> x((size_t)n);
    double obj = 0, bound = 0;
    int found = 0, stats[5] = {0, 0, 0, 0, 0};
    const int st = ref(A.data(), m, n, b.data(), c.data(), lo.data(), hi.data(), from.basis.data(),
                       from.atUpper.data(), /*maximize=*/0, n, mask.data(), Solver::EPS, Solver::INT_TOL,
                       Solver::MIP_GAP, max_depth, 100000, Solver::MAX_ITER, x.data(), &obj, &bound, &found, stats);
    CHECK(st == g.status);
    CHECK((found != 0) == g.found);
    CHECK(stats[0] == g.nodes);
    CHECK(same_value(obj, g.objective) && same_value(bound, g.bound));
    CHECK((long)g.x.size() == n);
    for (int j = 0; j < n && j < (long)g.x.size(); ++j) CHECK(same_value(g.x[j], x[(size_t)j]));
    if (stats[0] > 1) ++*branched;
}

TEST(BoundedBranchAndBound_MatchesTheRef) {
    const RefLib lib("LP_MIP_BOUNDED_REF");
    RefMipBounded ref = lib.symbol<RefMipBounded>("ref_mip_bounded");
    int branched = 0, optimal = 0;
    for (uint64_t seed = 0; ref && seed < 16; ++seed) {
        const int m = 3 + (int)(seed % 4), k = 4 + (int)(seed % 5), n = k + m;
        MatrixXd A;
        VectorXd b, c;
        std::vector<double> lo, hi;
        Canonical primal = min_problem(700 + seed, m, k, &A, &b, &c, &lo, &hi);
        Solver s(primal);
        std::vector<bool> integer((size_t)n, false);
        for (int j = 0; j < k; ++j) integer[(size_t)j] = seed % 3 != 1 || j % 2 == 0;   // some mixed masks
        const Solver::BoundedResult r = s.boundedSimplex(lo, hi, false);
        if (r.status != LP_OPTIMAL) {
            const Solver::IntegerResult skip = s.boundedBranchAndBound(integer, lo, hi, r);
            CHECK(skip.status == r.status && !skip.found && skip.nodes == 0);
            continue;
        }
        const int depth = seed % 2 ? 200 : 64;   // beyond the row form's cap on every other problem
        const Solver::IntegerResult g = s.boundedBranchAndBound(integer, lo, hi, r, depth);
        check_against(ref, A, b, c, lo, hi, r, integer, depth, g, &branched);
        const Solver::IntegerResult own = s.boundedBranchAndBound(integer, lo, hi, depth);
        check_against(ref, A, b, c, lo, hi, r, integer, depth, own, &branched);
        if (g.status == LP_OPTIMAL) {
            ++optimal;
            CHECK(g.objective == g.bound);
            for (int j = 0; j < k; ++j) {
                if (integer[(size_t)j]) CHECK(std::fabs(g.x[j] - std::round(g.x[j])) <= Solver::INT_TOL);
                CHECK(g.x[j] >= lo[(size_t)j] - 1e-9 && g.x[j] <= hi[(size_t)j] + 1e-9);
            }
        }
    }
    CHECK(branched > 0);
    CHECK(optimal > 0);
}

TEST(BoundedBranchAndBound_NotOptimalAndRefusals) {
    MatrixXd A;
    VectorXd b, c;
    std::vector<double> lo, hi;
    Canonical primal = min_problem(3, 4, 5, &A, &b, &c, &lo, &hi);
    Solver s(primal);
    Solver::BoundedResult r = s.boundedSimplex(lo, hi, false);
    CHECK(r.status == LP_OPTIMAL);
    std::vector<bool> integer(9, false);
    for (int j = 0; j < 5; ++j) integer[(size_t)j] = true;
    r.status = LP_INFEASIBLE;
    const Solver::IntegerResult g = s.boundedBranchAndBound(integer, lo, hi, r);
    CHECK(g.status == LP_INFEASIBLE && !g.found && std::isnan(g.objective) && g.nodes == 0);
    r.status = LP_OPTIMAL;
    CHECK_THROWS(s.boundedBranchAndBound(std::vector<bool>(3, true), lo, hi, r), std::invalid_argument);
    CHECK_THROWS(s.boundedBranchAndBound(integer, std::vector<double>(3, 0.0), hi, r), std::invalid_argument);
    CHECK_THROWS(s.boundedBranchAndBound(integer, lo, hi, r, 1025), std::invalid_argument);
    std::vector<double> frac = hi;
    frac[0] = 2.5;   // a marked column with a fractional upper bound
    CHECK_THROWS(s.boundedBranchAndBound(integer, lo, frac, r), std::invalid_argument);
    Solver::BoundedResult bad = r;
    bad.basis[0] = 9;   // outside the columns
    CHECK_THROWS(s.boundedBranchAndBound(integer, lo, hi, bad), std::invalid_argument);
}

int main(int argc, char** argv) { return run_all(argc > 1 ? argv[1] : nullptr); }
