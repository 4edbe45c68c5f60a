// GPU tests of the Solver::boundedSimplex and Solver::boundedResolve overloads that take a pivot rule, on Beale's
// cycling LP (Chvatal's form) with every column boxed to [0, 100]: Dantzig's rule cycles until the iteration limit, in
// the cold solve and in the re-solve from the slack basis; Bland's rule and Devex pricing end optimal with the pivot
// counts of tests/ref/bounded_rules_ref.c.  The overloads without a rule ignore setPivotRule.
#include <stdexcept>
#include <vector>

#include "check.h"
#include "Canonical.h"
#include "Common.h"
#include "SimplexSolover.h"

using lpla::MatrixXd;
using lpla::VectorXd;
typedef Solver::PivotRule Rule;

static Canonical beale(bool maximize) {
    // max 10x1 - 57x2 - 9x3 - 24x4 s.t. the two degenerate rows and x1 <= 1, slack basis {4, 5, 6}
    const double a[3][7] = {{0.5, -5.5, -2.5, 9, 1, 0, 0}, {0.5, -1.5, -0.5, 1, 0, 1, 0}, {1, 0, 0, 0, 0, 0, 1}};
    MatrixXd A(3, 7);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 7; ++j) A(i, j) = a[i][j];
    VectorXd b(3), c(7);
    b[0] = 0; b[1] = 0; b[2] = 1;
    const double c0[7] = {10, -57, -9, -24, 0, 0, 0};
    for (int j = 0; j < 7; ++j) c[j] = maximize ? c0[j] : -c0[j];
    Canonical can(A, b, c, {4, 5, 6}, /*minimize=*/!maximize);
    can.SetOriginalVariablesCount(4);
    return can;
}

static const std::vector<double> LO(7, 0.0), HI(7, 100.0);

static bool is_vertex(const Solver::BoundedResult& r, bool maximize) {
    return r.status == LP_OPTIMAL && r.objective == (maximize ? 1.0 : -1.0) && r.x.size() == 4 && r.x[0] == 1 &&
           r.x[1] == 0 && r.x[2] == 1 && r.x[3] == 0;
}

TEST(BoundedRules_ColdSolveOfBealeBoxed) {
    for (bool maximize : {true, false}) {
        Solver s(beale(maximize));
        const Solver::BoundedResult d = s.boundedSimplex(LO, HI, Rule::Dantzig, false);
        CHECK(d.status == LP_ITER_LIMIT && d.iterations[0] == 4 && d.iterations[2] == Solver::MAX_ITER);
        CHECK_THROWS(s.boundedSimplex(LO, HI, Rule::Dantzig), std::runtime_error);
        const Solver::BoundedResult bl = s.boundedSimplex(LO, HI, Rule::Bland);
        CHECK(is_vertex(bl, maximize));
        CHECK(bl.iterations[0] == 3 && bl.iterations[1] == 0 && bl.iterations[2] == 2 && bl.iterations[3] == 0);
        const Solver::BoundedResult dv = s.boundedSimplex(LO, HI, Rule::Devex);
        CHECK(is_vertex(dv, maximize));
        CHECK(dv.iterations[0] == 4 && dv.iterations[1] == 0 && dv.iterations[2] == 1 && dv.iterations[3] == 0);
        // the overload without a rule stays with Dantzig's whatever setPivotRule says
        s.setPivotRule(Rule::Bland);
        const Solver::BoundedResult plain = s.boundedSimplex(LO, HI, false);
        CHECK(plain.status == LP_ITER_LIMIT && plain.basis == d.basis && plain.atUpper == d.atUpper);
        for (int k = 0; k < 4; ++k) CHECK(plain.iterations[k] == d.iterations[k]);
    }
}

TEST(BoundedRules_ResolveOfBealeBoxedFromTheSlackBasis) {
    for (bool maximize : {true, false}) {
        Solver s(beale(maximize));
        Solver::BoundedResult start;
        start.basis = {4, 5, 6};
        start.atUpper.assign(7, 0);
        const Solver::BoundedResult d = s.boundedResolve(LO, HI, start, Rule::Dantzig, false);
        CHECK(d.status == LP_ITER_LIMIT && d.iterations[0] == 0 && d.iterations[1] == Solver::MAX_ITER);
        const Solver::BoundedResult bl = s.boundedResolve(LO, HI, start, Rule::Bland);
        CHECK(is_vertex(bl, maximize));
        CHECK(bl.iterations[0] == 0 && bl.iterations[1] == 7 && bl.iterations[2] == 0);
        const Solver::BoundedResult dv = s.boundedResolve(LO, HI, start, Rule::Devex);
        CHECK(is_vertex(dv, maximize));
        CHECK(dv.iterations[0] == 0 && dv.iterations[1] == 3 && dv.iterations[2] == 0);
        s.setPivotRule(Rule::Devex);
        const Solver::BoundedResult plain = s.boundedResolve(LO, HI, start, false);
        CHECK(plain.status == LP_ITER_LIMIT && plain.basis == d.basis && plain.atUpper == d.atUpper);
        // an optimal result fed back under a rule is optimal at once
        const Solver::BoundedResult again = s.boundedResolve(LO, HI, bl, Rule::Bland);
        CHECK(is_vertex(again, maximize) && again.iterations[1] == 0 && again.basis == bl.basis);
    }
}

TEST(BoundedRules_WrongSizesThrow) {
    Solver s(beale(true));
    CHECK_THROWS(s.boundedSimplex(std::vector<double>(6, 0.0), HI, Rule::Bland), std::invalid_argument);
    Solver::BoundedResult bad;
    bad.basis = {4, 5};
    bad.atUpper.assign(7, 0);
    CHECK_THROWS(s.boundedResolve(LO, HI, bad, Rule::Devex), std::invalid_argument);
}

int main(int argc, char** argv) { return run_all(argc > 1 ? argv[1] : nullptr); }
