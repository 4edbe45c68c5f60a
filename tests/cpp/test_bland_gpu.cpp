// GPU tests of Solver::setPivotRule: Bland's rule solves Beale's cycling LP (Chvatal's form), which the
// default rule (Dantzig's) cycles on until the iteration limit.
#include "check.h"
#include "Canonical.h"
#include "Common.h"
#include "SimplexSolover.h"

using lpla::MatrixXd;
using lpla::VectorXd;

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

TEST(Bland_SolvesBeale) {
    Solver s(beale(true));
    CHECK(s.pivotRule() == Solver::PivotRule::Dantzig);
    s.setPivotRule(Solver::PivotRule::Bland);
    VectorXd x = s.solve();
    CHECK(x.size() == 4 && x[0] == 1 && x[1] == 0 && x[2] == 1 && x[3] == 0);
    auto r = s.solve_ex();
    CHECK(r.status == LP_OPTIMAL && r.objective == 1 && r.iterations == 7);
}
TEST(Dantzig_CyclesOnBeale) {
    CHECK_THROWS(Solver(beale(true)).solve(), std::runtime_error);
    auto r = Solver(beale(true)).solve_ex(false);
    CHECK(r.status == LP_ITER_LIMIT && r.iterations == Solver::MAX_ITER);
}
TEST(Bland_TwoPhaseBeale) {
    for (bool maximize : {true, false}) {
        Solver s(beale(maximize));
        s.setPivotRule(Solver::PivotRule::Bland);
        int it[3] = {0, 0, 0};
        auto r = s.twoPhaseSimplex_ex(true, it);
        CHECK(r.status == LP_OPTIMAL && r.objective == (maximize ? 1.0 : -1.0));
        CHECK(r.x[0] == 1 && r.x[1] == 0 && r.x[2] == 1 && r.x[3] == 0);
        CHECK(r.iterations == it[0] + it[1] + it[2]);
        auto d = Solver(beale(maximize)).twoPhaseSimplex_ex(false);
        CHECK(d.status == LP_ITER_LIMIT);
    }
}

int main(int argc, char** argv) { return run_all(argc > 1 ? argv[1] : nullptr); }
