// GPU tests of Solver::duals: on MIN canonical problems the dual of the reference's Canonical::GetDual()
// (max b.y, A^T y <= c with y = u - v free) is solved by twoPhaseSimplex(); the primal's Solver::duals must give
// y = u - v and d = the dual's slacks.
#include <cmath>
#include <cstdint>

#include "check.h"
#include "fixtures.h"
#include "Canonical.h"
#include "SimplexSolover.h"

using lpla::MatrixXd;
using lpla::VectorXd;

TEST(Duals_MatchTheSolvedDual) {
    int checked = 0;
    for (uint64_t seed = 0; seed < 24; ++seed) {
        const int m = 3 + (int)(seed % 9), k = 4 + (int)(seed % 13);
        Canonical primal = min_problem(seed, m, k);
        Solver ps(primal);
        const Solver::Result pr = ps.twoPhaseSimplex_ex();
        const Solver::Duals du = ps.duals(pr);
        CHECK(du.status == LP_OPTIMAL);
        CHECK(std::fabs(du.objective - pr.objective) <= 1e-9 * (1 + std::fabs(pr.objective)));   // strong duality
        std::unique_ptr<Canonical> dual = primal.GetDual();   // max b.(u - v), A^T (u - v) + s = c
        const int n = k + m;
        dual->SetOriginalVariablesCount(2 * m + n);           // the slacks too
        const Solver::Result dr = Solver(*dual).twoPhaseSimplex_ex();
        CHECK(dr.status == LP_OPTIMAL);
        CHECK(std::fabs(dr.objective - pr.objective) <= 1e-9 * (1 + std::fabs(pr.objective)));
        for (int i = 0; i < m; ++i) CHECK(std::fabs(du.y[i] - (dr.x[i] - dr.x[m + i])) <= 1e-9);
        for (int j = 0; j < n; ++j) {
            CHECK(std::fabs(du.d[j] - dr.x[2 * m + j]) <= 1e-9);
            CHECK(du.d[j] >= -Solver::EPS);                   // min at an optimum
        }
        for (int t = 0; t < m; ++t) CHECK(du.d[pr.basis[(size_t)t]] == 0.0);
        ++checked;
    }
    CHECK(checked == 24);
}

TEST(Duals_NotOptimalIsNaN) {
    Canonical primal = min_problem(3, 4, 5);
    Solver s(primal);
    Solver::Result r = s.twoPhaseSimplex_ex();
    r.status = LP_UNBOUNDED;
    const Solver::Duals d = s.duals(r);
    CHECK(d.status == LP_UNBOUNDED && std::isnan(d.objective) && std::isnan(d.y[0]) && std::isnan(d.d[0]));
    r.status = LP_OPTIMAL;
    r.basis[1] = r.basis[0];   // repeated index: singular
    const Solver::Duals e = s.duals(r);
    CHECK(e.status == LP_SINGULAR && std::isnan(e.y[0]));
    r.basis[1] = 1000;         // out of range
    CHECK_THROWS(s.duals(r), std::invalid_argument);
}

int main(int argc, char** argv) { return run_all(argc > 1 ? argv[1] : nullptr); }
