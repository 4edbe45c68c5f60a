// GPU tests of Solver::parametricCost: after twoPhaseSimplex_ex() on MIN canonical problems the parametric cost path
// from the final basis equals tests/ref/parametric_cost_ref.c's bit for bit (the library named by
// LP_PARAMETRIC_COST_REF, loaded at run time), and the path is concave.
#include <cmath>
#include <cstdint>

#include "check.h"
#include "fixtures.h"
#include "Canonical.h"
#include "SimplexSolover.h"

using lpla::MatrixXd;
using lpla::VectorXd;

typedef int (*RefParametricCost)(const double*, int, int, const double*, const double*, const int*, int,
                                 const double*, double, double, int, int*, double*, double*, double*, int*, int*,
                                 int*);

// a seeded cost direction with mixed signs, scaled by |c| (0.5 where c_j = 0); positive = true takes |g|
static VectorXd direction(uint64_t seed, const VectorXd& c, bool positive) {
    uint64_t s = seed * 104729 + 5;
    VectorXd g(c.size());
    for (long j = 0; j < c.size(); ++j) {
        g[j] = (2.0 * u01(s) - 1.0) * (c[j] != 0.0 ? std::fabs(c[j]) : 0.5);
        if (positive) g[j] = std::fabs(g[j]);
    }
    return g;
}

TEST(ParametricCost_MatchesTheRef) {
    const RefLib lib("LP_PARAMETRIC_COST_REF");
    RefParametricCost ref = lib.symbol<RefParametricCost>("ref_parametric_cost");
    int multi = 0, unbounded = 0;
    for (uint64_t seed = 0; ref && seed < 24; ++seed) {
        const int m = 3 + (int)(seed % 9), k = 4 + (int)(seed % 13), n = k + m;
        MatrixXd A;
        VectorXd b, c;
        Canonical primal = min_problem(300 + seed, m, k, &A, &b, &c);
        Solver ps(primal);
        const Solver::Result pr = ps.twoPhaseSimplex_ex();
        CHECK(pr.status == LP_OPTIMAL);
        const VectorXd g = direction(seed, c, seed % 2 == 0);
        const double t_max = seed % 3 == 2 ? 0.5 : INFINITY;
        const Solver::Parametric p = ps.parametricCost(pr, g, t_max);
        const int MB = Solver::MAX_BREAKS;
        std::vector<double> t(MB + 2), obj(MB + 2), slope(MB + 1);
        std::vector<int> enter(MB + 1), leave(MB + 1), basis((size_t)m);
        int nseg = -1;
        const int st = ref(A.data(), m, n, b.data(), c.data(), pr.basis.data(), /*maximize=*/0, g.data(), t_max,
                           Solver::EPS, MB, &nseg, t.data(), obj.data(), slope.data(), enter.data(), leave.data(),
                           basis.data());
        CHECK(st == p.status);
        CHECK(nseg >= 1 && (long)p.slope.size() == nseg && (long)p.t.size() == nseg + 1);
        for (int q = 0; q <= nseg; ++q) CHECK(same_bits(p.t[q], t[(size_t)q]) && same_bits(p.obj[q], obj[(size_t)q]));
        for (int q = 0; q < nseg; ++q) {
            CHECK(same_bits(p.slope[q], slope[(size_t)q]));
            CHECK(p.enter[(size_t)q] == enter[(size_t)q] && p.leave[(size_t)q] == leave[(size_t)q]);
            if (q + 1 < nseg) CHECK(p.slope[q + 1] <= p.slope[q] + 1e-9 * (1 + std::fabs(p.slope[q])));   // concave
        }
        CHECK(p.basis == basis);
        if (nseg >= 3) ++multi;
        if (st == LP_UNBOUNDED) ++unbounded;
    }
    CHECK(multi > 0);
    CHECK(unbounded > 0);
}

TEST(ParametricCost_NotOptimalHasNoSegments) {
    MatrixXd A;
    VectorXd b, c;
    Canonical primal = min_problem(3, 4, 5, &A, &b, &c);
    Solver s(primal);
    Solver::Result r = s.twoPhaseSimplex_ex();
    const VectorXd g = direction(3, c, false);
    r.status = LP_INFEASIBLE;
    const Solver::Parametric p = s.parametricCost(r, g, INFINITY);
    CHECK(p.status == LP_INFEASIBLE && p.t.size() == 0 && p.slope.size() == 0 && p.enter.empty());
    r.status = LP_OPTIMAL;
    r.basis[1] = r.basis[0];   // repeated index: singular
    const Solver::Parametric e = s.parametricCost(r, g, INFINITY);
    CHECK(e.status == LP_SINGULAR && e.t.size() == 0 && e.basis == r.basis);
    r.basis[1] = 1000;         // out of range
    CHECK_THROWS(s.parametricCost(r, g, INFINITY), std::invalid_argument);
    CHECK_THROWS(s.parametricCost(r, VectorXd::Zero(3), INFINITY), std::invalid_argument);
}

int main(int argc, char** argv) { return run_all(argc > 1 ? argv[1] : nullptr); }
