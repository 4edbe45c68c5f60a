// GPU tests of Solver::parametricRhs: after twoPhaseSimplex_ex() on MIN canonical problems the parametric path from
// the final basis equals tests/ref/parametric_ref.c's bit for bit (the library named by LP_PARAMETRIC_REF, loaded at
// run time), and the path is continuous and convex.
#include <cmath>
#include <cstdint>

#include "check.h"
#include "fixtures.h"
#include "Canonical.h"
#include "SimplexSolover.h"

using lpla::MatrixXd;
using lpla::VectorXd;

typedef int (*RefParametric)(const double*, int, int, const double*, const double*, const int*, int, const double*,
                             double, double, int, int*, double*, double*, double*, int*, int*, int*);

// a seeded direction with mixed signs, scaled by |b|
static VectorXd direction(uint64_t seed, const VectorXd& b) {
    uint64_t s = seed * 104729 + 3;
    VectorXd d(b.size());
    for (long i = 0; i < b.size(); ++i) d[i] = (2.0 * u01(s) - 1.0) * std::fabs(b[i]);
    return d;
}

TEST(Parametric_MatchesTheRef) {
    const RefLib lib("LP_PARAMETRIC_REF");
    RefParametric ref = lib.symbol<RefParametric>("ref_parametric");
    int multi = 0;
    for (uint64_t seed = 0; ref && seed < 24; ++seed) {
        const int m = 3 + (int)(seed % 9), k = 4 + (int)(seed % 13), n = k + m;
        MatrixXd A;
        VectorXd b, c;
        Canonical primal = min_problem(200 + seed, m, k, &A, &b, &c);
        Solver ps(primal);
        const Solver::Result pr = ps.twoPhaseSimplex_ex();
        CHECK(pr.status == LP_OPTIMAL);
        const VectorXd d = direction(seed, b);
        const double t_max = seed % 3 == 2 ? 0.5 : INFINITY;
        const Solver::Parametric g = ps.parametricRhs(pr, d, t_max);
        const int MB = Solver::MAX_BREAKS;
        std::vector<double> t(MB + 2), obj(MB + 2), slope(MB + 1);
        std::vector<int> enter(MB + 1), leave(MB + 1), basis((size_t)m);
        int nseg = -1;
        const int st = ref(A.data(), m, n, b.data(), c.data(), pr.basis.data(), /*maximize=*/0, d.data(), t_max,
                           Solver::EPS, MB, &nseg, t.data(), obj.data(), slope.data(), enter.data(), leave.data(),
                           basis.data());
        CHECK(st == g.status);
        CHECK(nseg >= 1 && (long)g.slope.size() == nseg && (long)g.t.size() == nseg + 1);
        for (int q = 0; q <= nseg; ++q) CHECK(same_bits(g.t[q], t[(size_t)q]) && same_bits(g.obj[q], obj[(size_t)q]));
        for (int q = 0; q < nseg; ++q) {
            CHECK(same_bits(g.slope[q], slope[(size_t)q]));
            CHECK(g.enter[(size_t)q] == enter[(size_t)q] && g.leave[(size_t)q] == leave[(size_t)q]);
            if (q + 1 < nseg) CHECK(g.slope[q] <= g.slope[q + 1] + 1e-9 * (1 + std::fabs(g.slope[q])));   // convex
        }
        CHECK(g.basis == basis);
        if (nseg >= 3) ++multi;
    }
    CHECK(multi > 0);
}

TEST(Parametric_NotOptimalHasNoSegments) {
    MatrixXd A;
    VectorXd b, c;
    Canonical primal = min_problem(3, 4, 5, &A, &b, &c);
    Solver s(primal);
    Solver::Result r = s.twoPhaseSimplex_ex();
    const VectorXd d = direction(3, b);
    r.status = LP_UNBOUNDED;
    const Solver::Parametric g = s.parametricRhs(r, d, INFINITY);
    CHECK(g.status == LP_UNBOUNDED && g.t.size() == 0 && g.slope.size() == 0 && g.enter.empty());
    r.status = LP_OPTIMAL;
    r.basis[1] = r.basis[0];   // repeated index: singular
    const Solver::Parametric e = s.parametricRhs(r, d, INFINITY);
    CHECK(e.status == LP_SINGULAR && e.t.size() == 0 && e.basis == r.basis);
    r.basis[1] = 1000;         // out of range
    CHECK_THROWS(s.parametricRhs(r, d, INFINITY), std::invalid_argument);
}

int main(int argc, char** argv) { return run_all(argc > 1 ? argv[1] : nullptr); }
