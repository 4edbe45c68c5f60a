// GPU tests of Solver::parametricCost: after twoPhaseSimplex_ex() on MIN canonical problems the parametric cost path
// from the final basis equals tests/ref/parametric_cost_ref.c's bit for bit (the library named by
// LP_PARAMETRIC_COST_REF, loaded at run time), and the path is concave.
#include <dlfcn.h>

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "check.h"
#include "Canonical.h"
#include "SimplexSolover.h"

using lpla::MatrixXd;
using lpla::VectorXd;

static double u01(uint64_t& s) {   // splitmix64
    uint64_t z = (s += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    z ^= z >> 31;
    return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}

// min c.x, A0 x >= b, x >= 0 as [A0 | -I]: k originals, m surplus columns; c > 0 on the originals
static Canonical min_problem(uint64_t seed, int m, int k, MatrixXd* Aout, VectorXd* bout, VectorXd* cout) {
    uint64_t s = seed * 7919 + 17;
    MatrixXd A = MatrixXd::Zero(m, k + m);
    VectorXd b(m), c = VectorXd::Zero(k + m);
    for (int i = 0; i < m; ++i) {
        for (int j = 0; j < k; ++j) A(i, j) = u01(s);
        A(i, k + i) = -1.0;
        b[i] = 1.0 + u01(s);
    }
    for (int j = 0; j < k; ++j) c[j] = 0.1 + u01(s);
    std::vector<int> basis((size_t)m);
    for (int i = 0; i < m; ++i) basis[(size_t)i] = k + i;   // (ignored by the two-phase flow)
    *Aout = A;
    *bout = b;
    *cout = c;
    Canonical can(A, b, c, basis, /*minimize=*/true);
    can.SetOriginalVariablesCount(k + m);
    return can;
}

typedef int (*RefParametricCost)(const double*, int, int, const double*, const double*, const int*, int,
                                 const double*, double, double, int, int*, double*, double*, double*, int*, int*,
                                 int*);

static bool same_bits(double a, double b) {
    if (std::isnan(a) || std::isnan(b)) return std::isnan(a) && std::isnan(b);
    uint64_t x, y;
    std::memcpy(&x, &a, 8);
    std::memcpy(&y, &b, 8);
    return x == y;
}

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
    const char* path = std::getenv("LP_PARAMETRIC_COST_REF");
    CHECK(path != nullptr);
    if (!path) return;
    void* h = dlopen(path, RTLD_NOW | RTLD_LOCAL);
    CHECK(h != nullptr);
    if (!h) return;
    RefParametricCost ref = reinterpret_cast<RefParametricCost>(dlsym(h, "ref_parametric_cost"));
    CHECK(ref != nullptr);
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
    dlclose(h);
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
