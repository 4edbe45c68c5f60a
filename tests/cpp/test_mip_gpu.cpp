// GPU tests of Solver::branchAndBound: after twoPhaseSimplex_ex() on MIN canonical problems the search from the final
// basis equals tests/ref/mip_ref.c's bit for bit (the library named by LP_MIP_REF, loaded at run time), and the form
// that starts from the problem's own basis agrees with the reference from that basis.
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
        b[i] = 1.0 + 3.0 * u01(s);
    }
    for (int j = 0; j < k; ++j) c[j] = 0.1 + u01(s);
    std::vector<int> basis((size_t)m);
    for (int i = 0; i < m; ++i) basis[(size_t)i] = k + i;   // dual feasible for min with c >= 0
    *Aout = A;
    *bout = b;
    *cout = c;
    Canonical can(A, b, c, basis, /*minimize=*/true);
    can.SetOriginalVariablesCount(k + m);
    return can;
}

typedef int (*RefMip)(const double*, int, int, const double*, const double*, const int*, int, int, const int*, double,
                      double, double, int, int, int, double*, double*, double*, int*, int*);

static bool same_value(double a, double b) { return (std::isnan(a) && std::isnan(b)) || a == b; }

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
    const char* path = std::getenv("LP_MIP_REF");
    CHECK(path != nullptr);
    if (!path) return;
    void* h = dlopen(path, RTLD_NOW | RTLD_LOCAL);
    CHECK(h != nullptr);
    if (!h) return;
    RefMip ref = reinterpret_cast<RefMip>(dlsym(h, "ref_mip"));
    CHECK(ref != nullptr);
    int branched = 0, optimal = 0;
    for (uint64_t seed = 0; ref && seed < 16; ++seed) {
        const int m = 3 + (int)(seed % 4), k = 4 + (int)(seed % 5), n = k + m;
        MatrixXd A;
        VectorXd b, c;
        Canonical primal = min_problem(500 + seed, m, k, &A, &b, &c);
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
    dlclose(h);
}

TEST(BranchAndBound_NotOptimalAndBadMask) {
    MatrixXd A;
    VectorXd b, c;
    Canonical primal = min_problem(3, 4, 5, &A, &b, &c);
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
