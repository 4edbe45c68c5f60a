// GPU tests of Solver::ranging: after twoPhaseSimplex_ex() on MIN canonical problems the ranges at the final basis
// equal tests/ref/ranging_ref.c's bit for bit (the library named by LP_RANGING_REF, loaded at run time), and the
// basis stays optimal with b_i or c_j moved just inside either finite end.
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

// the basis stays optimal for (A, b, c) under the sense: B^-1 b >= 0 and reduced costs >= 0 (min)
static bool basis_optimal(const MatrixXd& A, const VectorXd& b, const VectorXd& c, const std::vector<int>& basis,
                          double tol) {
    const int m = (int)A.rows(), n = (int)A.cols();
    // solve B x = b and B^T y = c_B by Gauss-Jordan on small dense systems
    std::vector<double> M((size_t)m * (m + 2));
    for (int i = 0; i < m; ++i) {
        for (int t = 0; t < m; ++t) M[(size_t)i * (m + 2) + t] = A(i, basis[(size_t)t]);
        M[(size_t)i * (m + 2) + m] = b[i];
    }
    std::vector<double> MT((size_t)m * (m + 1));
    for (int t = 0; t < m; ++t) {
        for (int i = 0; i < m; ++i) MT[(size_t)t * (m + 1) + i] = A(i, basis[(size_t)t]);
        MT[(size_t)t * (m + 1) + m] = c[basis[(size_t)t]];
    }
    auto solve = [m](std::vector<double>& T, int ld) {
        for (int col = 0; col < m; ++col) {
            int p = col;
            for (int i = col + 1; i < m; ++i)
                if (std::fabs(T[(size_t)i * ld + col]) > std::fabs(T[(size_t)p * ld + col])) p = i;
            for (int j = 0; j < ld; ++j) std::swap(T[(size_t)p * ld + j], T[(size_t)col * ld + j]);
            const double u = T[(size_t)col * ld + col];
            for (int j = 0; j < ld; ++j) T[(size_t)col * ld + j] /= u;
            for (int i = 0; i < m; ++i) {
                if (i == col) continue;
                const double l = T[(size_t)i * ld + col];
                for (int j = 0; j < ld; ++j) T[(size_t)i * ld + j] -= l * T[(size_t)col * ld + j];
            }
        }
    };
    solve(M, m + 2);
    solve(MT, m + 1);
    for (int t = 0; t < m; ++t)
        if (M[(size_t)t * (m + 2) + m] < -tol) return false;
    for (int j = 0; j < n; ++j) {
        double d = c[j];
        for (int i = 0; i < m; ++i) d -= A(i, j) * MT[(size_t)i * (m + 1) + m];
        if (d < -tol) return false;
    }
    return true;
}

TEST(Ranging_EndsBoundTheBasis) {
    int checked = 0;
    for (uint64_t seed = 0; seed < 16; ++seed) {
        const int m = 3 + (int)(seed % 6), k = 4 + (int)(seed % 9);
        MatrixXd A;
        VectorXd b, c;
        Canonical primal = min_problem(seed, m, k, &A, &b, &c);
        Solver ps(primal);
        const Solver::Result pr = ps.twoPhaseSimplex_ex();
        CHECK(pr.status == LP_OPTIMAL);
        const Solver::Ranging rg = ps.ranging(pr);
        CHECK(rg.status == LP_OPTIMAL);
        const int n = k + m;
        CHECK(basis_optimal(A, b, c, pr.basis, 1e-9));
        for (int i = 0; i < m; ++i) {
            CHECK(rg.b_lo[i] <= b[i] + 1e-12 && b[i] <= rg.b_hi[i] + 1e-12);
            for (int side = 0; side < 2; ++side) {
                const double end = side ? rg.b_hi[i] : rg.b_lo[i];
                if (!std::isfinite(end)) continue;
                VectorXd bi = b;
                bi[i] = end + (side ? -1e-6 : 1e-6) * (1 + std::fabs(end - b[i]));   // just inside
                CHECK(basis_optimal(A, bi, c, pr.basis, 1e-9));
                const int leave = side ? rg.b_leave_hi[(size_t)i] : rg.b_leave_lo[(size_t)i];
                CHECK(leave >= 0 && leave < n);
            }
        }
        for (int j = 0; j < n; ++j) {
            CHECK(rg.c_lo[j] <= c[j] + 1e-12 && c[j] <= rg.c_hi[j] + 1e-12);
            for (int side = 0; side < 2; ++side) {
                const double end = side ? rg.c_hi[j] : rg.c_lo[j];
                if (!std::isfinite(end)) continue;
                VectorXd ci = c;
                ci[j] = end + (side ? -1e-6 : 1e-6) * (1 + std::fabs(end - c[j]));
                CHECK(basis_optimal(A, b, ci, pr.basis, 1e-9));
            }
        }
        ++checked;
    }
    CHECK(checked == 16);
}

typedef int (*RefRanging)(const double*, int, int, const double*, const double*, const int*, int, double, double*,
                          int*, double*, int*);

static bool same_bits(double a, double b) {
    if (std::isnan(a) || std::isnan(b)) return std::isnan(a) && std::isnan(b);
    uint64_t x, y;
    std::memcpy(&x, &a, 8);
    std::memcpy(&y, &b, 8);
    return x == y;
}

TEST(Ranging_MatchesTheRef) {
    const char* path = std::getenv("LP_RANGING_REF");
    CHECK(path != nullptr);
    if (!path) return;
    void* h = dlopen(path, RTLD_NOW | RTLD_LOCAL);
    CHECK(h != nullptr);
    if (!h) return;
    RefRanging ref = reinterpret_cast<RefRanging>(dlsym(h, "ref_ranging"));
    CHECK(ref != nullptr);
    for (uint64_t seed = 0; ref && seed < 24; ++seed) {
        const int m = 3 + (int)(seed % 9), k = 4 + (int)(seed % 13), n = k + m;
        MatrixXd A;
        VectorXd b, c;
        Canonical primal = min_problem(100 + seed, m, k, &A, &b, &c);
        Solver ps(primal);
        const Solver::Result pr = ps.twoPhaseSimplex_ex();
        CHECK(pr.status == LP_OPTIMAL);
        const Solver::Ranging g = ps.ranging(pr);
        std::vector<double> rhs(2 * (size_t)m), cost(2 * (size_t)n);
        std::vector<int> rv(2 * (size_t)m), cv(2 * (size_t)n);
        const int st = ref(A.data(), m, n, b.data(), c.data(), pr.basis.data(), /*maximize=*/0, Solver::EPS,
                           rhs.data(), rv.data(), cost.data(), cv.data());
        CHECK(st == g.status && st == LP_OPTIMAL);
        for (int i = 0; i < m; ++i) {
            CHECK(same_bits(g.b_lo[i], rhs[2 * (size_t)i]) && same_bits(g.b_hi[i], rhs[2 * (size_t)i + 1]));
            CHECK(g.b_leave_lo[(size_t)i] == rv[2 * (size_t)i] && g.b_leave_hi[(size_t)i] == rv[2 * (size_t)i + 1]);
        }
        for (int j = 0; j < n; ++j) {
            CHECK(same_bits(g.c_lo[j], cost[2 * (size_t)j]) && same_bits(g.c_hi[j], cost[2 * (size_t)j + 1]));
            CHECK(g.c_enter_lo[(size_t)j] == cv[2 * (size_t)j] && g.c_enter_hi[(size_t)j] == cv[2 * (size_t)j + 1]);
        }
    }
    dlclose(h);
}

TEST(Ranging_NotOptimalIsNaN) {
    MatrixXd A;
    VectorXd b, c;
    Canonical primal = min_problem(3, 4, 5, &A, &b, &c);
    Solver s(primal);
    Solver::Result r = s.twoPhaseSimplex_ex();
    r.status = LP_UNBOUNDED;
    const Solver::Ranging g = s.ranging(r);
    CHECK(g.status == LP_UNBOUNDED && std::isnan(g.b_lo[0]) && std::isnan(g.c_hi[0]) && g.c_enter_lo[0] == -1);
    r.status = LP_OPTIMAL;
    r.basis[1] = r.basis[0];   // repeated index: singular
    const Solver::Ranging e = s.ranging(r);
    CHECK(e.status == LP_SINGULAR && std::isnan(e.b_hi[0]) && e.b_leave_lo[0] == -1);
    r.basis[1] = 1000;         // out of range
    CHECK_THROWS(s.ranging(r), std::invalid_argument);
}

int main(int argc, char** argv) { return run_all(argc > 1 ? argv[1] : nullptr); }
