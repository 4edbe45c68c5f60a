// GPU tests of Solver::ranging: after twoPhaseSimplex_ex() on MIN canonical problems the ranges at the final basis
// equal tests/ref/ranging_ref.c's bit for bit (the library named by LP_RANGING_REF, loaded at run time), and the
// basis stays optimal with b_i or c_j moved just inside either finite end.
#include <cmath>
#include <cstdint>

#include "check.h"
#include "fixtures.h"
#include "Canonical.h"
#include "SimplexSolover.h"

using lpla::MatrixXd;
using lpla::VectorXd;

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

TEST(Ranging_MatchesTheRef) {
    const RefLib lib("LP_RANGING_REF");
    RefRanging ref = lib.symbol<RefRanging>("ref_ranging");
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
