// GPU tests of Solver::certificate: after twoPhaseSimplex_ex(false) on MIN canonical problems that are infeasible
// (phase-I bases with artificials) or unbounded in phase II, the certificate at the final basis equals
// tests/ref/certificate_ref.c's bit for bit (the library named by LP_CERTIFICATE_REF, loaded at run time), and its
// vectors prove the verdict.
#include <cmath>
#include <cstdint>

#include "check.h"
#include "fixtures.h"
#include "Canonical.h"
#include "SimplexSolover.h"

using lpla::MatrixXd;
using lpla::VectorXd;

// min c.x over [A0 | -I] x = b, x >= 0 (k originals, m surplus columns), c > 0 on the originals.  kind 0: feasible;
// kind 1: row r made non-negative (its surplus a slack) with b_r < 0: infeasible; kind 2: columns 0 and 1 ride the
// ray x0 = 2t, x1 = t (rows 0 and 1 only) with negative costs, rows 0 and 1 slack rows: unbounded in phase II.
static Canonical problem(uint64_t seed, int m, int k, int kind, MatrixXd* Aout, VectorXd* bout, VectorXd* cout) {
    uint64_t s = seed * 7919 + 17;
    MatrixXd A = MatrixXd::Zero(m, k + m);
    VectorXd b(m), c = VectorXd::Zero(k + m);
    for (int i = 0; i < m; ++i) {
        for (int j = 0; j < k; ++j) A(i, j) = u01(s);
        A(i, k + i) = -1.0;
        b[i] = 1.0 + u01(s);
    }
    for (int j = 0; j < k; ++j) c[j] = 0.1 + u01(s);
    if (kind == 1) {
        const int r = (int)(seed % (uint64_t)m);
        for (int j = 0; j < k; ++j) A(r, j) = 0.1 + u01(s);
        A(r, k + r) = 1.0;
        b[r] = -1.0 - u01(s);
    } else if (kind == 2) {
        for (int i = 0; i < m; ++i) A(i, 0) = A(i, 1) = 0.0;
        A(0, 0) = -1.0, A(0, 1) = 1.0, A(0, k) = 1.0;
        A(1, 0) = 1.0, A(1, 1) = -2.0, A(1, k + 1) = 1.0;
        c[0] = c[1] = -1.5;
    }
    std::vector<int> basis((size_t)m);
    for (int i = 0; i < m; ++i) basis[(size_t)i] = k + i;   // (ignored by the two-phase flow)
    *Aout = A;
    *bout = b;
    *cout = c;
    Canonical can(A, b, c, basis, /*minimize=*/true);
    can.SetOriginalVariablesCount(k + m);
    return can;
}

typedef int (*RefCertificate)(const double*, int, int, const double*, const double*, const int*, int, double, int*,
                              double*, double*, double*, int*);

TEST(Certificate_MatchesTheRefAndProves) {
    const RefLib lib("LP_CERTIFICATE_REF");
    RefCertificate ref = lib.symbol<RefCertificate>("ref_certificate");
    int seen[3] = {0, 0, 0};
    for (uint64_t seed = 0; ref && seed < 24; ++seed) {
        const int m = 3 + (int)(seed % 9), k = 4 + (int)(seed % 13), n = k + m, kind = (int)(seed % 3);
        MatrixXd A;
        VectorXd b, c;
        Solver ps(problem(200 + seed, m, k, kind, &A, &b, &c));
        const Solver::Result pr = ps.twoPhaseSimplex_ex(false);
        CHECK(pr.status == (kind == 0 ? LP_OPTIMAL : kind == 1 ? LP_INFEASIBLE : LP_UNBOUNDED));
        const Solver::Certificate g = ps.certificate(pr);
        CHECK(g.status == pr.status);
        if (kind == 0) {   // an optimal result keeps its status and gets NONE
            CHECK(g.kind == LP_CERT_NONE && g.index == -1 && std::isnan(g.value));
            ++seen[0];
            continue;
        }
        bool artificial = false;
        for (int t = 0; t < m; ++t) artificial = artificial || pr.basis[(size_t)t] >= n;
        CHECK(artificial == (kind == 1));   // the phase-I basis, passed as it is
        int rk = -1, ri = -2;
        double rv = 0.0;
        std::vector<double> f((size_t)m), r((size_t)n);
        const int st = ref(A.data(), m, n, b.data(), c.data(), pr.basis.data(), /*maximize=*/0, Solver::EPS, &rk,
                           f.data(), r.data(), &rv, &ri);
        CHECK(st == LP_OPTIMAL && rk == g.kind && ri == g.index && same_bits(rv, g.value));
        for (int i = 0; i < m; ++i) CHECK(same_bits(f[(size_t)i], g.farkas[i]));
        for (int j = 0; j < n; ++j) CHECK(same_bits(r[(size_t)j], g.ray[j]));
        if (kind == 1) {
            CHECK(g.kind == LP_CERT_FARKAS);
            double bf = 0.0;
            for (int i = 0; i < m; ++i) bf += b[i] * g.farkas[i];
            CHECK(bf < 0.0);
            for (int j = 0; j < n; ++j) {
                double s = 0.0;
                for (int i = 0; i < m; ++i) s += A(i, j) * g.farkas[i];
                CHECK(s >= -1e-7);
            }
        } else {
            CHECK(g.kind == LP_CERT_RAY);
            double cr = 0.0;
            for (int j = 0; j < n; ++j) {
                CHECK(g.ray[j] >= -1e-7);
                cr += c[j] * g.ray[j];
            }
            CHECK(cr < 0.0);
            for (int i = 0; i < m; ++i) {
                double s = 0.0;
                for (int j = 0; j < n; ++j) s += A(i, j) * g.ray[j];
                CHECK(std::fabs(s) <= 1e-7);
            }
        }
        ++seen[kind];
    }
    CHECK(seen[0] == 8 && seen[1] == 8 && seen[2] == 8);
}

int main(int argc, char** argv) { return run_all(argc > 1 ? argv[1] : nullptr); }
