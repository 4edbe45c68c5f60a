// GPU tests of Solver::boundedCertificateLarge: after an infeasible or unbounded Solver::boundedSimplexLarge and after a
// Solver::boundedResolveLarge that a raised bound drives to LP_INFEASIBLE, on 160 x 320 boxed LPs (beyond
// lp_basis_bounded_certificate_fits), the certificate satisfies its own inequalities and equals
// tests/ref/bounded_certificate_ref.c's bit for bit (the library named by LP_BOUNDED_CERTIFICATE_REF, loaded at run
// time); the LDS method still refuses the shape; a result that is optimal keeps its status with NONE, a repeated basis
// index is singular, crossed bounds are infeasible without a vector, and a bad flag, index or eps throws
// std::invalid_argument.  (No test_ prefix: tests/test_bounded_certificate_large_cpp.py runs this program.)
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>

#include "check.h"
#include "fixtures.h"
#include "Canonical.h"
#include "SimplexSolover.h"

using lpla::MatrixXd;
using lpla::VectorXd;

static const double INF = std::numeric_limits<double>::infinity();
static const int M = 160, K = 160, N = M + K;

enum Kind { FEASIBLE, INFEASIBLE, UNBOUNDED };

// tests/cpp/test_bounded_certificate_gpu.cpp's problems at 160 x 320 (b_i in 0.125 k [1, 2), A0 >= 0.05).  INFEASIBLE:
// column 1 fixed far above what the rows allow.  UNBOUNDED: column 0 (in [0, inf)) negated with an improving cost and
// every slack in [0, inf), so the ray moves column 0 and the basic variables with it.
static Canonical large_problem(uint64_t seed, bool maximize, Kind kind, MatrixXd* A, VectorXd* b, VectorXd* c,
                               std::vector<double>* lo, std::vector<double>* hi) {
    boxed_problem(seed, M, K, maximize, A, b, c, lo, hi, /*a_offset=*/0.05, /*b_scale=*/0.125);
    if (kind == INFEASIBLE) (*lo)[1] = (*hi)[1] = 1000.0;
    if (kind == UNBOUNDED) {
        for (int i = 0; i < M; ++i) (*A)(i, 0) = -(*A)(i, 0);
        (*c)[0] = maximize ? 1.0 : -1.0;
    }
    return last_columns_basic(*A, *b, *c, maximize);
}

typedef int (*RefBoundedCertificate)(const double*, int, int, const double*, const double*, const double*,
                                     const double*, const int*, const int*, int, double, int*, double*, double*,
                                     double*, int*);

// FARKAS: with g = A^T f, f.b lies below the minimum of g.x over the box; RAY: A r = 0, r >= 0, r = 0 under a finite
// upper bound, c.r = value of the improving sign
static void check_inequalities(const Solver::Certificate& g, const MatrixXd& A, const VectorXd& b, const VectorXd& c,
                               const std::vector<double>& lo, const std::vector<double>& hi, bool maximize) {
    if (g.kind == LP_CERT_FARKAS) {
        double fb = 0.0, least = 0.0;
        for (int i = 0; i < M; ++i) fb += g.farkas[i] * b[i];
        for (int j = 0; j < N; ++j) {
            double gj = 0.0;
            for (int i = 0; i < M; ++i) gj += g.farkas[i] * A(i, j);
            if (hi[(size_t)j] == INF) {
                CHECK(gj >= -1e-7);
                least += gj * lo[(size_t)j];
            } else {
                least += std::min(gj * lo[(size_t)j], gj * hi[(size_t)j]);
            }
        }
        CHECK(fb < least - 1e-7);
        CHECK(g.value < 0 && least - fb >= std::fabs(g.value) * (1.0 - 1e-6) - 1e-7);
        CHECK(std::isnan(g.ray[0]) && std::isnan(g.ray[N - 1]));
    } else if (g.kind == LP_CERT_RAY) {
        double cr = 0.0;
        for (int j = 0; j < N; ++j) {
            CHECK(g.ray[j] >= -1e-8 && (hi[(size_t)j] == INF || g.ray[j] <= 1e-8));
            cr += c[j] * g.ray[j];
        }
        for (int i = 0; i < M; ++i) {
            double ar = 0.0;
            for (int j = 0; j < N; ++j) ar += A(i, j) * g.ray[j];
            CHECK(std::fabs(ar) < 1e-8);
        }
        CHECK(maximize ? cr > 0 : cr < 0);
        CHECK(std::fabs(cr - g.value) <= 1e-8 && g.ray[g.index] == 1.0);
        CHECK(std::isnan(g.farkas[0]) && std::isnan(g.farkas[M - 1]));
    }
}

// the certificate of `from` against its inequalities and the reference at the same basis and flags; returns the kind
static int compare(RefBoundedCertificate ref, const Solver& s, const MatrixXd& A, const VectorXd& b, const VectorXd& c,
                   const std::vector<double>& lo, const std::vector<double>& hi, const Solver::BoundedResult& from,
                   bool maximize, int* index_out) {
    const Solver::Certificate g = s.boundedCertificateLarge(lo, hi, from);
    check_inequalities(g, A, b, c, lo, hi, maximize);
    std::vector<double> farkas((size_t)M), ray((size_t)N);
    double value = 0.0;
    int kind = -1, index = -2;
    const int st = ref(A.data(), M, N, b.data(), c.data(), lo.data(), hi.data(), from.basis.data(),
                       from.atUpper.data(), maximize ? 1 : 0, Solver::EPS, &kind, farkas.data(), ray.data(), &value,
                       &index);
    CHECK(st == LP_OPTIMAL && g.status == from.status);
    CHECK(g.kind == kind && g.index == index && same_bits(g.value, value));
    for (int i = 0; i < M; ++i) CHECK(same_bits(g.farkas[i], farkas[(size_t)i]));
    for (int j = 0; j < N; ++j) CHECK(same_bits(g.ray[j], ray[(size_t)j]));
    CHECK_THROWS(s.boundedCertificate(lo, hi, from), std::invalid_argument);   // the LDS method refuses this shape
    *index_out = g.index;
    return g.kind;
}

TEST(BoundedCertificateLarge_MatchesTheRefAndItsInequalities) {
    const RefLib lib("LP_BOUNDED_CERTIFICATE_REF");
    RefBoundedCertificate ref = lib.symbol<RefBoundedCertificate>("ref_bounded_certificate");
    CHECK(lp_basis_bounded_certificate_fits(M, N) == 0);
    int phase1 = 0, rays = 0, dual = 0;
    for (uint64_t seed = 1; ref && seed <= 2; ++seed) {
        const bool maximize = seed % 2 == 0;
        MatrixXd A;
        VectorXd b, c;
        std::vector<double> lo, hi;
        int index = -2;
        {   // phase I of the cold solve
            Solver s(large_problem(seed, maximize, INFEASIBLE, &A, &b, &c, &lo, &hi));
            const Solver::BoundedResult r = s.boundedSimplexLarge(lo, hi, /*throw_on_failure=*/false);
            CHECK(r.status == LP_INFEASIBLE);
            if (r.status == LP_INFEASIBLE && compare(ref, s, A, b, c, lo, hi, r, maximize, &index) == LP_CERT_FARKAS &&
                index == -1)
                ++phase1;
        }
        {   // phase II of the cold solve
            Solver s(large_problem(seed, maximize, UNBOUNDED, &A, &b, &c, &lo, &hi));
            const Solver::BoundedResult r = s.boundedSimplexLarge(lo, hi, /*throw_on_failure=*/false);
            CHECK(r.status == LP_UNBOUNDED);
            if (r.status == LP_UNBOUNDED && compare(ref, s, A, b, c, lo, hi, r, maximize, &index) == LP_CERT_RAY) ++rays;
        }
        {   // the dual simplex of a re-solve: column 0 pushed far above what the rows allow
            Solver s(large_problem(seed, maximize, FEASIBLE, &A, &b, &c, &lo, &hi));
            const Solver::BoundedResult cold = s.boundedSimplexLarge(lo, hi, /*throw_on_failure=*/false);
            CHECK(cold.status == LP_OPTIMAL);
            if (cold.status != LP_OPTIMAL) continue;
            lo[0] = 1000.0;
            const Solver::BoundedResult r = s.boundedResolveLarge(lo, hi, cold, /*throw_on_failure=*/false);
            CHECK(r.status == LP_INFEASIBLE);
            if (r.status == LP_INFEASIBLE && compare(ref, s, A, b, c, lo, hi, r, maximize, &index) == LP_CERT_FARKAS &&
                index >= 0)
                ++dual;
        }
    }
    std::printf("  %d phase-I, %d ray, %d dual-simplex certificates\n", phase1, rays, dual);
    CHECK(phase1 == 2 && rays == 2 && dual == 2);
}

TEST(BoundedCertificateLarge_StatusesAndExceptions) {
    MatrixXd A;
    VectorXd b, c;
    std::vector<double> lo, hi;
    Solver s(large_problem(2, true, INFEASIBLE, &A, &b, &c, &lo, &hi));
    Solver::BoundedResult r = s.boundedSimplexLarge(lo, hi, /*throw_on_failure=*/false);
    CHECK(r.status == LP_INFEASIBLE);
    const Solver::Certificate g = s.boundedCertificateLarge(lo, hi, r);
    CHECK(g.status == LP_INFEASIBLE && g.kind == LP_CERT_FARKAS && g.value < 0 && std::isnan(g.ray[0]));
    CHECK(s.boundedCertificateLarge(lo, hi, r, 1e6).kind == LP_CERT_NONE);   // nothing passes an eps this large
    Solver::BoundedResult opt = r;
    opt.status = LP_OPTIMAL;   // a result that did not fail keeps its status and gets NONE
    const Solver::Certificate none = s.boundedCertificateLarge(lo, hi, opt);
    CHECK(none.status == LP_OPTIMAL && none.kind == LP_CERT_NONE && std::isnan(none.farkas[0]) &&
          std::isnan(none.value) && none.index == -1);
    Solver::BoundedResult rep = r;
    rep.basis[1] = rep.basis[0];   // repeated index: singular
    const Solver::Certificate e = s.boundedCertificateLarge(lo, hi, rep);
    CHECK(e.status == LP_SINGULAR && e.kind == LP_CERT_NONE && std::isnan(e.farkas[0]) && e.index == -1);
    std::vector<double> crossed = hi;
    crossed[3] = lo[3] - 1.0;      // crossed bounds: infeasible without a vector, nothing thrown, also with the repeat
    const Solver::Certificate x = s.boundedCertificateLarge(lo, crossed, r);
    CHECK(x.status == LP_INFEASIBLE && x.kind == LP_CERT_NONE && std::isnan(x.value));
    CHECK(s.boundedCertificateLarge(lo, crossed, rep).status == LP_INFEASIBLE);
    Solver::BoundedResult bad = r;
    bad.basis[1] = N + M;          // out of range (N + M - 1 is the last artificial)
    CHECK_THROWS(s.boundedCertificateLarge(lo, hi, bad), std::invalid_argument);
    bad = r;
    bad.atUpper[0] = 1;            // column 0 has no upper bound
    CHECK(hi[0] == INF);
    CHECK_THROWS(s.boundedCertificateLarge(lo, hi, bad), std::invalid_argument);
    CHECK_THROWS(s.boundedCertificateLarge(lo, hi, r, -1.0), std::invalid_argument);
    // and a good call afterwards
    const Solver::Certificate again = s.boundedCertificateLarge(lo, hi, r);
    CHECK(again.kind == LP_CERT_FARKAS && same_bits(again.value, g.value));
}

int main(int argc, char** argv) { return run_all(argc > 1 ? argv[1] : nullptr); }
