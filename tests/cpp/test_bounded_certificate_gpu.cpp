// GPU tests of Solver::boundedCertificate: after an infeasible or unbounded Solver::boundedSimplex and after a
// Solver::boundedResolve that a tightened bound drives to LP_INFEASIBLE it equals
// tests/ref/bounded_certificate_ref.c's bit for bit (the library named by LP_BOUNDED_CERTIFICATE_REF, loaded at run
// time); a result that is optimal keeps its status with NONE, a repeated basis index is singular, crossed bounds are
// infeasible without a vector, and a bad flag, index, eps or size throws std::invalid_argument.
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

enum Kind { FEASIBLE, INFEASIBLE, UNBOUNDED };

// fixtures.h's boxed problem with A0 >= 0.05, changed after it is drawn.  INFEASIBLE: column 1 fixed far above what the
// rows allow.  UNBOUNDED: column 0 (in [0, inf)) negated with an improving cost and every slack in [0, inf), so the
// ray moves column 0 and the basic variables with it.
static Canonical boxed_problem(uint64_t seed, int m, int k, bool maximize, Kind kind, MatrixXd* A, VectorXd* b,
                               VectorXd* c, std::vector<double>* lo, std::vector<double>* hi) {
    ::boxed_problem(seed, m, k, maximize, A, b, c, lo, hi, /*a_offset=*/0.05);
    if (kind == INFEASIBLE) (*lo)[1] = (*hi)[1] = 1000.0;
    if (kind == UNBOUNDED) {
        for (int i = 0; i < m; ++i) (*A)(i, 0) = -(*A)(i, 0);
        (*c)[0] = maximize ? 1.0 : -1.0;
    }
    return last_columns_basic(*A, *b, *c, maximize);
}

typedef int (*RefBoundedCertificate)(const double*, int, int, const double*, const double*, const double*,
                                     const double*, const int*, const int*, int, double, int*, double*, double*,
                                     double*, int*);

// the mirror's certificate for `from` against the reference at the same basis and flags; returns the kind
static int compare(RefBoundedCertificate ref, const Solver& s, const MatrixXd& A, const VectorXd& b, const VectorXd& c,
                   const std::vector<double>& lo, const std::vector<double>& hi, const Solver::BoundedResult& from,
                   bool maximize, int* index_out) {
    const int m = (int)A.rows(), n = (int)A.cols();
    const Solver::Certificate g = s.boundedCertificate(lo, hi, from);
    std::vector<double> farkas((size_t)m), ray((size_t)n);
    double value = 0.0;
    int kind = -1, index = -2;
    const int st = ref(A.data(), m, n, b.data(), c.data(), lo.data(), hi.data(), from.basis.data(),
                       from.atUpper.data(), maximize ? 1 : 0, Solver::EPS, &kind, farkas.data(), ray.data(), &value,
                       &index);
    CHECK(st == LP_OPTIMAL && g.status == from.status);
    CHECK(g.kind == kind && g.index == index && same_bits(g.value, value));
    for (int i = 0; i < m; ++i) CHECK(same_bits(g.farkas[i], farkas[(size_t)i]));
    for (int j = 0; j < n; ++j) CHECK(same_bits(g.ray[j], ray[(size_t)j]));
    *index_out = g.index;
    return g.kind;
}

TEST(BoundedCertificate_MatchesTheRef) {
    const RefLib lib("LP_BOUNDED_CERTIFICATE_REF");
    RefBoundedCertificate ref = lib.symbol<RefBoundedCertificate>("ref_bounded_certificate");
    int phase1 = 0, rays = 0, dual = 0;
    for (uint64_t seed = 0; ref && seed < 12; ++seed) {
        const int m = 3 + (int)(seed % 5), k = 5 + (int)(seed % 7);
        const bool maximize = seed % 2 == 0;
        MatrixXd A;
        VectorXd b, c;
        std::vector<double> lo, hi;
        int index = -2;
        {   // phase I of the cold solve
            Canonical p = boxed_problem(seed, m, k, maximize, INFEASIBLE, &A, &b, &c, &lo, &hi);
            Solver s(p);
            const Solver::BoundedResult r = s.boundedSimplex(lo, hi, /*throw_on_failure=*/false);
            CHECK(r.status == LP_INFEASIBLE);
            if (r.status == LP_INFEASIBLE && compare(ref, s, A, b, c, lo, hi, r, maximize, &index) == LP_CERT_FARKAS &&
                index == -1)
                ++phase1;
        }
        {   // phase II of the cold solve
            Canonical p = boxed_problem(seed, m, k, maximize, UNBOUNDED, &A, &b, &c, &lo, &hi);
            Solver s(p);
            const Solver::BoundedResult r = s.boundedSimplex(lo, hi, /*throw_on_failure=*/false);
            CHECK(r.status == LP_UNBOUNDED);
            if (r.status == LP_UNBOUNDED && compare(ref, s, A, b, c, lo, hi, r, maximize, &index) == LP_CERT_RAY) ++rays;
        }
        {   // the dual simplex of a re-solve: column 0 pushed far above what the rows allow
            Canonical p = boxed_problem(seed, m, k, maximize, FEASIBLE, &A, &b, &c, &lo, &hi);
            Solver s(p);
            const Solver::BoundedResult cold = s.boundedSimplex(lo, hi, /*throw_on_failure=*/false);
            if (cold.status != LP_OPTIMAL) continue;
            lo[0] = 1000.0;
            const Solver::BoundedResult r = s.boundedResolve(lo, hi, cold, /*throw_on_failure=*/false);
            CHECK(r.status == LP_INFEASIBLE);
            if (r.status == LP_INFEASIBLE && compare(ref, s, A, b, c, lo, hi, r, maximize, &index) == LP_CERT_FARKAS &&
                index >= 0)
                ++dual;
        }
    }
    CHECK(phase1 == 12 && rays == 12 && dual >= 8);
}

TEST(BoundedCertificate_StatusesAndExceptions) {
    MatrixXd A;
    VectorXd b, c;
    std::vector<double> lo, hi;
    Canonical p = boxed_problem(2, 4, 7, true, INFEASIBLE, &A, &b, &c, &lo, &hi);
    const int n = 11;
    Solver s(p);
    Solver::BoundedResult r = s.boundedSimplex(lo, hi, /*throw_on_failure=*/false);
    CHECK(r.status == LP_INFEASIBLE);
    const Solver::Certificate g = s.boundedCertificate(lo, hi, r);
    CHECK(g.status == LP_INFEASIBLE && g.kind == LP_CERT_FARKAS && g.value < 0 && std::isnan(g.ray[0]));
    CHECK(s.boundedCertificate(lo, hi, r, 1e6).kind == LP_CERT_NONE);   // nothing passes an eps this large
    Solver::BoundedResult opt = r;
    opt.status = LP_OPTIMAL;   // a result that did not fail keeps its status and gets NONE
    const Solver::Certificate none = s.boundedCertificate(lo, hi, opt);
    CHECK(none.status == LP_OPTIMAL && none.kind == LP_CERT_NONE && std::isnan(none.farkas[0]) &&
          std::isnan(none.value) && none.index == -1);
    Solver::BoundedResult rep = r;
    rep.basis[1] = rep.basis[0];   // repeated index: singular
    const Solver::Certificate e = s.boundedCertificate(lo, hi, rep);
    CHECK(e.status == LP_SINGULAR && e.kind == LP_CERT_NONE && std::isnan(e.farkas[0]) && e.index == -1);
    std::vector<double> crossed = hi;
    crossed[3] = lo[3] - 1.0;      // crossed bounds: infeasible without a vector, nothing thrown
    const Solver::Certificate x = s.boundedCertificate(lo, crossed, r);
    CHECK(x.status == LP_INFEASIBLE && x.kind == LP_CERT_NONE && std::isnan(x.value));
    Solver::BoundedResult bad = r;
    bad.basis[1] = 1000;           // out of range
    CHECK_THROWS(s.boundedCertificate(lo, hi, bad), std::invalid_argument);
    bad = r;
    bad.atUpper[0] = 1;            // column 0 has no upper bound
    CHECK(hi[0] == INF);
    CHECK_THROWS(s.boundedCertificate(lo, hi, bad), std::invalid_argument);
    CHECK_THROWS(s.boundedCertificate(lo, hi, r, -1.0), std::invalid_argument);
    std::vector<double> few(lo.begin(), lo.begin() + n - 1);
    CHECK_THROWS(s.boundedCertificate(few, hi, r), std::invalid_argument);
    bad = r;
    bad.basis.pop_back();
    CHECK_THROWS(s.boundedCertificate(lo, hi, bad), std::invalid_argument);
}

int main(int argc, char** argv) { return run_all(argc > 1 ? argv[1] : nullptr); }
