// GPU tests of Solver::boundedCertificate: after an infeasible or unbounded Solver::boundedSimplex and after a
// Solver::boundedResolve that a tightened bound drives to LP_INFEASIBLE it equals
// tests/ref/bounded_certificate_ref.c's bit for bit (the library named by LP_BOUNDED_CERTIFICATE_REF, loaded at run
// time); a result that is optimal keeps its status with NONE, a repeated basis index is singular, crossed bounds are
// infeasible without a vector, and a bad flag, index, eps or size throws std::invalid_argument.
#include <dlfcn.h>

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "check.h"
#include "Canonical.h"
#include "SimplexSolover.h"

using lpla::MatrixXd;
using lpla::VectorXd;

static const double INF = std::numeric_limits<double>::infinity();

static double u01(uint64_t& s) {   // splitmix64
    uint64_t z = (s += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    z ^= z >> 31;
    return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}

enum Kind { FEASIBLE, INFEASIBLE, UNBOUNDED };

// [A0 | I] x = b with A0 > 0, k structural columns boxed in several ways, costs of both signs.  INFEASIBLE: column 1
// fixed far above what the rows allow.  UNBOUNDED: column 0 (in [0, inf)) negated with an improving cost and every
// slack in [0, inf), so the ray moves column 0 and the basic variables with it.
static Canonical boxed_problem(uint64_t seed, int m, int k, bool maximize, Kind kind, MatrixXd* Aout, VectorXd* bout,
                               VectorXd* cout, std::vector<double>* lo, std::vector<double>* hi) {
    uint64_t s = seed * 7919 + 29;
    const int n = k + m;
    MatrixXd A = MatrixXd::Zero(m, n);
    VectorXd b(m), c = VectorXd::Zero(n);
    for (int i = 0; i < m; ++i) {
        for (int j = 0; j < k; ++j) A(i, j) = 0.05 + u01(s);
        A(i, k + i) = 1.0;
        b[i] = 0.5 * k * (1.0 + u01(s));
    }
    lo->assign((size_t)n, 0.0);
    hi->assign((size_t)n, INF);
    for (int j = 0; j < k; ++j) {
        c[j] = u01(s) - 0.3;
        switch (j % 4) {
            case 1: (*hi)[(size_t)j] = 0.2 + 2.0 * u01(s); break;
            case 2: (*lo)[(size_t)j] = (*hi)[(size_t)j] = u01(s); break;
            case 3: (*lo)[(size_t)j] = -u01(s); (*hi)[(size_t)j] = 1.0 + u01(s); break;
            default: break;
        }
    }
    if (kind == INFEASIBLE) (*lo)[1] = (*hi)[1] = 1000.0;
    if (kind == UNBOUNDED) {
        for (int i = 0; i < m; ++i) A(i, 0) = -A(i, 0);
        c[0] = maximize ? 1.0 : -1.0;
    }
    std::vector<int> basis((size_t)m);
    for (int i = 0; i < m; ++i) basis[(size_t)i] = k + i;
    *Aout = A;
    *bout = b;
    *cout = c;
    Canonical can(A, b, c, basis, /*minimize=*/!maximize);
    can.SetOriginalVariablesCount(n);
    return can;
}

typedef int (*RefBoundedCertificate)(const double*, int, int, const double*, const double*, const double*,
                                     const double*, const int*, const int*, int, double, int*, double*, double*,
                                     double*, int*);

static bool same_bits(double a, double b) {
    if (std::isnan(a) || std::isnan(b)) return std::isnan(a) && std::isnan(b);
    uint64_t x, y;
    std::memcpy(&x, &a, 8);
    std::memcpy(&y, &b, 8);
    return x == y;
}

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
    const char* path = std::getenv("LP_BOUNDED_CERTIFICATE_REF");
    CHECK(path != nullptr);
    if (!path) return;
    void* h = dlopen(path, RTLD_NOW | RTLD_LOCAL);
    CHECK(h != nullptr);
    if (!h) return;
    RefBoundedCertificate ref = reinterpret_cast<RefBoundedCertificate>(dlsym(h, "ref_bounded_certificate"));
    CHECK(ref != nullptr);
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
    dlclose(h);
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
