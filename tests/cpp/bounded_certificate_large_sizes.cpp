// Solver::boundedCertificateLarge before it reaches the device: wrong-sized bounds and results throw
// std::invalid_argument with the method's own name, the bounds are checked before the result, and a result that is
// neither infeasible nor unbounded keeps its status with NONE, NaN and -1 without a device.  Needs no GPU.  (No test_
// prefix: tests/test_bounded_certificate_large_cpp.py runs this program.)
#include <cmath>
#include <stdexcept>
#include <string>

#include "check.h"
#include "Canonical.h"
#include "SimplexSolover.h"

using lpla::MatrixXd;
using lpla::VectorXd;

#define CHECK_WHAT(expr, text) do { std::string w_ = "(nothing thrown)"; \
    try { expr; } catch (const std::invalid_argument& e) { w_ = e.what(); } \
    catch (const std::exception& e) { w_ = std::string("(not std::invalid_argument) ") + e.what(); } \
    if (w_ != (text)) throw std::runtime_error(std::string(__FILE__) + ":" + std::to_string(__LINE__) + ": " #expr \
                                               " threw \"" + w_ + "\""); } while (0)

static const int SM = 3, SN = 6;

static Canonical problem() {
    MatrixXd A = MatrixXd::Zero(SM, SN);
    VectorXd b(SM), c = VectorXd::Zero(SN);
    for (int i = 0; i < SM; ++i) {
        for (int j = 0; j < SN - SM; ++j) A(i, j) = 1.0 + i + j;
        A(i, SN - SM + i) = 1.0;
        b[i] = 4.0 + i;
    }
    for (int j = 0; j < SN - SM; ++j) c[j] = 1.0;
    Canonical can(A, b, c, std::vector<int>{3, 4, 5}, /*minimize=*/false);
    can.SetOriginalVariablesCount(SN - SM);
    return can;
}

TEST(BoundedCertificateLarge_SizeChecks) {
    const Solver s(problem());
    const std::vector<double> lo(SN, 0.0), hi(SN, 9.0), few(SN - 1, 0.0);
    Solver::BoundedResult from, shortBasis, shortFlags;
    from.basis = shortFlags.basis = {3, 4, 5};
    shortBasis.basis = {3, 4};
    from.atUpper = shortBasis.atUpper = {0, 1, 0, 0, 0, 0};
    shortFlags.atUpper = {0, 1, 0, 0, 0};
    for (int status : {LP_INFEASIBLE, LP_UNBOUNDED}) {
        from.status = shortBasis.status = shortFlags.status = status;
        CHECK_WHAT(s.boundedCertificateLarge(few, hi, from), "Solver::boundedCertificateLarge: lo / hi size != cols(A)");
        CHECK_WHAT(s.boundedCertificateLarge(lo, few, from), "Solver::boundedCertificateLarge: lo / hi size != cols(A)");
        CHECK_WHAT(s.boundedCertificateLarge(lo, hi, shortBasis),
                   "Solver::boundedCertificateLarge: the result's basis / atUpper size != rows(A) / cols(A)");
        CHECK_WHAT(s.boundedCertificateLarge(lo, hi, shortFlags),
                   "Solver::boundedCertificateLarge: the result's basis / atUpper size != rows(A) / cols(A)");
        CHECK_WHAT(s.boundedCertificateLarge(few, hi, shortBasis),
                   "Solver::boundedCertificateLarge: lo / hi size != cols(A)");
        // the LDS method keeps its own name
        CHECK_WHAT(s.boundedCertificate(few, hi, from), "Solver::boundedCertificate: lo / hi size != cols(A)");
        CHECK_WHAT(s.boundedCertificate(lo, hi, shortBasis),
                   "Solver::boundedCertificate: the result's basis / atUpper size != rows(A) / cols(A)");
    }
}

TEST(BoundedCertificateLarge_AResultWithoutAVerdictKeepsItsStatus) {
    const Solver s(problem());
    const std::vector<double> lo(SN, 0.0), hi(SN, 9.0), few(SN - 1, 0.0);
    Solver::BoundedResult from;   // sizes not looked at: nothing is analysed
    for (int status : {LP_OPTIMAL, LP_ITER_LIMIT, LP_SINGULAR}) {
        from.status = status;
        const Solver::Certificate g = s.boundedCertificateLarge(lo, hi, from);
        CHECK(g.status == status && g.kind == LP_CERT_NONE && g.index == -1 && std::isnan(g.value));
        CHECK(g.farkas.size() == SM && g.ray.size() == SN && std::isnan(g.farkas[SM - 1]) && std::isnan(g.ray[0]));
    }
    // the bounds' sizes are checked even then
    CHECK_WHAT(s.boundedCertificateLarge(few, hi, from), "Solver::boundedCertificateLarge: lo / hi size != cols(A)");
}

int main(int argc, char** argv) { return run_all(argc > 1 ? argv[1] : nullptr); }
