// Solver::boundedDualsLarge and Solver::boundedRangingLarge before they reach the device: wrong-sized bounds and results
// throw std::invalid_argument with the method's own name, the bounds are checked before the result, and a result that
// is not optimal keeps its status with NaN and -1 without a device.  Needs no GPU.  (No test_ prefix:
// tests/test_bounded_sens_large_cpp.py runs this program.)
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

TEST(BoundedSensLarge_SizeChecks) {
    const Solver s(problem());
    const std::vector<double> lo(SN, 0.0), hi(SN, 9.0), few(SN - 1, 0.0);
    Solver::BoundedResult from, shortBasis, shortFlags;
    from.basis = shortFlags.basis = {3, 4, 5};
    shortBasis.basis = {3, 4};
    from.atUpper = shortBasis.atUpper = {0, 1, 0, 0, 0, 0};
    shortFlags.atUpper = {0, 1, 0, 0, 0};
    from.status = shortBasis.status = shortFlags.status = LP_OPTIMAL;
    CHECK_WHAT(s.boundedDualsLarge(few, hi, from), "Solver::boundedDualsLarge: lo / hi size != cols(A)");
    CHECK_WHAT(s.boundedDualsLarge(lo, few, from), "Solver::boundedDualsLarge: lo / hi size != cols(A)");
    CHECK_WHAT(s.boundedDualsLarge(lo, hi, shortBasis),
               "Solver::boundedDualsLarge: the result's basis / atUpper size != rows(A) / cols(A)");
    CHECK_WHAT(s.boundedDualsLarge(lo, hi, shortFlags),
               "Solver::boundedDualsLarge: the result's basis / atUpper size != rows(A) / cols(A)");
    CHECK_WHAT(s.boundedDualsLarge(few, hi, shortBasis), "Solver::boundedDualsLarge: lo / hi size != cols(A)");
    CHECK_WHAT(s.boundedRangingLarge(few, hi, from), "Solver::boundedRangingLarge: lo / hi size != cols(A)");
    CHECK_WHAT(s.boundedRangingLarge(lo, few, from), "Solver::boundedRangingLarge: lo / hi size != cols(A)");
    CHECK_WHAT(s.boundedRangingLarge(lo, hi, shortBasis),
               "Solver::boundedRangingLarge: the result's basis / atUpper size != rows(A) / cols(A)");
    CHECK_WHAT(s.boundedRangingLarge(lo, hi, shortFlags),
               "Solver::boundedRangingLarge: the result's basis / atUpper size != rows(A) / cols(A)");
    CHECK_WHAT(s.boundedRangingLarge(few, hi, shortBasis), "Solver::boundedRangingLarge: lo / hi size != cols(A)");
    // the LDS methods keep their own names
    CHECK_WHAT(s.boundedDuals(few, hi, from), "Solver::boundedDuals: lo / hi size != cols(A)");
    CHECK_WHAT(s.boundedRanging(lo, hi, shortBasis),
               "Solver::boundedRanging: the result's basis / atUpper size != rows(A) / cols(A)");
}

TEST(BoundedSensLarge_AResultThatIsNotOptimalKeepsItsStatus) {
    const Solver s(problem());
    const std::vector<double> lo(SN, 0.0), hi(SN, 9.0);
    Solver::BoundedResult from;   // sizes not looked at: nothing is analysed
    from.status = LP_UNBOUNDED;
    const Solver::BoundedDuals g = s.boundedDualsLarge(lo, hi, from);
    CHECK(g.status == LP_UNBOUNDED && g.x.size() == SN && g.y.size() == SM && std::isnan(g.x[0]) && std::isnan(g.y[SM - 1]));
    CHECK(std::isnan(g.d[SN - 1]) && std::isnan(g.objective));
    const Solver::BoundedRanging q = s.boundedRangingLarge(lo, hi, from);
    CHECK(q.status == LP_UNBOUNDED && std::isnan(q.b_lo[0]) && std::isnan(q.c_hi[SN - 1]));
    CHECK(q.b_leave_lo[0] == -1 && q.b_side_hi[SM - 1] == -1 && q.c_enter_hi[SN - 1] == -1);
}

int main(int argc, char** argv) { return run_all(argc > 1 ? argv[1] : nullptr); }
