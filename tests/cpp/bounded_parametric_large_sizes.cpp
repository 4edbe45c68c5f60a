// Solver::boundedParametricRhsLarge and Solver::boundedParametricCostLarge before they reach the device: wrong-sized
// bounds, results and directions throw std::invalid_argument, the bounds are checked before the result, and a result
// that is not optimal keeps its status without segments and without a device.  Needs no GPU.  (No test_ prefix:
// tests/test_bounded_parametric_large_cpp.py runs this program.)
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

TEST(BoundedParametricLarge_SizeChecks) {
    const Solver s(problem());
    const std::vector<double> lo(SN, 0.0), hi(SN, 9.0), few(SN - 1, 0.0);
    const VectorXd d = VectorXd::Zero(SM), g = VectorXd::Zero(SN);
    Solver::BoundedResult from, shortBasis, shortFlags;
    from.basis = shortFlags.basis = {3, 4, 5};
    shortBasis.basis = {3, 4};
    from.atUpper = shortBasis.atUpper = {0, 1, 0, 0, 0, 0};
    shortFlags.atUpper = {0, 1, 0, 0, 0};
    from.status = shortBasis.status = shortFlags.status = LP_OPTIMAL;
    const char* bounds = "Solver::boundedParametric: lo / hi size != cols(A)";
    const char* start = "Solver::boundedParametric: the result's basis / atUpper size != rows(A) / cols(A)";
    CHECK_WHAT(s.boundedParametricRhsLarge(few, hi, from, d, 1.0), bounds);
    CHECK_WHAT(s.boundedParametricCostLarge(lo, few, from, g, 1.0), bounds);
    CHECK_WHAT(s.boundedParametricRhsLarge(lo, hi, shortBasis, d, 1.0), start);
    CHECK_WHAT(s.boundedParametricCostLarge(lo, hi, shortFlags, g, 1.0), start);
    CHECK_WHAT(s.boundedParametricRhsLarge(few, hi, shortBasis, d, 1.0), bounds);   // the bounds first
    CHECK_WHAT(s.boundedParametricRhsLarge(lo, hi, from, g, 1.0), "Solver::boundedParametricRhs: d size != rows(A)");
    CHECK_WHAT(s.boundedParametricCostLarge(lo, hi, from, d, 1.0), "Solver::boundedParametricCost: g size != cols(A)");
    // the LDS methods answer the same way
    CHECK_WHAT(s.boundedParametricRhs(few, hi, from, d, 1.0), bounds);
    CHECK_WHAT(s.boundedParametricCost(lo, hi, shortBasis, g, 1.0), start);
}

TEST(BoundedParametricLarge_AResultThatIsNotOptimalKeepsItsStatus) {
    const Solver s(problem());
    const std::vector<double> lo(SN, 0.0), hi(SN, 9.0), few(SN - 1, 0.0);
    const VectorXd d = VectorXd::Zero(SM), g = VectorXd::Zero(SN);
    Solver::BoundedResult from;   // sizes not looked at: nothing is analysed
    from.basis = {5, 4, 3};
    for (int status : {LP_INFEASIBLE, LP_UNBOUNDED, LP_ITER_LIMIT, LP_SINGULAR}) {
        from.status = status;
        const Solver::BoundedParametric a = s.boundedParametricRhsLarge(lo, hi, from, d, 1.0);
        const Solver::BoundedParametric c = s.boundedParametricCostLarge(lo, hi, from, g, 1.0);
        CHECK(a.status == status && a.t.size() == 0 && a.obj.size() == 0 && a.slope.size() == 0 && a.side.empty());
        CHECK(c.status == status && c.enter.empty() && c.leave.empty() && c.basis == from.basis);
    }
    CHECK_WHAT(s.boundedParametricRhsLarge(few, hi, from, d, 1.0), "Solver::boundedParametric: lo / hi size != cols(A)");
}

int main(int argc, char** argv) { return run_all(argc > 1 ? argv[1] : nullptr); }
