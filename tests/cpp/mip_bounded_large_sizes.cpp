// Solver::boundedBranchAndBoundLarge before it reaches the device: a wrong-sized mask, wrong-sized bounds and starts
// throw std::invalid_argument with the method's own name, in that order, and a start that is not LP_OPTIMAL keeps its
// status without a search.  Needs no GPU.  (No test_ prefix: tests/test_mip_bounded_large_cpp.py runs this program.)
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

TEST(BoundedBranchAndBoundLarge_SizeChecks) {
    const Solver s(problem());
    const std::vector<double> lo(SN, 0.0), hi(SN, 9.0), few(SN - 1, 0.0);
    const std::vector<bool> mask{true, true, false, false, false, false}, shortMask(SN - 1, false);
    Solver::BoundedResult from, shortBasis, shortFlags;
    from.basis = shortFlags.basis = {3, 4, 5};
    shortBasis.basis = {3, 4};
    from.atUpper = shortBasis.atUpper = {0, 1, 0, 0, 0, 0};
    shortFlags.atUpper = {0, 1, 0, 0, 0};
    CHECK_WHAT(s.boundedBranchAndBoundLarge(shortMask, lo, hi, from),
               "Solver::boundedBranchAndBoundLarge: mask size != cols(A)");
    CHECK_WHAT(s.boundedBranchAndBoundLarge(mask, few, hi, from),
               "Solver::boundedBranchAndBoundLarge: lo / hi size != cols(A)");
    CHECK_WHAT(s.boundedBranchAndBoundLarge(mask, lo, few, from),
               "Solver::boundedBranchAndBoundLarge: lo / hi size != cols(A)");
    CHECK_WHAT(s.boundedBranchAndBoundLarge(mask, lo, hi, shortBasis),
               "Solver::boundedBranchAndBoundLarge: the start's basis / atUpper size != rows(A) / cols(A)");
    CHECK_WHAT(s.boundedBranchAndBoundLarge(mask, lo, hi, shortFlags),
               "Solver::boundedBranchAndBoundLarge: the start's basis / atUpper size != rows(A) / cols(A)");
    // the mask first, then lo / hi, then the start
    CHECK_WHAT(s.boundedBranchAndBoundLarge(shortMask, few, hi, shortBasis),
               "Solver::boundedBranchAndBoundLarge: mask size != cols(A)");
    CHECK_WHAT(s.boundedBranchAndBoundLarge(mask, few, hi, shortBasis),
               "Solver::boundedBranchAndBoundLarge: lo / hi size != cols(A)");
    // the form that solves the relaxation first checks the bounds there
    CHECK_WHAT(s.boundedBranchAndBoundLarge(shortMask, few, hi), "Solver::boundedSimplexLarge: lo / hi size != cols(A)");
}

TEST(BoundedBranchAndBoundLarge_AStartThatIsNotOptimalKeepsItsStatus) {
    const Solver s(problem());
    const std::vector<double> lo(SN, 0.0), hi(SN, 9.0);
    Solver::BoundedResult from;
    from.status = LP_INFEASIBLE;
    const Solver::IntegerResult r = s.boundedBranchAndBoundLarge(std::vector<bool>(1, true), lo, hi, from);
    CHECK(r.status == LP_INFEASIBLE && !r.found && r.nodes == 0);
    CHECK(std::isnan(r.objective) && std::isnan(r.bound) && (int)r.x.size() == SN - SM);
}

int main(int argc, char** argv) { return run_all(argc > 1 ? argv[1] : nullptr); }
