// The Solver::boundedSimplexLarge and Solver::boundedResolveLarge overloads that take a pivot rule, before they reach
// the device: wrong-sized bounds and starts throw std::invalid_argument with the method's own name under every rule,
// whatever throw_on_failure says, and the bounds are checked before the start.  Needs no GPU.  (No test_ prefix:
// tests/test_bounded_large_rules_cpp.py runs this program.)
#include <stdexcept>
#include <string>

#include "check.h"
#include "Canonical.h"
#include "SimplexSolover.h"

using lpla::MatrixXd;
using lpla::VectorXd;
typedef Solver::PivotRule Rule;

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

TEST(BoundedLargeRules_SizeChecks) {
    const Solver s(problem());
    const std::vector<double> lo(SN, 0.0), hi(SN, 9.0), few(SN - 1, 0.0);
    Solver::BoundedResult from, shortBasis, shortFlags;
    from.basis = shortFlags.basis = {3, 4, 5};
    shortBasis.basis = {3, 4};
    from.atUpper = shortBasis.atUpper = {0, 1, 0, 0, 0, 0};
    shortFlags.atUpper = {0, 1, 0, 0, 0};
    for (Rule rule : {Rule::Dantzig, Rule::Bland, Rule::Devex})
        for (bool thr : {true, false}) {
            CHECK_WHAT(s.boundedSimplexLarge(few, hi, rule, thr), "Solver::boundedSimplexLarge: lo / hi size != cols(A)");
            CHECK_WHAT(s.boundedSimplexLarge(lo, few, rule, thr), "Solver::boundedSimplexLarge: lo / hi size != cols(A)");
            CHECK_WHAT(s.boundedResolveLarge(few, hi, from, rule, thr),
                       "Solver::boundedResolveLarge: lo / hi size != cols(A)");
            CHECK_WHAT(s.boundedResolveLarge(lo, few, from, rule, thr),
                       "Solver::boundedResolveLarge: lo / hi size != cols(A)");
            CHECK_WHAT(s.boundedResolveLarge(lo, hi, shortBasis, rule, thr),
                       "Solver::boundedResolveLarge: the start's basis / atUpper size != rows(A) / cols(A)");
            CHECK_WHAT(s.boundedResolveLarge(lo, hi, shortFlags, rule, thr),
                       "Solver::boundedResolveLarge: the start's basis / atUpper size != rows(A) / cols(A)");
            // lo / hi first
            CHECK_WHAT(s.boundedResolveLarge(few, hi, shortBasis, rule, thr),
                       "Solver::boundedResolveLarge: lo / hi size != cols(A)");
        }
}

int main(int argc, char** argv) { return run_all(argc > 1 ? argv[1] : nullptr); }
