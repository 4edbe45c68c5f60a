// SimplexSolover.h — class Solver, the drop-in for /root/reference/src/SimplexSolover.h:10-452
// (the header keeps the reference's file name, misspelling included, so `#include
// "SimplexSolover.h"` keeps working).  Same constructor, same `solve()` signature and return
// value (x.head(n_orig), :435-439), same exception types; the arithmetic runs on the MI355X
// through lp_simplex_solve (include/simplexmethod_amd.h).
//
// solve() reproduces the live path of the reference: solve() -> solveWithBasis (:288-296,
// :408-451).  The reference's two-phase / artificial-basis code (:15-95, :211-265, :331-406) is
// unreachable through its public API (Canonical's constructor rejects an empty basis,
// Canonical.cpp:35-38) and internally inconsistent; twoPhaseSimplex() below is
// that flow designed afresh on the same GPU pivot kernels: it ignores the
// problem's basis indices and needs no feasible starting basis.
#pragma once

#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "Canonical.h"
#include "DeviceContext.h"

class Solver {
public:
    static constexpr double EPS = 1e-9;     // SimplexSolover.h:13
    static constexpr int MAX_ITER = 10000;  // SimplexSolover.h:426

    struct Result {            // what the reference computes but never returns (N is local, :419)
        lpla::VectorXd x;      // x.head(n_orig)
        std::vector<int> basis;  // final basis by position
        double objective = 0.0;  // Canonical::Evaluate of the full vertex
        int iterations = 0;
        int status = LP_OPTIMAL;
    };

    // The pivot rule of solve() and twoPhaseSimplex(): Dantzig's (the reference's, the default), Bland's,
    // which never cycles on degenerate problems and usually takes more pivots, or Devex pricing, which takes
    // fewer pivots on badly scaled or large problems and runs on a slower-per-pivot path
    // (include/simplexmethod_amd.h).
    enum class PivotRule { Dantzig = LP_PIVOT_DANTZIG, Bland = LP_PIVOT_BLAND, Devex = LP_PIVOT_DEVEX };
    // The pricing rule of the dual simplex of boundedResolve() and boundedResolveLarge(): the most violated basis
    // position leaves (Dantzig, the default), or the one of largest violation^2 / reference weight (Devex), which
    // takes fewer dual pivots on LPs of many rows (include/simplexmethod_amd.h, LP_DUAL_*).
    enum class DualRule { Dantzig = LP_DUAL_DANTZIG, Devex = LP_DUAL_DEVEX };
    // The ratio test of that dual simplex: the column of smallest ratio enters whatever its own box (Textbook, the
    // default), or a candidate whose flip to its other bound leaves the leaving row violated is flipped, O(m), and the
    // next one looked at (LongStep, the bound-flipping ratio test), which takes fewer dual pivots on boxed LPs
    // (include/simplexmethod_amd.h, LP_DUAL_RATIO_*).
    enum class DualRatio { Textbook = LP_DUAL_RATIO_TEXTBOOK, LongStep = LP_DUAL_RATIO_LONG_STEP };

    explicit Solver(const Canonical& problem, int device = 0) : _problem(problem), _device(device) {}

    void setPivotRule(PivotRule rule) { _rule = rule; }
    PivotRule pivotRule() const { return _rule; }

    // Throws std::runtime_error (unbounded / iteration limit / singular basis) like the
    // reference (:126, :443, :450).
    lpla::VectorXd solve() { return solve_ex().x; }

    Result solve_ex(bool throw_on_failure = true) {
        const View p = view();                                           // :409-414
        const std::vector<int>& basis = _problem.GetBasisIndices();
        lp_context* ctx = lpgpu::context(_device);
        Result r;
        r.x = lpla::VectorXd::Zero(p.no);
        r.basis.assign((size_t)p.m, -1);
        r.status = lp_simplex_solve_ex(ctx, p.A, p.m, p.n, p.b, p.c, basis.data(), p.maximize, p.no, EPS, MAX_ITER,
                                       r.x.data(), r.basis.data(), &r.objective, &r.iterations,
                                       static_cast<int>(_rule));
        if (throw_on_failure) lpgpu::throw_for_status(r.status, ctx);
        return r;
    }

    // Two-phase simplex for problems without a usable starting basis (Symmetrical min problems,
    // negative b): the reference's private twoPhaseSimplex (:383-406) with make_b_nonneg (:61-68),
    // createAuxiliaryProblem (:70-95) and replaceArtificialColumns (:331-381), every pivot on the
    // GPU (lp_simplex_two_phase).  The problem's basis indices are ignored.  Throws
    // std::runtime_error like the reference's sketch: no feasible solution (:352-353), linearly
    // dependent constraints (:372-380), unbounded, iteration limit.
    lpla::VectorXd twoPhaseSimplex() { return twoPhaseSimplex_ex().x; }

    Result twoPhaseSimplex_ex(bool throw_on_failure = true, int phase_iterations[3] = nullptr) {
        const View p = view();
        lp_context* ctx = lpgpu::context(_device);
        Result r;
        r.x = lpla::VectorXd::Zero(p.no);
        r.basis.assign((size_t)p.m, -1);
        int it[3] = {0, 0, 0};
        r.status = lp_simplex_two_phase_ex(ctx, p.A, p.m, p.n, p.b, p.c, p.maximize, p.no, EPS, MAX_ITER, r.x.data(),
                                           r.basis.data(), &r.objective, it, static_cast<int>(_rule));
        r.iterations = it[0] + it[1] + it[2];
        if (phase_iterations)
            for (int k = 0; k < 3; ++k) phase_iterations[k] = it[k];
        if (throw_on_failure) lpgpu::throw_for_status(r.status, ctx);
        return r;
    }

    // The dual solution at a result's final basis (lp_basis_duals): shadow prices y (dz/db for max and min
    // alike), reduced costs d = c - A^T y (exactly 0 on the basis) and the dual objective b.y.  At an optimum
    // of a max problem d <= EPS, of a min problem d >= -EPS, and objective equals the primal objective.
    // status: LP_OPTIMAL, LP_SINGULAR (y, d and objective NaN); a result that is not LP_OPTIMAL keeps its
    // status and gets NaN.
    struct Duals {
        lpla::VectorXd y, d;
        double objective = 0.0;
        int status = LP_OPTIMAL;
    };

    Duals duals(const Result& r) const {
        const View p = view();
        Duals out;
        out.y = lpla::VectorXd::Zero(p.m);
        out.d = lpla::VectorXd::Zero(p.n);
        out.status = r.status;
        if (r.status == LP_OPTIMAL) {
            if ((int)r.basis.size() != p.m) throw std::invalid_argument("Solver::duals: basis size != rows(A)");
            lp_context* ctx = lpgpu::context(_device);
            out.status = checked(lp_basis_duals(ctx, p.A, p.m, p.n, p.b, p.c, r.basis.data(), out.y.data(),
                                                out.d.data(), &out.objective), ctx);
        }
        if (out.status != LP_OPTIMAL) {
            out.y = nans(p.m);
            out.d = nans(p.n);
            out.objective = kNaN;
        }
        return out;
    }

    // RHS and cost ranging at a result's final basis (lp_basis_ranging) with EPS and the problem's sense: for each
    // b_i and c_j the interval over which that basis stays feasible / optimal (the others fixed), and the column
    // that leaves (b) or enters (c) at each end, -1 at an infinite end.  The ranges describe the basis, whose
    // optimality is not re-checked; at a degenerate optimum they can be narrower than the interval over which the
    // optimal value stays linear.  status: LP_OPTIMAL, LP_SINGULAR (NaN, -1); a result that is not LP_OPTIMAL
    // keeps its status and gets NaN.
    struct Ranging {
        lpla::VectorXd b_lo, b_hi, c_lo, c_hi;
        std::vector<int> b_leave_lo, b_leave_hi, c_enter_lo, c_enter_hi;
        int status = LP_OPTIMAL;
    };

    Ranging ranging(const Result& r) const {
        const View p = view();
        RangingEnds ends(p.m, p.n);
        Ranging out;
        out.status = r.status;
        if (r.status == LP_OPTIMAL) {
            if ((int)r.basis.size() != p.m) throw std::invalid_argument("Solver::ranging: basis size != rows(A)");
            lp_context* ctx = lpgpu::context(_device);
            out.status = checked(lp_basis_ranging(ctx, p.A, p.m, p.n, p.b, p.c, r.basis.data(), p.maximize, EPS,
                                                  ends.rhs.data(), ends.rv.data(), ends.cost.data(), ends.cv.data()),
                                 ctx);
        }
        ends.unpack(out);
        return out;
    }

    // The optimal value along b + t d for t in [0, tMax] (lp_basis_parametric) from a result's final basis, with EPS
    // and the problem's sense: breakpoints t (nseg+1), the optimal value at each (obj, nseg+1), the slope of each
    // segment and the pivot that ends it (enter / leave, nseg; enter -1 on the last segment).  status: LP_OPTIMAL
    // (reached tMax), LP_INFEASIBLE (infeasible past the last t), LP_ITER_LIMIT (more than MAX_BREAKS breakpoints),
    // LP_SINGULAR; a result that is not LP_OPTIMAL keeps its status and gets no segments.
    static constexpr int MAX_BREAKS = 64;
    struct Parametric {
        lpla::VectorXd t, obj, slope;
        std::vector<int> enter, leave, basis;
        int status = LP_OPTIMAL;
    };

    Parametric parametricRhs(const Result& r, const lpla::VectorXd& d, double tMax) const {
        return parametric(false, r, d, tMax);
    }

    // The optimal value along c + t g for t in [0, tMax] (lp_basis_parametric_cost) from a result's final basis, with
    // EPS and the problem's sense, in the Parametric form of parametricRhs: breakpoints t (nseg+1), the optimal value
    // at each (obj, nseg+1), the slope of each segment and the pivot that ends it (enter / leave, nseg; leave -1 on the
    // last segment).  status: LP_OPTIMAL (reached tMax), LP_UNBOUNDED (unbounded past the last t), LP_ITER_LIMIT (more
    // than MAX_BREAKS breakpoints), LP_SINGULAR; a result that is not LP_OPTIMAL keeps its status and gets no
    // segments.
    Parametric parametricCost(const Result& r, const lpla::VectorXd& g, double tMax) const {
        return parametric(true, r, g, tMax);
    }

    // Depth-first branch-and-bound (lp_mip_solve) with EPS and the problem's sense: the columns j with integer[j]
    // (one entry per column of A, none past the original variables) must be integral.  The root starts from the
    // problem's own basis, or from a result's final basis in the second form (a result that is not LP_OPTIMAL keeps
    // its status and gets found = false).  status: LP_OPTIMAL (the incumbent is optimal), LP_INFEASIBLE,
    // LP_UNBOUNDED (the root relaxation), LP_ITER_LIMIT (a depth, node or pivot limit: bound - objective is the gap
    // left), LP_SINGULAR.  x holds the original variables of the incumbent, NaN without one.  A basis that is no
    // valid start, a bad mask or a shape beyond lp_mip_fits throws std::invalid_argument.
    struct IntegerResult {
        int status = LP_OPTIMAL;
        bool found = false;
        lpla::VectorXd x;
        double objective = std::numeric_limits<double>::quiet_NaN();
        double bound = std::numeric_limits<double>::quiet_NaN();
        int nodes = 0;
        int restored = 0, rebuilt = 0;   // boundedBranchAndBoundLarge with snapshots: second children by kind
    };
    static constexpr double INT_TOL = 1e-6;
    static constexpr double MIP_GAP = 1e-9;

    IntegerResult branchAndBound(const std::vector<bool>& integer, int maxDepth = 32, int maxNodes = 100000) const {
        Result r;
        r.status = LP_OPTIMAL;
        r.basis = _problem.GetBasisIndices();
        return branchAndBound(integer, r, maxDepth, maxNodes);
    }

    IntegerResult branchAndBound(const std::vector<bool>& integer, const Result& r, int maxDepth = 32,
                                 int maxNodes = 100000) const {
        const View p = view();
        IntegerResult out = blankIntegerResult(r.status, p.no);
        if (r.status != LP_OPTIMAL) return out;
        if ((int)integer.size() != p.n) throw std::invalid_argument("Solver::branchAndBound: mask size != cols(A)");
        if ((int)r.basis.size() != p.m) throw std::invalid_argument("Solver::branchAndBound: basis size != rows(A)");
        const std::vector<int> mask(integer.begin(), integer.end());
        lp_context* ctx = lpgpu::context(_device);
        int found = 0, stats[4] = {0, 0, 0, 0};
        out.status = checked(lp_mip_solve(ctx, p.A, p.m, p.n, p.b, p.c, r.basis.data(), p.maximize, p.no, mask.data(),
                                          EPS, INT_TOL, MIP_GAP, maxDepth, maxNodes, MAX_ITER, out.x.data(),
                                          &out.objective, &out.bound, &found, stats), ctx);
        out.found = found != 0;
        out.nodes = stats[0];
        return out;
    }

    // The two-phase bounded-variable simplex (lp_simplex_bounded) with EPS, MAX_ITER and the problem's sense:
    // lo <= x <= hi per column of A (lo finite, hi finite or +inf, lo == hi a fixed column).  The problem's basis
    // indices are ignored.  atUpper[j] = 1 where the column is held complemented (a non-basic column at its upper
    // bound); iterations = phase-I pivots, drive-out pivots, phase-II pivots, bound flips.  x (the original
    // variables) and objective are NaN unless LP_OPTIMAL.  Throws like twoPhaseSimplex (std::runtime_error for
    // infeasible, unbounded, iteration limit, dependent rows) unless throw_on_failure is false; bad bounds, wrong
    // sizes or a shape beyond lp_simplex_bounded_fits throw std::invalid_argument either way.
    struct BoundedResult {
        lpla::VectorXd x;
        std::vector<int> basis;
        std::vector<int> atUpper;
        double objective = std::numeric_limits<double>::quiet_NaN();
        int iterations[4] = {0, 0, 0, 0};
        int status = LP_OPTIMAL;
    };

    BoundedResult boundedSimplex(const std::vector<double>& lo, const std::vector<double>& hi,
                                 bool throw_on_failure = true) const {
        return boundedRun("Solver::boundedSimplex", lo, hi, nullptr, nullptr, throw_on_failure);
    }

    // The same under a pivot rule (lp_simplex_bounded_ex), in phase I and phase II: PivotRule::Bland cannot cycle,
    // PivotRule::Devex prices on d*d/w and needs cols(A) more doubles of LDS (lp_simplex_bounded_rule_fits, else
    // std::invalid_argument); PivotRule::Dantzig is the form above bit for bit.  The forms without a rule ignore
    // setPivotRule.
    BoundedResult boundedSimplex(const std::vector<double>& lo, const std::vector<double>& hi, PivotRule rule,
                                 bool throw_on_failure = true) const {
        return boundedRun("Solver::boundedSimplex", lo, hi, nullptr, &rule, throw_on_failure);
    }

    // The same at any shape twoPhaseSimplex runs (lp_simplex_bounded_large): the tableau stays in device memory, one
    // selector and one update launch per iteration, Dantzig's rule; no lp_simplex_bounded_fits limit.  Result and
    // exceptions as boundedSimplex(lo, hi), and equal to it where both run.
    BoundedResult boundedSimplexLarge(const std::vector<double>& lo, const std::vector<double>& hi,
                                      bool throw_on_failure = true) const {
        return boundedRun("Solver::boundedSimplexLarge", lo, hi, nullptr, nullptr, throw_on_failure, true);
    }

    // The same under a pivot rule (lp_simplex_bounded_large_ex), in phase I and phase II, with no
    // lp_simplex_bounded_rule_fits limit: PivotRule::Bland cannot cycle, PivotRule::Devex keeps its weights in device
    // memory, PivotRule::Dantzig is the form above bit for bit.  Equal to boundedSimplex(lo, hi, rule) where both run.
    BoundedResult boundedSimplexLarge(const std::vector<double>& lo, const std::vector<double>& hi, PivotRule rule,
                                      bool throw_on_failure = true) const {
        return boundedRun("Solver::boundedSimplexLarge", lo, hi, nullptr, &rule, throw_on_failure, true);
    }

    // The same problem under the bounds lo, hi re-solved from the basis and flags of an earlier result
    // (lp_simplex_bounded_resolve): the bounded primal loop if `from` is still primal feasible, the bounded dual
    // simplex if it is only dual feasible, which it stays under any change of the bounds.  iterations = dual pivots,
    // primal pivots, bound flips, 0.  Exceptions as boundedSimplex; a start that is neither primal nor dual feasible,
    // a flag on a column without an upper bound or a basis index outside the columns throw std::invalid_argument.
    BoundedResult boundedResolve(const std::vector<double>& lo, const std::vector<double>& hi,
                                 const BoundedResult& from, bool throw_on_failure = true) const {
        return boundedRun("Solver::boundedResolve", lo, hi, &from, nullptr, throw_on_failure);
    }

    // The re-solve at any shape boundedSimplexLarge runs (lp_simplex_bounded_resolve_large), normally from its
    // result: the basis is installed on the tableau in device memory, then the bounded primal or dual loop runs there,
    // Dantzig's rule; no lp_simplex_bounded_fits limit.  Result and exceptions as boundedResolve(lo, hi, from), and
    // equal to it where both run.
    BoundedResult boundedResolveLarge(const std::vector<double>& lo, const std::vector<double>& hi,
                                      const BoundedResult& from, bool throw_on_failure = true) const {
        return boundedRun("Solver::boundedResolveLarge", lo, hi, &from, nullptr, throw_on_failure, true);
    }

    // The same under a pivot rule (lp_simplex_bounded_resolve_large_ex): the rule governs the primal loop only.  Equal
    // to boundedResolve(lo, hi, from, rule) where both run.
    BoundedResult boundedResolveLarge(const std::vector<double>& lo, const std::vector<double>& hi,
                                      const BoundedResult& from, PivotRule rule, bool throw_on_failure = true) const {
        return boundedRun("Solver::boundedResolveLarge", lo, hi, &from, &rule, throw_on_failure, true);
    }

    // The same under a pivot rule (lp_simplex_bounded_resolve_ex): the rule governs the primal loop only; the dual
    // simplex is the same under every rule.
    BoundedResult boundedResolve(const std::vector<double>& lo, const std::vector<double>& hi,
                                 const BoundedResult& from, PivotRule rule, bool throw_on_failure = true) const {
        return boundedRun("Solver::boundedResolve", lo, hi, &from, &rule, throw_on_failure);
    }

    // boundedResolve under a pivot rule and a dual pricing rule (lp_simplex_bounded_resolve_dual_ex): `rule` governs
    // the primal loop only and `dual` the dual simplex only.  DualRule::Dantzig is the form above bit for bit; under
    // DualRule::Devex status and objective are its up to rounding, the optimal basis and the pivot count may differ.  A
    // shape beyond lp_simplex_bounded_dual_rule_fits throws std::invalid_argument.
    BoundedResult boundedResolve(const std::vector<double>& lo, const std::vector<double>& hi,
                                 const BoundedResult& from, PivotRule rule, DualRule dual,
                                 bool throw_on_failure = true) const {
        return boundedRun("Solver::boundedResolve", lo, hi, &from, &rule, throw_on_failure, false, &dual);
    }

    // The same at any shape boundedSimplexLarge runs (lp_simplex_bounded_resolve_large_dual_ex): the dual weights live
    // in device memory.  Equal to boundedResolve(lo, hi, from, rule, dual) where both run.
    BoundedResult boundedResolveLarge(const std::vector<double>& lo, const std::vector<double>& hi,
                                      const BoundedResult& from, PivotRule rule, DualRule dual,
                                      bool throw_on_failure = true) const {
        return boundedRun("Solver::boundedResolveLarge", lo, hi, &from, &rule, throw_on_failure, true, &dual);
    }

    // boundedResolve under a dual ratio test too (lp_simplex_bounded_resolve_ratio_ex): `ratio` governs the entering
    // step of the dual simplex only.  DualRatio::Textbook is the form above bit for bit; under DualRatio::LongStep
    // status and objective are its up to rounding, and iterations[2] counts the dual simplex's bound flips.
    BoundedResult boundedResolve(const std::vector<double>& lo, const std::vector<double>& hi,
                                 const BoundedResult& from, PivotRule rule, DualRule dual, DualRatio ratio,
                                 bool throw_on_failure = true) const {
        return boundedRun("Solver::boundedResolve", lo, hi, &from, &rule, throw_on_failure, false, &dual, &ratio);
    }

    // The same at any shape boundedSimplexLarge runs (lp_simplex_bounded_resolve_large_ratio_ex).  Equal to
    // boundedResolve(lo, hi, from, rule, dual, ratio) where both run.
    BoundedResult boundedResolveLarge(const std::vector<double>& lo, const std::vector<double>& hi,
                                      const BoundedResult& from, PivotRule rule, DualRule dual, DualRatio ratio,
                                      bool throw_on_failure = true) const {
        return boundedRun("Solver::boundedResolveLarge", lo, hi, &from, &rule, throw_on_failure, true, &dual, &ratio);
    }

    // The dual solution of the bounded problem at a result's basis and flags (lp_basis_bounded_duals), in the original
    // variables: the point x (all columns of A) the basis and the flags define, shadow prices y, reduced costs d
    // (exactly 0 on the basis) and objective = b.y + sum d_j x_j over the non-basic columns, which equals c.x at an
    // optimum.  There a max problem has d <= EPS at a lower bound and d >= -EPS at an upper bound, a min problem the
    // other way round.  status: LP_OPTIMAL, LP_SINGULAR or LP_INFEASIBLE (some hi < lo), the last two with NaN; a
    // result that is not LP_OPTIMAL keeps its status and gets NaN.  Wrong sizes, bad bounds, a bad flag or index or a
    // shape beyond lp_basis_bounded_fits throw std::invalid_argument.
    struct BoundedDuals {
        lpla::VectorXd x, y, d;
        double objective = std::numeric_limits<double>::quiet_NaN();
        int status = LP_OPTIMAL;
    };

    BoundedDuals boundedDuals(const std::vector<double>& lo, const std::vector<double>& hi,
                              const BoundedResult& from) const {
        return boundedDualsRun("Solver::boundedDuals", lo, hi, from, false);
    }

    // The same at any shape boundedSimplexLarge runs (lp_basis_bounded_duals_large), normally at its result: the
    // analysis on a tableau in device memory, no lp_basis_bounded_fits limit.  Result and exceptions as
    // boundedDuals(lo, hi, from) minus the fit, and equal to it where both run.
    BoundedDuals boundedDualsLarge(const std::vector<double>& lo, const std::vector<double>& hi,
                                   const BoundedResult& from) const {
        return boundedDualsRun("Solver::boundedDualsLarge", lo, hi, from, true);
    }

    // RHS and cost ranging of the bounded problem at a result's basis and flags (lp_basis_bounded_ranging) with EPS and
    // the problem's sense: the fields of Ranging, plus for each end of a b range the bound its leaving variable leaves
    // at (b_side_lo / b_side_hi: 0 lower, 1 upper, -1 at an infinite end).  A non-basic column at its upper bound is
    // ranged with the opposite sense.  Statuses and exceptions as boundedDuals.
    struct BoundedRanging : Ranging {
        std::vector<int> b_side_lo, b_side_hi;
    };

    BoundedRanging boundedRanging(const std::vector<double>& lo, const std::vector<double>& hi,
                                  const BoundedResult& from) const {
        return boundedRangingRun("Solver::boundedRanging", lo, hi, from, false);
    }

    // The same at any shape boundedSimplexLarge runs (lp_basis_bounded_ranging_large); result and exceptions as
    // boundedRanging(lo, hi, from) minus the fit, and equal to it where both run.
    BoundedRanging boundedRangingLarge(const std::vector<double>& lo, const std::vector<double>& hi,
                                       const BoundedResult& from) const {
        return boundedRangingRun("Solver::boundedRangingLarge", lo, hi, from, true);
    }

    // Depth-first branch-and-bound over the bounds (lp_mip_bounded_solve) with EPS, INT_TOL, MIP_GAP, MAX_ITER and the
    // problem's sense: the bounded problem of boundedSimplex with the columns j of integer[j] integral (their lo and
    // finite hi must be integers).  A branch changes one bound, so the depth is not traded against the shape: maxDepth
    // goes to 1024.  The first form solves the relaxation by boundedSimplex first; the second starts from a result's
    // basis and flags (a result that is not LP_OPTIMAL keeps its status and gets found = false).  IntegerResult as
    // branchAndBound.  Exceptions as boundedResolve (wrong sizes, a start that is no valid one, bad bounds) and
    // branchAndBound (a bad mask, a shape beyond lp_mip_bounded_fits): std::invalid_argument.
    IntegerResult boundedBranchAndBound(const std::vector<bool>& integer, const std::vector<double>& lo,
                                        const std::vector<double>& hi, int maxDepth = 64,
                                        int maxNodes = 100000) const {
        return boundedBranchAndBound(integer, lo, hi, boundedSimplex(lo, hi, false), maxDepth, maxNodes);
    }

    IntegerResult boundedBranchAndBound(const std::vector<bool>& integer, const std::vector<double>& lo,
                                        const std::vector<double>& hi, const BoundedResult& from, int maxDepth = 64,
                                        int maxNodes = 100000) const {
        return boundedSearch("Solver::boundedBranchAndBound", integer, lo, hi, from, maxDepth, maxNodes, false);
    }

    // The same search at any shape boundedSimplexLarge runs (lp_mip_bounded_solve_large): the tableau stays in device
    // memory from a node to its first child, a second child is rebuilt there; no lp_mip_bounded_fits limit.  The first
    // form solves the relaxation by boundedSimplexLarge.  Result and exceptions as boundedBranchAndBound minus the fit,
    // and equal to it where both run.
    IntegerResult boundedBranchAndBoundLarge(const std::vector<bool>& integer, const std::vector<double>& lo,
                                             const std::vector<double>& hi, int maxDepth = 64,
                                             int maxNodes = 100000) const {
        return boundedBranchAndBoundLarge(integer, lo, hi, boundedSimplexLarge(lo, hi, false), maxDepth, maxNodes);
    }

    IntegerResult boundedBranchAndBoundLarge(const std::vector<bool>& integer, const std::vector<double>& lo,
                                             const std::vector<double>& hi, const BoundedResult& from,
                                             int maxDepth = 64, int maxNodes = 100000) const {
        return boundedSearch("Solver::boundedBranchAndBoundLarge", integer, lo, hi, from, maxDepth, maxNodes, true);
    }

    // The same with up to `snapshots` tableau snapshots in device memory (lp_mip_bounded_solve_large_ex, snapshots in
    // [0, 1024], else std::invalid_argument): a second child whose level's snapshot is still there starts from its
    // parent's final tableau like a first child instead of being rebuilt.  restored and rebuilt count the second
    // children by kind.  Status, found and nodes are those of the forms above; the objective agrees to rounding.
    IntegerResult boundedBranchAndBoundLarge(const std::vector<bool>& integer, const std::vector<double>& lo,
                                             const std::vector<double>& hi, int maxDepth, int maxNodes,
                                             int snapshots) const {
        return boundedBranchAndBoundLarge(integer, lo, hi, boundedSimplexLarge(lo, hi, false), maxDepth, maxNodes,
                                          snapshots);
    }

    IntegerResult boundedBranchAndBoundLarge(const std::vector<bool>& integer, const std::vector<double>& lo,
                                             const std::vector<double>& hi, const BoundedResult& from, int maxDepth,
                                             int maxNodes, int snapshots) const {
        return boundedSearch("Solver::boundedBranchAndBoundLarge", integer, lo, hi, from, maxDepth, maxNodes, true,
                             snapshots);
    }

    // The searches above under a dual ratio test (lp_mip_bounded_solve_ratio_ex, lp_mip_bounded_solve_large_ratio_ex):
    // `ratio` governs the entering step of every dual simplex run of the search, the root's, a first child's and a
    // second child's, rebuilt or restored.  DualRatio::Textbook is the form without it in every value; under
    // DualRatio::LongStep node order, branching and pruning are unchanged and the objective agrees within MIP_GAP plus
    // rounding wherever both searches finish.  Pricing stays Dantzig's.
    IntegerResult boundedBranchAndBound(const std::vector<bool>& integer, const std::vector<double>& lo,
                                        const std::vector<double>& hi, const BoundedResult& from, int maxDepth,
                                        int maxNodes, DualRatio ratio) const {
        return boundedSearch("Solver::boundedBranchAndBound", integer, lo, hi, from, maxDepth, maxNodes, false, -1,
                             &ratio);
    }

    IntegerResult boundedBranchAndBoundLarge(const std::vector<bool>& integer, const std::vector<double>& lo,
                                             const std::vector<double>& hi, const BoundedResult& from, int maxDepth,
                                             int maxNodes, int snapshots, DualRatio ratio) const {
        return boundedSearch("Solver::boundedBranchAndBoundLarge", integer, lo, hi, from, maxDepth, maxNodes, true,
                             snapshots, &ratio);
    }

    // Evidence for a result that is not optimal (lp_basis_certificate) at its final basis, with EPS and the problem's
    // sense.  A basis index n+i is row i's artificial, so the phase-I basis of an infeasible twoPhaseSimplex_ex(false)
    // result passes as it is.  kind LP_CERT_FARKAS: A^T farkas >= -EPS and b.farkas = value < 0 (no x >= 0 solves
    // A x = b); LP_CERT_RAY: A ray = 0, ray >= -EPS and c.ray = value improving (the objective is unbounded);
    // LP_CERT_NONE: nothing that passes its own EPS test.  farkas / ray are NaN unless the kind is theirs.
    // status: the result's LP_INFEASIBLE / LP_UNBOUNDED when a certificate was computed, LP_SINGULAR when the
    // crash fails; any other result keeps its status and gets NONE.
    struct Certificate {
        int kind = LP_CERT_NONE;
        lpla::VectorXd farkas, ray;
        double value = std::numeric_limits<double>::quiet_NaN();
        int index = -1;
        int status = LP_OPTIMAL;
    };

    Certificate certificate(const Result& r) const {
        const View p = view();
        Certificate out = blankCertificate(p, r.status);
        if (hasCertificate(r.status)) {
            if ((int)r.basis.size() != p.m) throw std::invalid_argument("Solver::certificate: basis size != rows(A)");
            lp_context* ctx = lpgpu::context(_device);
            mergeStatus(out, lp_basis_certificate(ctx, p.A, p.m, p.n, p.b, p.c, r.basis.data(), p.maximize, EPS,
                                                  &out.kind, out.farkas.data(), out.ray.data(), &out.value,
                                                  &out.index), ctx);
        }
        return out;
    }

    // Evidence for a bounded result that is not optimal (lp_basis_bounded_certificate) at its basis and flags, under
    // the bounds lo, hi it was solved with, with the given eps and the problem's sense, in the original variables.  A
    // basis index n+i is row i's artificial, so the phase-I basis of an infeasible boundedSimplex(lo, hi, false) result
    // passes as it is, as does the basis an infeasible or unbounded boundedResolve stopped at.  kind LP_CERT_FARKAS:
    // with g = A^T farkas, b.farkas < sum_j min(g_j lo_j, g_j hi_j) (no x in the box solves A x = b); LP_CERT_RAY:
    // A ray = 0, ray >= -eps, ray_k <= eps wherever hi_k is finite and c.ray = value improving; LP_CERT_NONE: nothing
    // that passes its own eps test.  status: the result's LP_INFEASIBLE / LP_UNBOUNDED when a certificate was computed
    // (an LP with some hi < lo is LP_INFEASIBLE with NONE), LP_SINGULAR when the crash fails; any other result keeps
    // its status and gets NONE.  Exceptions as boundedDuals.
    Certificate boundedCertificate(const std::vector<double>& lo, const std::vector<double>& hi,
                                   const BoundedResult& from, double eps = EPS) const {
        return boundedCertificateRun("Solver::boundedCertificate", lo, hi, from, eps, false);
    }

    // The same at any shape boundedSimplexLarge and boundedResolveLarge run (lp_basis_bounded_certificate_large):
    // result and exceptions as boundedCertificate(lo, hi, from, eps) minus the fit, and equal to it where both run.
    Certificate boundedCertificateLarge(const std::vector<double>& lo, const std::vector<double>& hi,
                                        const BoundedResult& from, double eps = EPS) const {
        return boundedCertificateRun("Solver::boundedCertificateLarge", lo, hi, from, eps, true);
    }

    // The optimal value of the bounded problem along b + t d (boundedParametricRhs, lp_basis_bounded_parametric) or
    // along c + t g (boundedParametricCost, lp_basis_bounded_parametric_cost) for t in [0, tMax], from a bounded
    // result's basis and flags under the bounds lo, hi it was solved with, with EPS and the problem's sense: the fields
    // of Parametric, plus side (nseg): the bound at which leave[k] stops (0 lower, 1 upper, -1 where leave[k] is -1),
    // and atUpper: the flags that go with the final basis.  On the cost path a bound flip is a breakpoint with
    // enter[k] == leave[k] and side[k] the bound flipped to.  status: LP_OPTIMAL (reached tMax), LP_INFEASIBLE (RHS
    // path: infeasible past the last t; either path: some hi < lo, no segments), LP_UNBOUNDED (cost path: unbounded
    // past the last t), LP_ITER_LIMIT (more than MAX_BREAKS breakpoints), LP_SINGULAR; a result that is not
    // LP_OPTIMAL keeps its status and gets no segments.  Exceptions as boundedDuals, with lp_basis_bounded_parametric_fits
    // / _cost_fits as the shape's limit; a result that is not optimal at t = 0 throws std::invalid_argument too.
    struct BoundedParametric : Parametric {
        std::vector<int> side, atUpper;
    };

    BoundedParametric boundedParametricRhs(const std::vector<double>& lo, const std::vector<double>& hi,
                                           const BoundedResult& from, const lpla::VectorXd& d, double tMax) const {
        return boundedParametric(false, lo, hi, from, d, tMax);
    }

    BoundedParametric boundedParametricCost(const std::vector<double>& lo, const std::vector<double>& hi,
                                            const BoundedResult& from, const lpla::VectorXd& g, double tMax) const {
        return boundedParametric(true, lo, hi, from, g, tMax);
    }

    // The same at any shape boundedSimplexLarge and boundedResolveLarge run (lp_basis_bounded_parametric_large,
    // lp_basis_bounded_parametric_cost_large): result and exceptions as boundedParametricRhs / boundedParametricCost
    // minus the fit (the selector's LDS bounds the rows instead: 6638 and 3982), and equal to them where both run.
    BoundedParametric boundedParametricRhsLarge(const std::vector<double>& lo, const std::vector<double>& hi,
                                                const BoundedResult& from, const lpla::VectorXd& d, double tMax) const {
        return boundedParametric(false, lo, hi, from, d, tMax, true);
    }

    BoundedParametric boundedParametricCostLarge(const std::vector<double>& lo, const std::vector<double>& hi,
                                                 const BoundedResult& from, const lpla::VectorXd& g,
                                                 double tMax) const {
        return boundedParametric(true, lo, hi, from, g, tMax, true);
    }

private:
    // The problem as the ABI takes it
    struct View {
        const double *A, *b, *c;
        int m, n, no, maximize;
    };
    View view() const {
        const lpla::MatrixXd& A = _problem.GetConstraintsMatrix();
        return {A.data(), _problem.GetRightHandSide().data(), _problem.GetObjectiveCoefficients().data(),
                (int)A.rows(), (int)A.cols(), _problem.GetOriginalVariablesCount(), _problem.IsMaximization() ? 1 : 0};
    }

    static constexpr double kNaN = std::numeric_limits<double>::quiet_NaN();

    // A status the analyses and searches hand back as it is; a runtime failure or a refused argument throws
    static int checked(int st, lp_context* ctx) {
        if (st < 0 || st == LP_BAD_ARG) lpgpu::throw_for_status(st, ctx);
        return st;
    }

    static lpla::VectorXd nans(int size) {
        lpla::VectorXd v = lpla::VectorXd::Zero(size);
        for (int i = 0; i < size; ++i) v[i] = kNaN;
        return v;
    }

    static void requireBounds(const char* who, const View& p, const std::vector<double>& lo,
                              const std::vector<double>& hi) {
        if ((int)lo.size() != p.n || (int)hi.size() != p.n)
            throw std::invalid_argument(std::string(who) + ": lo / hi size != cols(A)");
    }

    // whose: "start" (a solve or search goes on from it) or "result" (it is analysed)
    static void requireStart(const char* who, const char* whose, const View& p, const BoundedResult& from) {
        if ((int)from.basis.size() != p.m || (int)from.atUpper.size() != p.n)
            throw std::invalid_argument(std::string(who) + ": the " + whose +
                                        "'s basis / atUpper size != rows(A) / cols(A)");
    }

    // The (lo, hi) pairs an ABI ranging call wrote, one per row or column, as two vectors; `fill` in both unless ok
    template <class Vec, class T>
    static void unpackPairs(bool ok, const std::vector<T>& pairs, T fill, Vec& lo, Vec& hi) {
        const size_t count = pairs.size() / 2;
        lo = hi = Vec((long)count);
        for (size_t i = 0; i < count; ++i) {
            lo[(long)i] = ok ? pairs[2 * i] : fill;
            hi[(long)i] = ok ? pairs[2 * i + 1] : fill;
        }
    }

    // What lp_basis_ranging and lp_basis_bounded_ranging fill, and the Ranging it becomes under out.status
    struct RangingEnds {
        std::vector<double> rhs, cost;
        std::vector<int> rv, cv;
        RangingEnds(int m, int n)
            : rhs(2 * (size_t)m, kNaN), cost(2 * (size_t)n, kNaN), rv(2 * (size_t)m, -1), cv(2 * (size_t)n, -1) {}
        void unpack(Ranging& out) const {
            const bool ok = out.status == LP_OPTIMAL;
            unpackPairs(ok, rhs, kNaN, out.b_lo, out.b_hi);
            unpackPairs(ok, rv, -1, out.b_leave_lo, out.b_leave_hi);
            unpackPairs(ok, cost, kNaN, out.c_lo, out.c_hi);
            unpackPairs(ok, cv, -1, out.c_enter_lo, out.c_enter_hi);
        }
    };

    // What the four parametric ABI calls fill at MAX_BREAKS, and the Parametric its first nseg segments become
    struct PathBuffers {
        int nseg = 0;
        std::vector<double> t, obj, slope;
        std::vector<int> enter, leave;
        PathBuffers()
            : t(MAX_BREAKS + 2), obj(MAX_BREAKS + 2), slope(MAX_BREAKS + 1), enter(MAX_BREAKS + 1),
              leave(MAX_BREAKS + 1) {}
        void unpack(Parametric& out) const {
            out.t = lpla::VectorXd::Zero(nseg ? nseg + 1 : 0);
            out.obj = lpla::VectorXd::Zero(nseg ? nseg + 1 : 0);
            out.slope = lpla::VectorXd::Zero(nseg);
            for (int k = 0; k < nseg + (nseg ? 1 : 0); ++k) {
                out.t[k] = t[(size_t)k];
                out.obj[k] = obj[(size_t)k];
            }
            for (int k = 0; k < nseg; ++k) out.slope[k] = slope[(size_t)k];
            out.enter.assign(enter.begin(), enter.begin() + nseg);
            out.leave.assign(leave.begin(), leave.begin() + nseg);
        }
    };

    static IntegerResult blankIntegerResult(int status, int no) {
        IntegerResult out;
        out.status = status;
        out.x = nans(no);
        return out;
    }

    // The certificate methods: NaN vectors and the result's status, which stands unless the call reports a failure
    static Certificate blankCertificate(const View& p, int status) {
        Certificate out;
        out.farkas = nans(p.m);
        out.ray = nans(p.n);
        out.status = status;
        return out;
    }
    static bool hasCertificate(int status) { return status == LP_INFEASIBLE || status == LP_UNBOUNDED; }
    static void mergeStatus(Certificate& out, int st, lp_context* ctx) {
        if (checked(st, ctx) != LP_OPTIMAL) out.status = st;
    }

    // parametricRhs (dir = d, rows(A) entries) or parametricCost (dir = g, cols(A) entries)
    Parametric parametric(bool cost, const Result& r, const lpla::VectorXd& dir, double tMax) const {
        const View p = view();
        const std::string who = cost ? "Solver::parametricCost" : "Solver::parametricRhs";
        Parametric out;
        out.status = r.status;
        out.basis = r.basis;
        PathBuffers path;
        if (r.status == LP_OPTIMAL) {
            if ((int)r.basis.size() != p.m) throw std::invalid_argument(who + ": basis size != rows(A)");
            if ((int)dir.size() != (cost ? p.n : p.m))
                throw std::invalid_argument(who + (cost ? ": g size != cols(A)" : ": d size != rows(A)"));
            lp_context* ctx = lpgpu::context(_device);
            out.basis.assign((size_t)p.m, -1);
            out.status = checked((cost ? lp_basis_parametric_cost : lp_basis_parametric)(
                                     ctx, p.A, p.m, p.n, p.b, p.c, r.basis.data(), p.maximize, dir.data(), tMax, EPS,
                                     MAX_BREAKS, &path.nseg, path.t.data(), path.obj.data(), path.slope.data(),
                                     path.enter.data(), path.leave.data(), out.basis.data()), ctx);
        }
        path.unpack(out);
        return out;
    }

    BoundedParametric boundedParametric(bool cost, const std::vector<double>& lo, const std::vector<double>& hi,
                                        const BoundedResult& from, const lpla::VectorXd& dir, double tMax,
                                        bool large = false) const {
        const View p = view();
        requireBounds("Solver::boundedParametric", p, lo, hi);
        BoundedParametric out;
        out.status = from.status;
        out.basis = from.basis;
        out.atUpper = from.atUpper;
        PathBuffers path;
        std::vector<int> side(MAX_BREAKS + 1);
        if (from.status == LP_OPTIMAL) {
            requireStart("Solver::boundedParametric", "result", p, from);
            if ((int)dir.size() != (cost ? p.n : p.m))
                throw std::invalid_argument(cost ? "Solver::boundedParametricCost: g size != cols(A)"
                                                 : "Solver::boundedParametricRhs: d size != rows(A)");
            lp_context* ctx = lpgpu::context(_device);
            out.basis.assign((size_t)p.m, -1);
            out.atUpper.assign((size_t)p.n, 0);
            const auto entry = large ? (cost ? lp_basis_bounded_parametric_cost_large : lp_basis_bounded_parametric_large)
                                     : (cost ? lp_basis_bounded_parametric_cost : lp_basis_bounded_parametric);
            out.status = checked(entry(ctx, p.A, p.m, p.n, p.b, p.c, lo.data(), hi.data(), from.basis.data(),
                                       from.atUpper.data(), p.maximize, dir.data(), tMax, EPS, MAX_BREAKS, &path.nseg,
                                       path.t.data(), path.obj.data(), path.slope.data(), path.enter.data(),
                                       path.leave.data(), side.data(), out.basis.data(), out.atUpper.data()), ctx);
        }
        path.unpack(out);
        out.side.assign(side.begin(), side.begin() + path.nseg);
        return out;
    }

    // boundedDuals, or with large boundedDualsLarge
    BoundedDuals boundedDualsRun(const char* who, const std::vector<double>& lo, const std::vector<double>& hi,
                                 const BoundedResult& from, bool large) const {
        const View p = view();
        requireBounds(who, p, lo, hi);
        BoundedDuals out;
        out.x = lpla::VectorXd::Zero(p.n);
        out.y = lpla::VectorXd::Zero(p.m);
        out.d = lpla::VectorXd::Zero(p.n);
        out.status = from.status;
        if (from.status == LP_OPTIMAL) {
            requireStart(who, "result", p, from);
            lp_context* ctx = lpgpu::context(_device);
            const auto entry = large ? lp_basis_bounded_duals_large : lp_basis_bounded_duals;
            out.status = checked(entry(ctx, p.A, p.m, p.n, p.b, p.c, lo.data(), hi.data(), from.basis.data(),
                                       from.atUpper.data(), out.x.data(), out.y.data(), out.d.data(), &out.objective),
                                 ctx);
        }
        if (out.status != LP_OPTIMAL) {
            out.x = out.d = nans(p.n);
            out.y = nans(p.m);
            out.objective = kNaN;
        }
        return out;
    }

    // boundedCertificate, or with large boundedCertificateLarge
    Certificate boundedCertificateRun(const char* who, const std::vector<double>& lo, const std::vector<double>& hi,
                                      const BoundedResult& from, double eps, bool large) const {
        const View p = view();
        requireBounds(who, p, lo, hi);
        Certificate out = blankCertificate(p, from.status);
        if (hasCertificate(from.status)) {
            requireStart(who, "result", p, from);
            lp_context* ctx = lpgpu::context(_device);
            const auto entry = large ? lp_basis_bounded_certificate_large : lp_basis_bounded_certificate;
            mergeStatus(out, entry(ctx, p.A, p.m, p.n, p.b, p.c, lo.data(), hi.data(), from.basis.data(),
                                   from.atUpper.data(), p.maximize, eps, &out.kind, out.farkas.data(), out.ray.data(),
                                   &out.value, &out.index), ctx);
        }
        return out;
    }

    // boundedRanging, or with large boundedRangingLarge
    BoundedRanging boundedRangingRun(const char* who, const std::vector<double>& lo, const std::vector<double>& hi,
                                     const BoundedResult& from, bool large) const {
        const View p = view();
        requireBounds(who, p, lo, hi);
        RangingEnds ends(p.m, p.n);
        std::vector<int> rs(2 * (size_t)p.m, -1);
        BoundedRanging out;
        out.status = from.status;
        if (from.status == LP_OPTIMAL) {
            requireStart(who, "result", p, from);
            lp_context* ctx = lpgpu::context(_device);
            const auto entry = large ? lp_basis_bounded_ranging_large : lp_basis_bounded_ranging;
            out.status = checked(entry(ctx, p.A, p.m, p.n, p.b, p.c, lo.data(), hi.data(), from.basis.data(),
                                       from.atUpper.data(), p.maximize, EPS, ends.rhs.data(), ends.rv.data(), rs.data(),
                                       ends.cost.data(), ends.cv.data()), ctx);
        }
        ends.unpack(out);
        unpackPairs(out.status == LP_OPTIMAL, rs, -1, out.b_side_lo, out.b_side_hi);
        return out;
    }

    // boundedSimplex (from null) or boundedResolve, through the entry without a rule (rule null) or its _ex form;
    // large: boundedSimplexLarge, or with from boundedResolveLarge, the same way; dual (with from and rule): the
    // re-solve's _dual_ex form; ratio (with dual): its _ratio_ex form
    BoundedResult boundedRun(const char* who, const std::vector<double>& lo, const std::vector<double>& hi,
                             const BoundedResult* from, const PivotRule* rule, bool throw_on_failure,
                             bool large = false, const DualRule* dual = nullptr, const DualRatio* ratio = nullptr) const {
        const View p = view();
        requireBounds(who, p, lo, hi);
        if (from) requireStart(who, "start", p, *from);
        BoundedResult out;
        out.x = nans(p.no);
        out.basis.assign((size_t)p.m, -1);
        out.atUpper.assign((size_t)p.n, 0);
        lp_context* ctx = lpgpu::context(_device);
        if (from && rule && dual && ratio) {
            const auto entry = large ? lp_simplex_bounded_resolve_large_ratio_ex : lp_simplex_bounded_resolve_ratio_ex;
            out.status = entry(ctx, p.A, p.m, p.n, p.b, p.c, lo.data(), hi.data(), from->basis.data(),
                               from->atUpper.data(), p.maximize, p.no, EPS, MAX_ITER, out.x.data(), out.basis.data(),
                               out.atUpper.data(), &out.objective, out.iterations, (int)*rule, (int)*dual, (int)*ratio);
        } else if (from && rule && dual) {
            const auto entry = large ? lp_simplex_bounded_resolve_large_dual_ex : lp_simplex_bounded_resolve_dual_ex;
            out.status = entry(ctx, p.A, p.m, p.n, p.b, p.c, lo.data(), hi.data(), from->basis.data(),
                               from->atUpper.data(), p.maximize, p.no, EPS, MAX_ITER, out.x.data(), out.basis.data(),
                               out.atUpper.data(), &out.objective, out.iterations, (int)*rule, (int)*dual);
        } else if (large && from && rule)
            out.status = lp_simplex_bounded_resolve_large_ex(ctx, p.A, p.m, p.n, p.b, p.c, lo.data(), hi.data(),
                                                             from->basis.data(), from->atUpper.data(), p.maximize,
                                                             p.no, EPS, MAX_ITER, out.x.data(), out.basis.data(),
                                                             out.atUpper.data(), &out.objective, out.iterations,
                                                             (int)*rule);
        else if (large && rule)
            out.status = lp_simplex_bounded_large_ex(ctx, p.A, p.m, p.n, p.b, p.c, lo.data(), hi.data(), p.maximize,
                                                     p.no, EPS, MAX_ITER, out.x.data(), out.basis.data(),
                                                     out.atUpper.data(), &out.objective, out.iterations, (int)*rule);
        else if (large && from)
            out.status = lp_simplex_bounded_resolve_large(ctx, p.A, p.m, p.n, p.b, p.c, lo.data(), hi.data(),
                                                          from->basis.data(), from->atUpper.data(), p.maximize, p.no,
                                                          EPS, MAX_ITER, out.x.data(), out.basis.data(),
                                                          out.atUpper.data(), &out.objective, out.iterations);
        else if (large)
            out.status = lp_simplex_bounded_large(ctx, p.A, p.m, p.n, p.b, p.c, lo.data(), hi.data(), p.maximize, p.no,
                                                  EPS, MAX_ITER, out.x.data(), out.basis.data(), out.atUpper.data(),
                                                  &out.objective, out.iterations);
        else if (!from && !rule)
            out.status = lp_simplex_bounded(ctx, p.A, p.m, p.n, p.b, p.c, lo.data(), hi.data(), p.maximize, p.no, EPS,
                                            MAX_ITER, out.x.data(), out.basis.data(), out.atUpper.data(),
                                            &out.objective, out.iterations);
        else if (!from)
            out.status = lp_simplex_bounded_ex(ctx, p.A, p.m, p.n, p.b, p.c, lo.data(), hi.data(), p.maximize, p.no,
                                               EPS, MAX_ITER, out.x.data(), out.basis.data(), out.atUpper.data(),
                                               &out.objective, out.iterations, (int)*rule);
        else if (!rule)
            out.status = lp_simplex_bounded_resolve(ctx, p.A, p.m, p.n, p.b, p.c, lo.data(), hi.data(),
                                                    from->basis.data(), from->atUpper.data(), p.maximize, p.no, EPS,
                                                    MAX_ITER, out.x.data(), out.basis.data(), out.atUpper.data(),
                                                    &out.objective, out.iterations);
        else
            out.status = lp_simplex_bounded_resolve_ex(ctx, p.A, p.m, p.n, p.b, p.c, lo.data(), hi.data(),
                                                       from->basis.data(), from->atUpper.data(), p.maximize, p.no, EPS,
                                                       MAX_ITER, out.x.data(), out.basis.data(), out.atUpper.data(),
                                                       &out.objective, out.iterations, (int)*rule);
        if (throw_on_failure) lpgpu::throw_for_status(out.status, ctx);
        checked(out.status, ctx);
        return out;
    }

    // boundedBranchAndBound, or with large boundedBranchAndBoundLarge, from a result's basis and flags; snapshots >= 0
    // (large only): the _ex entry with that many snapshots; ratio: the _ratio_ex entries (large: snapshots as given, a
    // negative count refused by the entry)
    IntegerResult boundedSearch(const char* who, const std::vector<bool>& integer, const std::vector<double>& lo,
                                const std::vector<double>& hi, const BoundedResult& from, int maxDepth, int maxNodes,
                                bool large, int snapshots = -1, const DualRatio* ratio = nullptr) const {
        const View p = view();
        IntegerResult out = blankIntegerResult(from.status, p.no);
        if (from.status != LP_OPTIMAL) return out;
        if ((int)integer.size() != p.n) throw std::invalid_argument(std::string(who) + ": mask size != cols(A)");
        requireBounds(who, p, lo, hi);
        requireStart(who, "start", p, from);
        const std::vector<int> mask(integer.begin(), integer.end());
        lp_context* ctx = lpgpu::context(_device);
        int found = 0, stats[7] = {0, 0, 0, 0, 0, 0, 0};
        if (ratio && large) {
            out.status = checked(lp_mip_bounded_solve_large_ratio_ex(
                ctx, p.A, p.m, p.n, p.b, p.c, lo.data(), hi.data(), from.basis.data(), from.atUpper.data(), p.maximize,
                p.no, mask.data(), EPS, INT_TOL, MIP_GAP, maxDepth, maxNodes, MAX_ITER, out.x.data(), &out.objective,
                &out.bound, &found, stats, snapshots, (int)*ratio), ctx);
        } else if (ratio) {
            out.status = checked(lp_mip_bounded_solve_ratio_ex(
                ctx, p.A, p.m, p.n, p.b, p.c, lo.data(), hi.data(), from.basis.data(), from.atUpper.data(), p.maximize,
                p.no, mask.data(), EPS, INT_TOL, MIP_GAP, maxDepth, maxNodes, MAX_ITER, out.x.data(), &out.objective,
                &out.bound, &found, stats, (int)*ratio), ctx);
        } else if (large && snapshots >= 0) {
            out.status = checked(lp_mip_bounded_solve_large_ex(
                ctx, p.A, p.m, p.n, p.b, p.c, lo.data(), hi.data(), from.basis.data(), from.atUpper.data(), p.maximize,
                p.no, mask.data(), EPS, INT_TOL, MIP_GAP, maxDepth, maxNodes, MAX_ITER, out.x.data(), &out.objective,
                &out.bound, &found, stats, snapshots), ctx);
        } else {
            const auto entry = large ? lp_mip_bounded_solve_large : lp_mip_bounded_solve;
            out.status = checked(entry(ctx, p.A, p.m, p.n, p.b, p.c, lo.data(), hi.data(), from.basis.data(),
                                       from.atUpper.data(), p.maximize, p.no, mask.data(), EPS, INT_TOL, MIP_GAP,
                                       maxDepth, maxNodes, MAX_ITER, out.x.data(), &out.objective, &out.bound, &found,
                                       stats), ctx);
        }
        out.found = found != 0;
        out.nodes = stats[0];
        out.restored = stats[5];
        out.rebuilt = stats[6];
        return out;
    }

    Canonical _problem;  // deep copy, as in the reference (:285)
    int _device;
    PivotRule _rule = PivotRule::Dantzig;
};
