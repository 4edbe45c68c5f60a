// GPU tests of Solver::boundedParametricRhs and Solver::boundedParametricCost: after Solver::boundedSimplex they equal
// tests/ref/bounded_parametric_ref.c's bit for bit at two shapes and both senses (the library named by
// LP_BOUNDED_PARAMETRIC_REF, loaded at run time), as do lp_basis_bounded_parametric_batched and
// lp_basis_bounded_parametric_cost_batched on a batch of three LPs with a run status; a result that is not optimal
// keeps its status without segments, a repeated basis index is singular, crossed bounds are infeasible without
// segments, and a bad flag, index, size or a start that is not optimal throws std::invalid_argument.
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
static const int MB = Solver::MAX_BREAKS;

// [A0 | I] x = b with A0 > 0, k structural columns boxed in several ways (free above, boxed, fixed, a negative lower
// bound), costs of both signs; d (m) and g (n) are seeded directions of mixed signs.  Not fixtures.h's boxed_problem:
// d is drawn row by row between the draws of A and b, so the stream differs from the first row on.
static Canonical boxed_problem(uint64_t seed, int m, int k, bool maximize, MatrixXd* Aout, VectorXd* bout,
                               VectorXd* cout, std::vector<double>* lo, std::vector<double>* hi, VectorXd* d,
                               VectorXd* g) {
    uint64_t s = seed * 7919 + 31;
    const int n = k + m;
    MatrixXd A = MatrixXd::Zero(m, n);
    VectorXd b(m), c = VectorXd::Zero(n);
    *d = VectorXd::Zero(m);
    *g = VectorXd::Zero(n);
    for (int i = 0; i < m; ++i) {
        for (int j = 0; j < k; ++j) A(i, j) = 0.05 + u01(s);
        A(i, k + i) = 1.0;
        b[i] = 0.5 * k * (1.0 + u01(s));
        (*d)[i] = (2.0 * u01(s) - 1.0) * b[i];
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
    for (int j = 0; j < n; ++j) (*g)[j] = 2.0 * u01(s) - 1.0;
    std::vector<int> basis((size_t)m);
    for (int i = 0; i < m; ++i) basis[(size_t)i] = k + i;
    *Aout = A;
    *bout = b;
    *cout = c;
    Canonical can(A, b, c, basis, /*minimize=*/!maximize);
    can.SetOriginalVariablesCount(n);
    return can;
}

typedef int (*RefBoundedParametric)(const double*, int, int, const double*, const double*, const double*, const double*,
                                    const int*, const int*, int, const double*, double, double, int, int*, double*,
                                    double*, double*, int*, int*, int*, int*, int*);

// One reference path in the padded layout
struct RefPath {
    int status = -1, nseg = -7;
    std::vector<double> t, obj, slope;
    std::vector<int> enter, leave, side, basis, up;
    RefPath(RefBoundedParametric ref, const MatrixXd& A, const VectorXd& b, const VectorXd& c,
            const std::vector<double>& lo, const std::vector<double>& hi, const std::vector<int>& basis_in,
            const std::vector<int>& up_in, bool maximize, const VectorXd& dir, double tMax)
        : t(MB + 2), obj(MB + 2), slope(MB + 1), enter(MB + 1), leave(MB + 1), side(MB + 1), basis((size_t)A.rows()),
          up((size_t)A.cols()) {
        status = ref(A.data(), (int)A.rows(), (int)A.cols(), b.data(), c.data(), lo.data(), hi.data(), basis_in.data(),
                     up_in.data(), maximize ? 1 : 0, dir.data(), tMax, Solver::EPS, MB, &nseg, t.data(), obj.data(),
                     slope.data(), enter.data(), leave.data(), side.data(), basis.data(), up.data());
    }
};

// the mirror's path against the reference's; returns the number of breakpoints whose leaving variable stops at its upper
// bound, flips included
static int compare(const Solver::BoundedParametric& g, const RefPath& w) {
    CHECK(g.status == w.status);
    const int ns = w.nseg;
    CHECK((int)g.slope.size() == ns && (int)g.t.size() == (ns ? ns + 1 : 0) && (int)g.obj.size() == (ns ? ns + 1 : 0));
    CHECK((int)g.enter.size() == ns && (int)g.leave.size() == ns && (int)g.side.size() == ns);
    if ((int)g.slope.size() != ns || (int)g.side.size() != ns) return 0;
    int upper = 0;
    for (int k = 0; k < ns; ++k) {
        CHECK(same_bits(g.t[k], w.t[(size_t)k]) && same_bits(g.obj[k], w.obj[(size_t)k]));
        CHECK(same_bits(g.slope[k], w.slope[(size_t)k]));
        CHECK(g.enter[(size_t)k] == w.enter[(size_t)k] && g.leave[(size_t)k] == w.leave[(size_t)k]);
        CHECK(g.side[(size_t)k] == w.side[(size_t)k]);
        upper += g.side[(size_t)k] == 1;
    }
    if (ns) CHECK(same_bits(g.t[ns], w.t[(size_t)ns]) && same_bits(g.obj[ns], w.obj[(size_t)ns]));
    CHECK(g.basis == w.basis && g.atUpper == w.up);
    return upper;
}

TEST(BoundedParametric_SolverMatchesTheRef) {
    const RefLib lib("LP_BOUNDED_PARAMETRIC_REF");
    RefBoundedParametric rhs = lib.symbol<RefBoundedParametric>("ref_bounded_parametric");
    RefBoundedParametric cost = lib.symbol<RefBoundedParametric>("ref_bounded_parametric_cost");
    int paths = 0, breaks = 0, upper = 0;
    for (uint64_t seed = 0; seed < 12; ++seed) {
        const int m = seed % 2 ? 9 : 4, k = seed % 2 ? 14 : 7;   // two shapes
        const bool maximize = (seed / 2) % 2 == 0;
        MatrixXd A;
        VectorXd b, c, d, g;
        std::vector<double> lo, hi;
        Canonical p = boxed_problem(seed, m, k, maximize, &A, &b, &c, &lo, &hi, &d, &g);
        Solver s(p);
        const Solver::BoundedResult r = s.boundedSimplex(lo, hi, /*throw_on_failure=*/false);
        if (r.status != LP_OPTIMAL) continue;
        for (double tMax : {INF, 0.4}) {
            const Solver::BoundedParametric pr = s.boundedParametricRhs(lo, hi, r, d, tMax);
            upper += compare(pr, RefPath(rhs, A, b, c, lo, hi, r.basis, r.atUpper, maximize, d, tMax));
            const Solver::BoundedParametric pc = s.boundedParametricCost(lo, hi, r, g, tMax);
            upper += compare(pc, RefPath(cost, A, b, c, lo, hi, r.basis, r.atUpper, maximize, g, tMax));
            paths += 2;
            breaks += (int)pr.slope.size() + (int)pc.slope.size() - 2;
        }
    }
    CHECK(paths >= 40 && breaks >= 60 && upper >= 5);
}

TEST(BoundedParametric_CAbiBatchMatchesTheRef) {
    const RefLib lib("LP_BOUNDED_PARAMETRIC_REF");
    RefBoundedParametric refs[2] = {lib.symbol<RefBoundedParametric>("ref_bounded_parametric"),
                                    lib.symbol<RefBoundedParametric>("ref_bounded_parametric_cost")};
    lp_context* ctx = lpgpu::context(0);
    for (int shape = 0; shape < 2; ++shape) {
        const int m = shape ? 9 : 4, k = shape ? 14 : 7, n = k + m, B = 3;
        std::vector<double> A, b, c, lo, hi, d, g;
        std::vector<int> basis, up, run;
        std::vector<MatrixXd> As;
        std::vector<VectorXd> bs, cs, ds, gs;
        std::vector<std::vector<double>> los, his;
        std::vector<Solver::BoundedResult> rs;
        for (uint64_t seed = 20; (int)rs.size() < B; ++seed) {
            MatrixXd Ak;
            VectorXd bk, ck, dk, gk;
            std::vector<double> lk, hk;
            Canonical p = boxed_problem(seed, m, k, true, &Ak, &bk, &ck, &lk, &hk, &dk, &gk);
            Solver s(p);
            const Solver::BoundedResult r = s.boundedSimplex(lk, hk, false);
            if (r.status != LP_OPTIMAL) continue;
            As.push_back(Ak); bs.push_back(bk); cs.push_back(ck); ds.push_back(dk); gs.push_back(gk);
            los.push_back(lk); his.push_back(hk); rs.push_back(r);
            A.insert(A.end(), Ak.data(), Ak.data() + (size_t)m * n);
            b.insert(b.end(), bk.data(), bk.data() + m);
            c.insert(c.end(), ck.data(), ck.data() + n);
            d.insert(d.end(), dk.data(), dk.data() + m);
            g.insert(g.end(), gk.data(), gk.data() + n);
            lo.insert(lo.end(), lk.begin(), lk.end());
            hi.insert(hi.end(), hk.begin(), hk.end());
            basis.insert(basis.end(), r.basis.begin(), r.basis.end());
            up.insert(up.end(), r.atUpper.begin(), r.atUpper.end());
            run.push_back(rs.size() == 2 ? LP_INFEASIBLE : LP_OPTIMAL);   // the second LP is passed over
        }
        for (int path = 0; path < 2; ++path) {
            std::vector<int> nseg(B), enter(B * (MB + 1)), leave(B * (MB + 1)), side(B * (MB + 1)), bo(B * m),
                uo(B * n), st(B);
            std::vector<double> t(B * (MB + 2)), obj(B * (MB + 2)), slope(B * (MB + 1));
            const int rc = (path ? lp_basis_bounded_parametric_cost_batched : lp_basis_bounded_parametric_batched)(
                ctx, B, A.data(), m, n, b.data(), c.data(), lo.data(), hi.data(), basis.data(), up.data(), run.data(), 1,
                path ? g.data() : d.data(), INF, Solver::EPS, MB, nseg.data(), t.data(), obj.data(), slope.data(),
                enter.data(), leave.data(), side.data(), bo.data(), uo.data(), st.data());
            CHECK(rc == LP_OPTIMAL);
            for (int q = 0; q < B; ++q) {
                if (run[(size_t)q] != LP_OPTIMAL) {
                    CHECK(st[(size_t)q] == LP_INFEASIBLE && nseg[(size_t)q] == 0 && std::isnan(t[(size_t)q * (MB + 2)]));
                    CHECK(side[(size_t)q * (MB + 1)] == -1 && bo[(size_t)q * m] == rs[(size_t)q].basis[0]);
                    continue;
                }
                const RefPath w(refs[path], As[(size_t)q], bs[(size_t)q], cs[(size_t)q], los[(size_t)q], his[(size_t)q],
                                rs[(size_t)q].basis, rs[(size_t)q].atUpper, true, path ? gs[(size_t)q] : ds[(size_t)q],
                                INF);
                CHECK(st[(size_t)q] == w.status && nseg[(size_t)q] == w.nseg);
                for (int j = 0; j < MB + 2; ++j) {
                    CHECK(same_bits(t[(size_t)q * (MB + 2) + j], w.t[(size_t)j]));
                    CHECK(same_bits(obj[(size_t)q * (MB + 2) + j], w.obj[(size_t)j]));
                }
                for (int j = 0; j < MB + 1; ++j) {
                    const size_t o = (size_t)q * (MB + 1) + j;
                    CHECK(same_bits(slope[o], w.slope[(size_t)j]) && enter[o] == w.enter[(size_t)j]);
                    CHECK(leave[o] == w.leave[(size_t)j] && side[o] == w.side[(size_t)j]);
                }
                for (int i = 0; i < m; ++i) CHECK(bo[(size_t)q * m + i] == w.basis[(size_t)i]);
                for (int j = 0; j < n; ++j) CHECK(uo[(size_t)q * n + j] == w.up[(size_t)j]);
            }
        }
        CHECK(lp_basis_bounded_parametric_fits(m, n) == 1 && lp_basis_bounded_parametric_cost_fits(m, n) == 1);
    }
    CHECK(lp_basis_bounded_parametric_fits(200, 400) == 0 && lp_basis_bounded_parametric_cost_fits(200, 400) == 0);
}

TEST(BoundedParametric_StatusesAndExceptions) {
    MatrixXd A;
    VectorXd b, c, d, g;
    std::vector<double> lo, hi;
    Canonical p = boxed_problem(2, 4, 7, true, &A, &b, &c, &lo, &hi, &d, &g);
    const int n = 11;
    Solver s(p);
    const Solver::BoundedResult r = s.boundedSimplex(lo, hi, /*throw_on_failure=*/false);
    CHECK(r.status == LP_OPTIMAL);
    const Solver::BoundedParametric ok = s.boundedParametricRhs(lo, hi, r, d, 0.25);
    CHECK(ok.status == LP_OPTIMAL && ok.slope.size() >= 1 && ok.t[(int)ok.slope.size()] == 0.25);
    CHECK(ok.enter.back() == -1 && ok.leave.back() == -1 && ok.side.back() == -1);
    Solver::BoundedResult failed = r;
    failed.status = LP_UNBOUNDED;   // a result that is not optimal keeps its status and gets no segments
    const Solver::BoundedParametric none = s.boundedParametricCost(lo, hi, failed, g, INF);
    CHECK(none.status == LP_UNBOUNDED && none.t.size() == 0 && none.slope.size() == 0 && none.side.empty());
    CHECK(none.basis == r.basis && none.atUpper == r.atUpper);
    Solver::BoundedResult rep = r;
    rep.basis[1] = rep.basis[0];    // repeated index: singular, the given basis and flags back
    const Solver::BoundedParametric e = s.boundedParametricRhs(lo, hi, rep, d, INF);
    CHECK(e.status == LP_SINGULAR && e.slope.size() == 0 && e.basis == rep.basis && e.atUpper == rep.atUpper);
    std::vector<double> crossed = hi;
    crossed[3] = lo[3] - 1.0;       // crossed bounds: infeasible without segments, nothing thrown
    const Solver::BoundedParametric x = s.boundedParametricCost(lo, crossed, r, g, INF);
    CHECK(x.status == LP_INFEASIBLE && x.t.size() == 0);
    Solver::BoundedResult bad = r;
    bad.basis[1] = 1000;            // out of range
    CHECK_THROWS(s.boundedParametricRhs(lo, hi, bad, d, INF), std::invalid_argument);
    bad = r;
    bad.atUpper[0] = 1;             // column 0 has no upper bound
    CHECK(hi[0] == INF);
    CHECK_THROWS(s.boundedParametricCost(lo, hi, bad, g, INF), std::invalid_argument);
    CHECK_THROWS(s.boundedParametricRhs(lo, hi, r, d, -1.0), std::invalid_argument);
    CHECK_THROWS(s.boundedParametricRhs(lo, hi, r, g, INF), std::invalid_argument);    // g has n entries, d needs m
    CHECK_THROWS(s.boundedParametricCost(lo, hi, r, d, INF), std::invalid_argument);
    std::vector<double> few(lo.begin(), lo.begin() + n - 1);
    CHECK_THROWS(s.boundedParametricRhs(few, hi, r, d, INF), std::invalid_argument);
    bad = r;
    bad.basis.pop_back();
    CHECK_THROWS(s.boundedParametricCost(lo, hi, bad, g, INF), std::invalid_argument);
    Solver::BoundedResult slack = r;   // the slack basis without flags is not optimal at t = 0: re-solve first
    for (int i = 0; i < 4; ++i) slack.basis[(size_t)i] = 7 + i;
    slack.atUpper.assign((size_t)n, 0);
    bool differs = slack.basis != r.basis;
    CHECK(differs);
    if (differs) CHECK_THROWS(s.boundedParametricRhs(lo, hi, slack, d, INF), std::invalid_argument);
}

int main(int argc, char** argv) { return run_all(argc > 1 ? argv[1] : nullptr); }
