// GPU tests of Solver::setPivotRule(PivotRule::Devex): solve() and twoPhaseSimplex() give, bit for bit, what
// tests/ref/devex_ref.c recorded in tests/golden/devex_cases.json (the file named by LP_DEVEX_GOLDEN).
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>

#include "check.h"
#include "fixtures.h"
#include "Canonical.h"
#include "Common.h"
#include "SimplexSolover.h"

using lpla::MatrixXd;
using lpla::VectorXd;

struct Case {
    std::string name;
    int two_phase = 0, maximize = 0, m = 0, n = 0, n_orig = 0, status = 0;
    std::vector<double> A, b, c, x, iters, basis, basis_out;   // A row-major m x n
    double obj = 0.0;
};

// The value of "key" inside the JSON object text `s`: a number, or an array of numbers (python's repr of a double
// reads back exactly through strtod).
static std::vector<double> numbers(const std::string& s, const char* key) {
    const std::string pat = std::string("\"") + key + "\":";
    size_t p = s.find(pat);
    CHECK(p != std::string::npos);
    p += pat.size();
    while (s[p] == ' ') ++p;
    std::vector<double> out;
    if (s[p] != '[') {
        out.push_back(std::strtod(s.c_str() + p, nullptr));
        return out;
    }
    ++p;
    for (;;) {
        while (s[p] == ' ' || s[p] == ',') ++p;
        if (s[p] == ']') break;
        char* end = nullptr;
        out.push_back(std::strtod(s.c_str() + p, &end));
        p = (size_t)(end - s.c_str());
    }
    return out;
}

static std::vector<Case> load_cases() {
    const char* path = std::getenv("LP_DEVEX_GOLDEN");
    CHECK(path != nullptr);
    std::ifstream f(path);
    CHECK(f.good());
    std::stringstream ss;
    ss << f.rdbuf();
    const std::string all = ss.str();
    std::vector<Case> cases;
    for (size_t p = all.find("{\"name\""); p != std::string::npos;) {   // one object per case, no nesting
        const size_t q = all.find("{\"name\"", p + 1);
        const std::string s = all.substr(p, q == std::string::npos ? std::string::npos : q - p);
        Case k;
        const size_t n0 = s.find('"', 8) + 1;
        k.name = s.substr(n0, s.find('"', n0) - n0);
        k.two_phase = (int)numbers(s, "two_phase")[0];
        k.maximize = (int)numbers(s, "maximize")[0];
        k.m = (int)numbers(s, "m")[0];
        k.n = (int)numbers(s, "n")[0];
        k.n_orig = (int)numbers(s, "n_orig")[0];
        k.status = (int)numbers(s, "status")[0];
        k.A = numbers(s, "A");
        k.b = numbers(s, "b");
        k.c = numbers(s, "c");
        k.basis = numbers(s, "basis");
        k.iters = numbers(s, "iters");
        k.basis_out = numbers(s, "basis_out");
        k.x = numbers(s, "x");
        k.obj = numbers(s, "obj")[0];
        CHECK((int)k.A.size() == k.m * k.n && (int)k.b.size() == k.m && (int)k.c.size() == k.n && k.iters.size() == 3);
        cases.push_back(k);
        p = q;
    }
    return cases;
}

static Canonical canonical(const Case& k) {
    MatrixXd A(k.m, k.n);
    for (int i = 0; i < k.m; ++i)
        for (int j = 0; j < k.n; ++j) A(i, j) = k.A[(size_t)i * k.n + j];
    VectorXd b(k.m), c(k.n);
    for (int i = 0; i < k.m; ++i) b[i] = k.b[(size_t)i];
    for (int j = 0; j < k.n; ++j) c[j] = k.c[(size_t)j];
    std::vector<int> basis((size_t)k.m);
    for (int i = 0; i < k.m; ++i) basis[(size_t)i] = k.two_phase ? k.n - k.m + i : (int)k.basis[(size_t)i];   // (ignored by the two-phase flow)
    Canonical can(A, b, c, basis, /*minimize=*/!k.maximize);
    can.SetOriginalVariablesCount(k.n_orig);
    return can;
}

static void check_result(const Case& k, const Solver::Result& r) {
    CHECK(r.status == k.status);
    CHECK((int)r.basis.size() == k.m);
    for (int i = 0; i < k.m; ++i) CHECK(r.basis[(size_t)i] == (int)k.basis_out[(size_t)i]);
    if (k.status != LP_OPTIMAL) return;
    CHECK((int)r.x.size() == k.n_orig && (int)k.x.size() == k.n_orig);
    for (int j = 0; j < k.n_orig; ++j) CHECK(same_bits_or_zeros(r.x[j], k.x[(size_t)j]));
    CHECK(same_bits_or_zeros(r.objective, k.obj));
}

TEST(Devex_Solve) {
    int ran = 0;
    for (const Case& k : load_cases()) {
        if (k.two_phase) continue;
        Solver s(canonical(k));
        CHECK(s.pivotRule() == Solver::PivotRule::Dantzig);
        s.setPivotRule(Solver::PivotRule::Devex);
        CHECK(s.pivotRule() == Solver::PivotRule::Devex);
        auto r = s.solve_ex(false);
        std::printf("  %s: status %d, %d pivots\n", k.name.c_str(), r.status, r.iterations);
        check_result(k, r);
        CHECK(r.iterations == (int)k.iters[2]);
        if (k.status == LP_OPTIMAL) {
            VectorXd x = s.solve();
            for (int j = 0; j < k.n_orig; ++j) CHECK(same_bits_or_zeros(x[j], k.x[(size_t)j]));
        } else {
            CHECK_THROWS(s.solve(), std::runtime_error);
        }
        ++ran;
    }
    CHECK(ran >= 4);
}

TEST(Devex_TwoPhase) {
    int ran = 0, drove_out = 0;
    for (const Case& k : load_cases()) {
        if (!k.two_phase) continue;
        Solver s(canonical(k));
        s.setPivotRule(Solver::PivotRule::Devex);
        int it[3] = {0, 0, 0};
        auto r = s.twoPhaseSimplex_ex(false, it);
        std::printf("  %s: status %d, pivots %d + %d + %d\n", k.name.c_str(), r.status, it[0], it[1], it[2]);
        check_result(k, r);
        for (int q = 0; q < 3; ++q) CHECK(it[q] == (int)k.iters[(size_t)q]);
        CHECK(r.iterations == it[0] + it[1] + it[2]);
        if (k.status != LP_OPTIMAL) CHECK_THROWS(s.twoPhaseSimplex(), std::runtime_error);
        drove_out += it[1] > 0;
        ++ran;
    }
    CHECK(ran >= 4 && drove_out >= 1);
}

TEST(Devex_LeavesDantzigAlone) {
    for (const Case& k : load_cases()) {
        if (k.two_phase || k.status != LP_OPTIMAL) continue;
        Solver d(canonical(k)), x(canonical(k));
        x.setPivotRule(Solver::PivotRule::Devex);
        auto rd = d.solve_ex(false), rx = x.solve_ex(false);
        if (rd.status != LP_OPTIMAL) continue;   // (Beale's LP: Dantzig's rule cycles)
        CHECK(std::fabs(rd.objective - rx.objective) <= 1e-9 * std::fabs(rd.objective));
    }
}

int main(int argc, char** argv) { return run_all(argc > 1 ? argv[1] : nullptr); }
