// GPU tests of the Solver::boundedSimplexLarge and Solver::boundedResolveLarge overloads that take a pivot rule, against
// tests/golden/bounded_large_rules_cases.json (the file named by LP_BOUNDED_LARGE_RULES_GOLDEN, written from
// tests/ref/bounded_rules_ref.c by tests/golden/make_bounded_large_rules_golden.py): PivotRule::Bland finishes the
// cycling boxed LP that the form without a rule leaves at the iteration limit, PivotRule::Devex equals the recorded
// result on a 160 x 320 boxed LP bit for bit, PivotRule::Dantzig equals the form without a rule, and the re-solve
// takes a rule in its primal loop.  (No test_ prefix: tests/test_bounded_large_rules_cpp.py runs this program.)
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <fstream>
#include <limits>
#include <sstream>

#include "check.h"
#include "fixtures.h"
#include "Canonical.h"
#include "SimplexSolover.h"

using lpla::MatrixXd;
using lpla::VectorXd;
typedef Solver::PivotRule Rule;

// The value of "key" inside the JSON object text `s`: a number, or an array of numbers.
static std::vector<double> numbers(const std::string& s, const char* key) {
    const std::string pat = std::string("\"") + key + "\":";
    size_t p = s.find(pat);
    CHECK(p != std::string::npos);
    if (p == std::string::npos) return {};
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

static std::string golden() {
    const char* path = std::getenv("LP_BOUNDED_LARGE_RULES_GOLDEN");
    CHECK(path != nullptr);
    if (!path) return "";
    std::ifstream f(path);
    CHECK(f.good());
    std::stringstream ss;
    ss << f.rdbuf();
    return ss.str();
}

// r against the recorded result under `prefix` (status, iters, obj, x, basis, at_upper)
static void check_recorded(const Solver::BoundedResult& r, const std::string& g, const std::string& prefix, int m, int n) {
    auto get = [&](const char* key) { return numbers(g, (prefix + key).c_str()); };
    const std::vector<double> x = get("x"), basis = get("basis"), up = get("at_upper"), iters = get("iters");
    CHECK((int)x.size() == n && (int)basis.size() == m && (int)up.size() == n && iters.size() == 4);
    if ((int)x.size() != n || (int)basis.size() != m || (int)up.size() != n || iters.size() != 4) return;
    CHECK(r.status == (int)get("status")[0] && r.status == LP_OPTIMAL);
    CHECK(same_bits_or_zeros(r.objective, get("obj")[0]));
    CHECK((int)r.x.size() == n && (int)r.basis.size() == m && (int)r.atUpper.size() == n);
    if ((int)r.x.size() != n || (int)r.basis.size() != m || (int)r.atUpper.size() != n) return;
    for (int j = 0; j < n; ++j)
        CHECK(same_bits_or_zeros(r.x[j], x[(size_t)j]) && r.atUpper[(size_t)j] == (int)up[(size_t)j]);
    for (int t = 0; t < m; ++t) CHECK(r.basis[(size_t)t] == (int)basis[(size_t)t]);
    for (int q = 0; q < 4; ++q) CHECK(r.iterations[q] == (int)iters[(size_t)q]);
}

static bool same_result(const Solver::BoundedResult& a, const Solver::BoundedResult& b) {
    if (a.status != b.status || a.basis != b.basis || a.atUpper != b.atUpper || a.x.size() != b.x.size()) return false;
    for (int q = 0; q < 4; ++q)
        if (a.iterations[q] != b.iterations[q]) return false;
    for (int j = 0; j < (int)a.x.size(); ++j)
        if (!same_bits(a.x[j], b.x[j])) return false;
    return same_bits(a.objective, b.objective);
}

TEST(BoundedSimplexLarge_BlandFinishesTheCyclingLp) {
    const std::string g = golden();
    if (g.empty()) return;
    const int m = (int)numbers(g, "cyc_m")[0], n = (int)numbers(g, "cyc_n")[0], k = n - m;
    const std::vector<double> A0 = numbers(g, "cyc_A0"), b0 = numbers(g, "cyc_b"), c0 = numbers(g, "cyc_c0");
    CHECK((int)A0.size() == m * k && (int)b0.size() == m && (int)c0.size() == k);
    if ((int)A0.size() != m * k || (int)b0.size() != m || (int)c0.size() != k) return;
    MatrixXd A = MatrixXd::Zero(m, n);
    VectorXd b(m), c = VectorXd::Zero(n);
    for (int i = 0; i < m; ++i) {
        for (int j = 0; j < k; ++j) A(i, j) = A0[(size_t)i * k + j];
        A(i, k + i) = 1.0;
        b[i] = b0[(size_t)i];
    }
    for (int j = 0; j < k; ++j) c[j] = c0[(size_t)j];
    const std::vector<double> lo((size_t)n, 0.0), hi((size_t)n, numbers(g, "cyc_hi")[0]);
    Solver s(last_columns_basic(A, b, c, /*maximize=*/true));
    // without a rule, and under Dantzig's: the iteration limit in phase II
    const Solver::BoundedResult plain = s.boundedSimplexLarge(lo, hi, false);
    CHECK(plain.status == LP_ITER_LIMIT && plain.iterations[2] == Solver::MAX_ITER);
    CHECK_THROWS(s.boundedSimplexLarge(lo, hi), std::runtime_error);
    CHECK(same_result(s.boundedSimplexLarge(lo, hi, Rule::Dantzig, false), plain));
    const Solver::BoundedResult bl = s.boundedSimplexLarge(lo, hi, Rule::Bland);
    std::printf("  Bland: status %d, iterations %d + %d + %d, %d flips\n", bl.status, bl.iterations[0], bl.iterations[1],
                bl.iterations[2], bl.iterations[3]);
    check_recorded(bl, g, "cyc_", m, n);
    // the shape fits LDS too: the same result there
    CHECK(same_result(bl, s.boundedSimplex(lo, hi, Rule::Bland)));
    // the form without a rule ignores setPivotRule
    s.setPivotRule(Rule::Bland);
    CHECK(same_result(s.boundedSimplexLarge(lo, hi, false), plain));
}

TEST(BoundedSimplexLarge_DevexMatchesTheGolden) {
    const std::string g = golden();
    if (g.empty()) return;
    const int seed = (int)numbers(g, "dev_seed")[0], m = (int)numbers(g, "dev_m")[0], k = (int)numbers(g, "dev_k")[0];
    const int n = m + k;
    const bool maximize = numbers(g, "dev_maximize")[0] != 0.0;
    CHECK(m == 160 && n == 320 && lp_simplex_bounded_fits(m, n) == 0);
    std::vector<double> lo, hi;
    Solver s(boxed_problem((uint64_t)seed, m, k, maximize, nullptr, nullptr, nullptr, &lo, &hi, /*a_offset=*/0.0,
                           /*b_scale=*/0.125));
    const Solver::BoundedResult dv = s.boundedSimplexLarge(lo, hi, Rule::Devex);
    std::printf("  Devex: status %d, iterations %d + %d + %d, %d flips\n", dv.status, dv.iterations[0], dv.iterations[1],
                dv.iterations[2], dv.iterations[3]);
    check_recorded(dv, g, "dev_", m, n);
    // Dantzig's rule is the form without a rule, and another path than Devex
    const Solver::BoundedResult plain = s.boundedSimplexLarge(lo, hi);
    CHECK(same_result(s.boundedSimplexLarge(lo, hi, Rule::Dantzig), plain));
    CHECK(plain.iterations[0] != dv.iterations[0]);
    // the LDS form still refuses this shape under a rule
    CHECK_THROWS(s.boundedSimplex(lo, hi, Rule::Devex, false), std::invalid_argument);
    // the re-solve after a cost change, under each rule: the primal loop from the optimal basis
    {
        MatrixXd A;
        VectorXd b, c;
        boxed_problem((uint64_t)seed, m, k, maximize, &A, &b, &c, &lo, &hi, 0.0, 0.125);
        for (int j = 0; j < k; j += 7) c[j] = -c[j];
        Solver t(last_columns_basic(A, b, c, maximize));
        const Solver::BoundedResult w0 = t.boundedResolveLarge(lo, hi, plain);
        CHECK(w0.status == LP_OPTIMAL && w0.iterations[0] == 0 && w0.iterations[1] > 0);
        CHECK(same_result(t.boundedResolveLarge(lo, hi, plain, Rule::Dantzig), w0));
        for (Rule rule : {Rule::Bland, Rule::Devex}) {
            const Solver::BoundedResult w = t.boundedResolveLarge(lo, hi, plain, rule);
            CHECK(w.status == LP_OPTIMAL && w.iterations[0] == 0 && w.iterations[1] > 0);
            CHECK(!std::isnan(w.objective) && (int)w.x.size() == n);
        }
    }
}

int main(int argc, char** argv) { return run_all(argc > 1 ? argv[1] : nullptr); }
