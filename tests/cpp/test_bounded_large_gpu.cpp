// GPU tests of Solver::boundedSimplexLarge: on a 160 x 320 boxed LP (beyond lp_simplex_bounded_fits) the result equals,
// bit for bit, what tests/ref/bounded_ref.c recorded in tests/golden/bounded_large_case.json (the file named by
// LP_BOUNDED_LARGE_GOLDEN; tests/golden/make_bounded_large_golden.py restates large_problem below); an infeasible and
// an unbounded LP throw unless asked not to, and bad bounds throw std::invalid_argument.
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <limits>
#include <sstream>

#include "check.h"
#include "fixtures.h"
#include "Canonical.h"
#include "SimplexSolover.h"

using lpla::MatrixXd;
using lpla::VectorXd;

static const double INF = std::numeric_limits<double>::infinity();

// fixtures.h's boxed problem with b_i in 0.125 k [1, 2), as tests/golden/make_bounded_large_golden.py restates it
static Canonical large_problem(uint64_t seed, int m, int k, bool maximize, std::vector<double>* lo,
                               std::vector<double>* hi) {
    return boxed_problem(seed, m, k, maximize, nullptr, nullptr, nullptr, lo, hi, /*a_offset=*/0.0, /*b_scale=*/0.125);
}

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

TEST(BoundedSimplexLarge_MatchesTheGolden) {
    const char* path = std::getenv("LP_BOUNDED_LARGE_GOLDEN");
    CHECK(path != nullptr);
    if (!path) return;
    std::ifstream f(path);
    CHECK(f.good());
    std::stringstream ss;
    ss << f.rdbuf();
    const std::string g = ss.str();
    const int seed = (int)numbers(g, "seed")[0], m = (int)numbers(g, "m")[0], k = (int)numbers(g, "k")[0], n = m + k;
    const bool maximize = numbers(g, "maximize")[0] != 0.0;
    const std::vector<double> x = numbers(g, "x"), basis = numbers(g, "basis"), up = numbers(g, "at_upper"),
                              iters = numbers(g, "iters");
    CHECK(m == 160 && n == 320 && lp_simplex_bounded_fits(m, n) == 0);
    CHECK((int)x.size() == n && (int)basis.size() == m && (int)up.size() == n && iters.size() == 4);
    if ((int)x.size() != n || (int)basis.size() != m || (int)up.size() != n || iters.size() != 4) return;
    CHECK(iters[0] > 0 && iters[2] > 0 && iters[3] > 0);
    std::vector<double> lo, hi;
    Solver s(large_problem((uint64_t)seed, m, k, maximize, &lo, &hi));
    const Solver::BoundedResult r = s.boundedSimplexLarge(lo, hi);
    std::printf("  status %d, iterations %d + %d + %d, %d flips\n", r.status, r.iterations[0], r.iterations[1],
                r.iterations[2], r.iterations[3]);
    CHECK(r.status == (int)numbers(g, "status")[0] && r.status == LP_OPTIMAL);
    CHECK(same_bits_or_zeros(r.objective, numbers(g, "obj")[0]));
    CHECK((int)r.x.size() == n && (int)r.basis.size() == m && (int)r.atUpper.size() == n);
    for (int j = 0; j < n; ++j)
        CHECK(same_bits_or_zeros(r.x[j], x[(size_t)j]) && r.atUpper[(size_t)j] == (int)up[(size_t)j]);
    for (int t = 0; t < m; ++t) CHECK(r.basis[(size_t)t] == (int)basis[(size_t)t]);
    for (int q = 0; q < 4; ++q) CHECK(r.iterations[q] == (int)iters[(size_t)q]);
    // the LDS entry still refuses this shape
    CHECK_THROWS(s.boundedSimplex(lo, hi, false), std::invalid_argument);
}

TEST(BoundedSimplexLarge_ExceptionMapping) {
    const int m = 160, k = 160, n = m + k;
    std::vector<double> lo, hi;
    Canonical p = large_problem(3, m, k, true, &lo, &hi);
    Solver s(p);
    // infeasible: hi < lo on one column (no iteration), and a column fixed far above what the rows allow (phase I)
    std::vector<double> crossed = hi;
    crossed[1] = lo[1] - 1.0;
    const Solver::BoundedResult g = s.boundedSimplexLarge(lo, crossed, false);
    CHECK(g.status == LP_INFEASIBLE && std::isnan(g.objective));
    for (int q = 0; q < 4; ++q) CHECK(g.iterations[q] == 0);
    CHECK_THROWS(s.boundedSimplexLarge(lo, crossed), std::runtime_error);
    std::vector<double> lo2 = lo, hi2 = hi;
    lo2[0] = hi2[0] = 1e6;
    const Solver::BoundedResult h = s.boundedSimplexLarge(lo2, hi2, false);
    CHECK(h.status == LP_INFEASIBLE && std::isnan(h.objective) && std::isnan(h.x[0]));
    CHECK_THROWS(s.boundedSimplexLarge(lo2, hi2), std::runtime_error);
    // unbounded: a free-upwards column that no row holds, with an improving cost
    {
        MatrixXd A = p.GetConstraintsMatrix();
        VectorXd c = p.GetObjectiveCoefficients();
        for (int i = 0; i < m; ++i) A(i, 0) = 0.0;
        c[0] = 1.0;
        std::vector<int> basis((size_t)m);
        for (int i = 0; i < m; ++i) basis[(size_t)i] = k + i;
        Canonical q(A, p.GetRightHandSide(), c, basis, /*minimize=*/false);
        q.SetOriginalVariablesCount(n);
        Solver u(q);
        std::vector<double> lo3 = lo, hi3 = hi;
        lo3[0] = 0.0;
        hi3[0] = INF;
        const Solver::BoundedResult w = u.boundedSimplexLarge(lo3, hi3, false);
        CHECK(w.status == LP_UNBOUNDED && std::isnan(w.objective));
        CHECK_THROWS(u.boundedSimplexLarge(lo3, hi3), std::runtime_error);
    }
    std::vector<double> free_lo = lo;
    free_lo[1] = -INF;
    CHECK_THROWS(s.boundedSimplexLarge(free_lo, hi, false), std::invalid_argument);
    CHECK_THROWS(s.boundedSimplexLarge(std::vector<double>(3, 0.0), hi), std::invalid_argument);
}

int main(int argc, char** argv) { return run_all(argc > 1 ? argv[1] : nullptr); }
