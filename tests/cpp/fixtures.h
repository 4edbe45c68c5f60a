// What the Solver test programs share: the random stream, the exact comparisons, the C restatements under tests/ref
// loaded at run time, and the two families of seeded LPs.  A generator here draws from its stream in a fixed order;
// the constants its users differ in are parameters, and a user that draws more or in another order keeps its own.
#pragma once
#include <dlfcn.h>

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "check.h"
#include "Canonical.h"

inline double u01(uint64_t& s) {   // splitmix64
    uint64_t z = (s += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    z ^= z >> 31;
    return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}

// Against a restatement run in the same process: the same bits, any NaN equal to any NaN.
inline bool same_bits(double a, double b) {
    if (std::isnan(a) || std::isnan(b)) return std::isnan(a) && std::isnan(b);
    uint64_t x, y;
    std::memcpy(&x, &a, 8);
    std::memcpy(&y, &b, 8);
    return x == y;
}

// Against a golden file: the same bits, or zeros of either sign.
inline bool same_bits_or_zeros(double a, double b) {
    uint64_t x, y;
    std::memcpy(&x, &a, 8);
    std::memcpy(&y, &b, 8);
    return x == y || (a == 0.0 && b == 0.0);
}

inline bool same_value(double a, double b) { return (std::isnan(a) && std::isnan(b)) || a == b; }

// The library of a restatement, named by an environment variable the runner sets; every step is CHECKed.
class RefLib {
public:
    explicit RefLib(const char* env) {
        const char* path = std::getenv(env);
        CHECK(path != nullptr);
        h_ = dlopen(path, RTLD_NOW | RTLD_LOCAL);
        CHECK(h_ != nullptr);
    }
    RefLib(const RefLib&) = delete;
    RefLib& operator=(const RefLib&) = delete;
    ~RefLib() { dlclose(h_); }
    template <class Fn>
    Fn symbol(const char* name) const {
        Fn fn = reinterpret_cast<Fn>(dlsym(h_, name));
        CHECK(fn != nullptr);
        return fn;
    }

private:
    void* h_ = nullptr;
};

// (A, b, c) with the last rows(A) columns as the basis and every column an original variable
inline Canonical last_columns_basic(const lpla::MatrixXd& A, const lpla::VectorXd& b, const lpla::VectorXd& c,
                                    bool maximize) {
    const int m = (int)A.rows(), n = (int)A.cols();
    std::vector<int> basis((size_t)m);
    for (int i = 0; i < m; ++i) basis[(size_t)i] = n - m + i;
    Canonical can(A, b, c, basis, /*minimize=*/!maximize);
    can.SetOriginalVariablesCount(n);
    return can;
}

// min c.x, A0 x >= b, x >= 0 as [A0 | -I]: k originals, m surplus columns (the basis, which the two-phase flow ignores
// and which is dual feasible); c > 0 on the originals, b in [1, 1 + b_spread).  A, b and c also go to the pointers
// that are not null.
inline Canonical min_problem(uint64_t seed, int m, int k, lpla::MatrixXd* Aout = nullptr, lpla::VectorXd* bout = nullptr,
                             lpla::VectorXd* cout = nullptr, double b_spread = 1.0) {
    uint64_t s = seed * 7919 + 17;
    lpla::MatrixXd A = lpla::MatrixXd::Zero(m, k + m);
    lpla::VectorXd b(m), c = lpla::VectorXd::Zero(k + m);
    for (int i = 0; i < m; ++i) {
        for (int j = 0; j < k; ++j) A(i, j) = u01(s);
        A(i, k + i) = -1.0;
        b[i] = 1.0 + b_spread * u01(s);
    }
    for (int j = 0; j < k; ++j) c[j] = 0.1 + u01(s);
    if (Aout) *Aout = A;
    if (bout) *bout = b;
    if (cout) *cout = c;
    return last_columns_basic(A, b, c, /*maximize=*/false);
}

// [A0 | I] x = b with A0 >= a_offset, k structural columns boxed in several ways (free above, boxed, fixed, a negative
// lower bound), costs of both signs, b_i in b_scale * k * [1, 2); the slack basis.  A, b and c also go to the
// pointers that are not null.
inline Canonical boxed_problem(uint64_t seed, int m, int k, bool maximize, lpla::MatrixXd* Aout, lpla::VectorXd* bout,
                               lpla::VectorXd* cout, std::vector<double>* lo, std::vector<double>* hi,
                               double a_offset = 0.0, double b_scale = 0.5) {
    uint64_t s = seed * 7919 + 29;
    const int n = k + m;
    lpla::MatrixXd A = lpla::MatrixXd::Zero(m, n);
    lpla::VectorXd b(m), c = lpla::VectorXd::Zero(n);
    for (int i = 0; i < m; ++i) {
        for (int j = 0; j < k; ++j) A(i, j) = a_offset + u01(s);
        A(i, k + i) = 1.0;
        b[i] = b_scale * k * (1.0 + u01(s));
    }
    lo->assign((size_t)n, 0.0);
    hi->assign((size_t)n, std::numeric_limits<double>::infinity());
    for (int j = 0; j < k; ++j) {
        c[j] = u01(s) - 0.3;
        switch (j % 4) {
            case 1: (*hi)[(size_t)j] = 0.2 + 2.0 * u01(s); break;
            case 2: (*lo)[(size_t)j] = (*hi)[(size_t)j] = u01(s); break;
            case 3: (*lo)[(size_t)j] = -u01(s); (*hi)[(size_t)j] = 1.0 + u01(s); break;
            default: break;
        }
    }
    if (Aout) *Aout = A;
    if (bout) *bout = b;
    if (cout) *cout = c;
    return last_columns_basic(A, b, c, maximize);
}
