// batched_bounded_resolve_body.hpp — the body of k_batched_bounded_resolve<NT> and of its rule forms
// (batched_bounded_resolve.hip, which describes the flow and the layout), included INSIDE each of them. As it stands
// it runs Dantzig's rule; under the macro LP_BOUNDED_BLAND or LP_BOUNDED_DEVEX batched_bounded_loop.hpp's loop runs
// that rule, and under LP_BOUNDED_DEVEX the carve carries the weights (wts). Under LP_BOUNDED_DUAL_DEVEX
// batched_bounded_dual_loop.hpp's loop prices by Devex with one weight per basis position (dwts), which share the
// region of wts: an LP runs one of the two loops. Under LP_BOUNDED_DUAL_LONG_STEP that loop's entering step is the
// bound-flipping ratio test, whose flips are counted with the primal loop's. BLAND = false is for
// batched_lds_loop.hpp, of which only the pivot is used. Not a standalone header.
    constexpr bool BLAND = false;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    char* base = reinterpret_cast<char*>(smem);
    const int m = d.m, n = d.n, W = n + 1;
#ifdef LP_BOUNDED_DEVEX
    const BoundedCarve K = bounded_carve(m, n, true);
#elif defined(LP_BOUNDED_DUAL_DEVEX)
    const BoundedCarve K = bounded_carve(m, n, false, m);
#else
    const BoundedCarve K = bounded_carve(m, n);
#endif
    const int pitch = K.pitch;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int lp = blockIdx.x;
    // ---- LDS carve
    Published* pubs = reinterpret_cast<Published*>(smem);
    double* T = reinterpret_cast<double*>(base + K.T);
    double* prow = reinterpret_cast<double*>(base + K.prow);
    double* lcol = reinterpret_cast<double*>(base + K.lcol);
    double* U = reinterpret_cast<double*>(base + K.U);
    double* lov = reinterpret_cast<double*>(base + K.lov);
    int* slotvar = reinterpret_cast<int*>(base + K.slotvar);
    int* basis = reinterpret_cast<int*>(base + K.basis);
    int* up = reinterpret_cast<int*>(base + K.up);
#ifdef LP_BOUNDED_DEVEX
    double* wts = reinterpret_cast<double*>(base + K.wts);   // the Devex weights, one per slot
#endif
#ifdef LP_BOUNDED_DUAL_DEVEX
    double* dwts = reinterpret_cast<double*>(base + K.wts);   // the dual Devex weights, one per basis position
#endif
    int* pub = pubs->v;   // [0] entering slot / crash row, [1] leaving position, [2] action / verdict, [3] block_any

    const double* A = d.A + (size_t)lp * m * n;
    const double* b = d.b + (size_t)lp * m;
    const double* c = d.c + (size_t)lp * n;
    const double* lo = d.lo + (size_t)lp * n;
    const double* hi = d.hi + (size_t)lp * n;
    const int* N = d.basis_in + (size_t)lp * m;
    const int* upin = d.at_upper_in + (size_t)lp * n;
    const double eps = d.eps;
    const bool maximize = d.maximize != 0;
    constexpr int ANY_WORD = 3;   // block_any's word of pub
#include "batched_block_any.hpp"

    // ---- load: slots = the columns in order (a flagged one sign-changed, cost included), basis = the artificials
    int bad = 0;
    for (int s = tid; s < n; s += NT) {
        const double l = lo[s], u = hi[s] - l;
        const int f = upin[s];
        slotvar[s] = s;
        up[s] = f;
        lov[s] = l;
        U[s] = u;
        T[(size_t)m * pitch + s] = f ? -c[s] : c[s];
        if (u < 0.0) bad = 1;
    }
    if (tid == 0) T[(size_t)m * pitch + n] = 0.0;
    for (int t = tid; t < m; t += NT) basis[t] = n + t;
    for (int e = tid; e < m * n; e += NT) {   // coalesced along the rows of a column
        const int s = e / m, i = e - s * m;
        const double a = A[e];
        T[(size_t)i * pitch + s] = upin[s] ? -a : a;
    }
    const bool crossed = block_any(bad);
    // ---- b' (one chain per row): the shift over lo_j != 0, then the complements over the flagged columns
    if (!crossed) {
        for (int i = tid; i < m; i += NT) {
            const double* row = T + (size_t)i * pitch;
            double acc = b[i];
            for (int j = 0; j < n; ++j) {
                const double l = lov[j];
                if (l != 0.0) acc = fma(up[j] ? row[j] : -row[j], l, acc);   // (-A_ij: a flagged slot holds it)
            }
            for (int j = 0; j < n; ++j)
                if (up[j]) acc = fma(row[j], U[j], acc);
            T[(size_t)i * pitch + n] = acc;
        }
    }
    // the crash is skipped when the basic columns, as loaded, are the unit vectors in order and their costs are zero
    int not_identity = 0;
    if (!crossed) {
        for (int e = tid; e < m * m; e += NT) {
            const int t = e / m, i = e - t * m;
            if (T[(size_t)i * pitch + N[t]] != ((i == t) ? 1.0 : 0.0)) not_identity = 1;
        }
        for (int t = tid; t < m; t += NT)
            if (T[(size_t)m * pitch + N[t]] != 0.0) not_identity = 1;
    }
    const bool identity = !block_any(not_identity);

    // ---- pivot(r, se); the bounded primal loop; the bounded dual loop
#include "batched_lds_loop.hpp"
#include "batched_bounded_loop.hpp"
#include "batched_bounded_dual_loop.hpp"
    (void)simplex;   // (batched_lds_loop.hpp's unbounded loop: only its pivot is used here)

    int it[3] = {0, 0, 0};   // dual pivots, primal pivots, bound flips
    int status = crossed ? LP_INFEASIBLE : LP_OPTIMAL;
    if (!crossed) {
#include "batched_resolve_crash.hpp"
    }
    if (!crossed && status == LP_OPTIMAL) {
        // ---- classification: two block reductions over the crashed tableau
        int pinf = 0, dinf = 0;
        for (int t = tid; t < m; t += NT) {
            const double xb = T[(size_t)t * pitch + n], u = U[basis[t]];
            if (xb < -eps || (u < INFINITY && u - xb < -eps)) pinf = 1;
        }
        const double* drow = T + (size_t)m * pitch;
        for (int s = tid; s < n; s += NT)
            if (slotvar[s] < n && (maximize ? (drow[s] > eps) : (drow[s] < -eps))) dinf = 1;
        const bool violated = block_any(pinf);
        const bool dual_feasible = !block_any(dinf);
        if (!violated)
            status = bounded_simplex(true, maximize, it[1], it[2]);   // artificial slots barred
        else if (dual_feasible)
#ifdef LP_BOUNDED_DUAL_LONG_STEP
            status = bounded_dual(it[0], it[2]);
#else
            status = bounded_dual(it[0]);
#endif
        else
            status = LP_BAD_ARG;
        __syncthreads();
    }
    // ---- outputs as batched_bounded.hip: x for LP_OPTIMAL; basis, flags and counters always (the given basis when
    // the crash failed or some hi < lo: the flags are the given ones then)
    if (status == LP_OPTIMAL) {
        for (int j = tid; j < n; j += NT) prow[j] = 0.0;
        __syncthreads();
        for (int t = tid; t < m; t += NT)
            if (basis[t] < n) prow[basis[t]] = T[(size_t)t * pitch + n];
        __syncthreads();
        double* x = d.x + (size_t)lp * n;
        for (int j = tid; j < n; j += NT) {
            const double v = prow[j];
            const double w = up[j] ? U[j] - v : v;
            x[j] = lov[j] == 0.0 ? w : lov[j] + w;
        }
    }
    const bool given = crossed || status == LP_SINGULAR;
    for (int t = tid; t < m; t += NT) d.basis_out[(size_t)lp * m + t] = given ? N[t] : basis[t];
    for (int j = tid; j < n; j += NT) d.at_upper[(size_t)lp * n + j] = up[j];
    if (tid == 0) {
        int* io = d.iters + (size_t)lp * 3;
        io[0] = it[0];
        io[1] = it[1];
        io[2] = it[2];
        d.status[lp] = status;
    }
