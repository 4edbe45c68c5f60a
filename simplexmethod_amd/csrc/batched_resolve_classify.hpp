// batched_resolve_classify.hpp — the classification of a row-form tableau whose basis batched_resolve_crash.hpp has
// installed (resolve_ref.c's), included INSIDE each kernel after the crash, where status == LP_OPTIMAL.  Not a
// standalone header.
//   reads:    m, n, pitch, T, slotvar, eps, tid, NT, block_any; drow, the reduced-cost row T + m * pitch; maximize, the
//             sense (a constexpr bool in the kernels that take it as a template parameter)
//   defines:  primal_feasible (no xB_t < -eps) and dual_feasible (no slot of a variable < n with d > eps (max) /
//             d < -eps (min)), the same in every thread; the kernel picks its loop or its verdict from them
//   barriers: six (two block_any calls)
//   included by: k_batched_resolve, k_batched_mip (its classify_run lambda), k_batched_parametric,
//             k_batched_parametric_cost
    int pinf = 0, dinf = 0;
    for (int t = tid; t < m; t += NT)
        if (T[(size_t)t * pitch + n] < -eps) pinf = 1;
    for (int s = tid; s < n; s += NT)
        if (slotvar[s] < n && (maximize ? (drow[s] > eps) : (drow[s] < -eps))) dinf = 1;
    const bool primal_feasible = !block_any(pinf);
    const bool dual_feasible = !block_any(dinf);
