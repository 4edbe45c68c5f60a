// batched_block_any.hpp — the block-wide OR of the one-LP-per-workgroup kernels that start from a given basis,
// included INSIDE each kernel body.  Not a standalone header.
//   reads:    tid, pub (the workgroup's published ints) and ANY_WORD, a constexpr int the kernel defines: the word of
//             pub that is this fragment's alone (3 beside the Published record of the simplex loops, 2 in the basis_*
//             analysis kernels, whose pub[3] is taken or absent)
//   defines:  block_any(flag): true in every thread when flag != 0 in some thread
//   barriers: three per call (clear, set, read); the word is free again when the call returns
//   included by: k_batched_resolve, k_batched_bounded_resolve, k_batched_mip, k_batched_mip_bounded,
//             k_batched_parametric, k_batched_parametric_cost (ANY_WORD 3); k_batched_duals, k_batched_ranging,
//             k_batched_certificate, k_batched_bounded_sens, k_batched_bounded_certificate (ANY_WORD 2)
// (__syncthreads_or would add static LDS beside the 160 KB of the largest shapes)
    auto block_any = [&](int flag) {
        if (tid == 0) pub[ANY_WORD] = 0;
        __syncthreads();
        if (flag) pub[ANY_WORD] = 1;
        __syncthreads();
        const bool any = pub[ANY_WORD] != 0;
        __syncthreads();
        return any;
    };
