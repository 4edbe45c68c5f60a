// batched_bounded_carve.hpp — the LDS carve of the bounded-variable kernels (batched_bounded.hip,
// batched_bounded_resolve.hip; the layout is described in the former), computed alike on the host (the launch's
// dynamic LDS size) and in the kernel.  Included after batched_scan.hpp (Published).  With `weights` the carve carries
// one more region behind the ints, wts (n doubles, 8-byte aligned): the Devex weights of the rule kernels; without it
// the carve is what it always was.  With `dual_weights` > 0 and no `weights` the region holds that many doubles: the
// dual loop's Devex weights, one per basis position (m).  A re-solve runs one of the two loops, so with both rules
// they share the n >= m doubles of `weights`.
#pragma once

namespace {

struct BoundedCarve {
    int pitch;
    size_t T, prow, lcol, U, lov, slotvar, basis, up, wts, bytes;   // byte offsets (wts: 0 without weights)
};

__host__ __device__ inline BoundedCarve bounded_carve(int m, int n, bool weights = false, int dual_weights = 0) {
    BoundedCarve k{};
    const int W = n + 1;
    k.pitch = (W & 1) ? W : W + 1;   // odd pitch: conflict-free column reads
    size_t o = sizeof(Published);
    k.T = o;
    o += sizeof(double) * (size_t)(m + 1) * k.pitch;
    k.prow = o;
    o += sizeof(double) * (size_t)W;
    k.lcol = o;
    o += sizeof(double) * (size_t)(m + 1);
    k.U = o;
    o += sizeof(double) * (size_t)n;
    k.lov = o;
    o += sizeof(double) * (size_t)n;
    k.slotvar = o;
    o += sizeof(int) * (size_t)n;
    k.basis = o;
    o += sizeof(int) * (size_t)m;
    k.up = o;
    o += sizeof(int) * (size_t)n;
    if (weights) {
        o = (o + 7) & ~(size_t)7;
        k.wts = o;
        o += sizeof(double) * (size_t)n;
    } else if (dual_weights > 0) {
        o = (o + 7) & ~(size_t)7;
        k.wts = o;
        o += sizeof(double) * (size_t)dual_weights;
    }
    k.bytes = (o + 15) & ~(size_t)15;
    return k;
}

}  // namespace
