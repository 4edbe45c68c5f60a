// batched_bounded_carve.hpp — the LDS carve of the bounded-variable kernels (batched_bounded.hip,
// batched_bounded_resolve.hip; the layout is described in the former), computed alike on the host (the launch's
// dynamic LDS size) and in the kernel.  Included after batched_scan.hpp (Published).
#pragma once

namespace {

struct BoundedCarve {
    int pitch;
    size_t T, prow, lcol, U, lov, slotvar, basis, up, bytes;   // byte offsets
};

__host__ __device__ inline BoundedCarve bounded_carve(int m, int n) {
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
    k.bytes = (o + 15) & ~(size_t)15;
    return k;
}

}  // namespace
