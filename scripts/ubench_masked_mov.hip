// ubench_masked_mov.hip — issue cost of a 64-bit select on gfx950, two ways: (i) a pair of v_cndmask_b32 on an
// SGPR-pair condition, (ii) one v_mov_b64 under a lane mask that a scalar instruction sets every five moves (the shape
// of leaf_verdict's row rotation in enum_leaf.hip: one condition per row, five columns) — and, as the yardstick, (iii)
// v_mov_b64 with the lane mask left alone.  Every wave runs a long unrolled run of one form on its own registers, at
// 1, 2 and 3 waves per SIMD, with per-lane masks that differ from group to group.  One workgroup of 256 x w threads
// per CU: each workgroup claims more than half of a CU's LDS (kLdsBytes, untouched), so that no two share a CU and
// the waves per SIMD are what the block size says.  Reported: ticks of the waves' own s_memtime counter per 64-bit
// select and SIMD, and next to it the same from the launch's wall time at the NOMINAL device clock (clockRate: the
// clock under load may differ, so compare the forms, not the two columns).
//
// Build: hipcc --offload-arch=gfx950 -O3 -o scripts/_build/ubench_masked_mov scripts/ubench_masked_mov.hip
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

#define CHECK(x)                                                                     \
    do {                                                                             \
        hipError_t e_ = (x);                                                         \
        if (e_ != hipSuccess) {                                                      \
            fprintf(stderr, "%s:%d %s -> %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
            exit(1);                                                                 \
        }                                                                            \
    } while (0)

constexpr int kGroups = 8;        // groups of five selects per loop body, a mask each
constexpr int kPerGroup = 5;
constexpr int kIters = 10000;     // 400,000 selects per wave and launch
constexpr int kLdsBytes = 96 * 1024;   // of a CU's 160 KB: one workgroup per CU

struct Params {
    const double* in;             // 10 doubles per lane
    const int* key;               // per-lane key: mask k holds the lanes with bit k of the key set
    unsigned long long* cycles;   // per wave
    double* out;                  // per lane, keeps the registers alive
    int iters;
};

// FORM 0: pairs of v_cndmask_b32; 1: v_mov_b64 under a mask set per group; 2: v_mov_b64, mask untouched
template <int FORM>
__global__ __launch_bounds__(768) void k_select(Params p) {
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    extern __shared__ char placement_only[];   // kLdsBytes, never accessed
    double d[kPerGroup], s[kPerGroup];
    for (int i = 0; i < kPerGroup; ++i) {
        d[i] = p.in[gid * 10 + i];
        s[i] = p.in[gid * 10 + 5 + i];
    }
    const int key = p.key[gid];
    unsigned long long mask[kGroups];
    for (int k = 0; k < kGroups; ++k) mask[k] = __ballot((key >> k) & 1);
    int dl[kPerGroup], dh[kPerGroup], sl[kPerGroup], sh[kPerGroup];
    for (int i = 0; i < kPerGroup; ++i) {
        dl[i] = __double2loint(d[i]);
        dh[i] = __double2hiint(d[i]);
        sl[i] = __double2loint(s[i]);
        sh[i] = __double2hiint(s[i]);
    }
    __syncthreads();
    const unsigned long long t0 = __builtin_readcyclecounter();
    for (int it = 0; it < p.iters; ++it) {
#pragma unroll
        for (int k = 0; k < kGroups; ++k) {
            if constexpr (FORM == 0) {
                asm volatile(
                    "v_cndmask_b32_e64 %0, %0, %10, %20\n\tv_cndmask_b32_e64 %1, %1, %11, %20\n\t"
                    "v_cndmask_b32_e64 %2, %2, %12, %20\n\tv_cndmask_b32_e64 %3, %3, %13, %20\n\t"
                    "v_cndmask_b32_e64 %4, %4, %14, %20\n\tv_cndmask_b32_e64 %5, %5, %15, %20\n\t"
                    "v_cndmask_b32_e64 %6, %6, %16, %20\n\tv_cndmask_b32_e64 %7, %7, %17, %20\n\t"
                    "v_cndmask_b32_e64 %8, %8, %18, %20\n\tv_cndmask_b32_e64 %9, %9, %19, %20"
                    : "+v"(dl[0]), "+v"(dh[0]), "+v"(dl[1]), "+v"(dh[1]), "+v"(dl[2]), "+v"(dh[2]), "+v"(dl[3]),
                      "+v"(dh[3]), "+v"(dl[4]), "+v"(dh[4])
                    : "v"(sl[0]), "v"(sh[0]), "v"(sl[1]), "v"(sh[1]), "v"(sl[2]), "v"(sh[2]), "v"(sl[3]), "v"(sh[3]),
                      "v"(sl[4]), "v"(sh[4]), "s"(mask[k]));
            } else if constexpr (FORM == 1) {
                unsigned long long sv;
                asm volatile(
                    "s_and_saveexec_b64 %0, %11\n\t"
                    "v_mov_b64 %1, %6\n\tv_mov_b64 %2, %7\n\tv_mov_b64 %3, %8\n\tv_mov_b64 %4, %9\n\tv_mov_b64 %5, %10\n\t"
                    "s_mov_b64 exec, %0"
                    : "=&s"(sv), "+v"(d[0]), "+v"(d[1]), "+v"(d[2]), "+v"(d[3]), "+v"(d[4])
                    : "v"(s[0]), "v"(s[1]), "v"(s[2]), "v"(s[3]), "v"(s[4]), "s"(mask[k])
                    : "scc");
            } else {
                asm volatile(
                    "v_mov_b64 %0, %5\n\tv_mov_b64 %1, %6\n\tv_mov_b64 %2, %7\n\tv_mov_b64 %3, %8\n\tv_mov_b64 %4, %9"
                    : "+v"(d[0]), "+v"(d[1]), "+v"(d[2]), "+v"(d[3]), "+v"(d[4])
                    : "v"(s[0]), "v"(s[1]), "v"(s[2]), "v"(s[3]), "v"(s[4]));
            }
        }
    }
    const unsigned long long t1 = __builtin_readcyclecounter();
    if ((threadIdx.x & 63) == 0) p.cycles[gid >> 6] = t1 - t0;
    double acc = 0.0;
    for (int i = 0; i < kPerGroup; ++i)
        acc += FORM == 0 ? __hiloint2double(dh[i], dl[i]) : d[i];
    p.out[gid] = acc;
}

template <int FORM>
double run(const char* name, Params p, int cus, int waves_per_simd, int clock_khz, unsigned long long* h_cycles) {
    const int threads = 256 * waves_per_simd;   // one workgroup per CU: 4 SIMDs x waves_per_simd waves
    const int waves = cus * threads / 64;
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_select<FORM>), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes));
    hipLaunchKernelGGL((k_select<FORM>), cus, threads, kLdsBytes, 0, p);   // warm-up
    CHECK(hipDeviceSynchronize());
    CHECK(hipEventRecord(e0));
    hipLaunchKernelGGL((k_select<FORM>), cus, threads, kLdsBytes, 0, p);
    CHECK(hipEventRecord(e1));
    CHECK(hipDeviceSynchronize());
    float ms = 0.f;
    CHECK(hipEventElapsedTime(&ms, e0, e1));
    CHECK(hipMemcpy(h_cycles, p.cycles, waves * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    double sum = 0.0, mx = 0.0;
    for (int w = 0; w < waves; ++w) {
        sum += (double)h_cycles[w];
        if ((double)h_cycles[w] > mx) mx = (double)h_cycles[w];
    }
    const double selects = (double)p.iters * kGroups * kPerGroup;
    const double per = sum / waves / selects / waves_per_simd;
    const double wall = (double)ms * 1e-3 * (double)clock_khz * 1e3 / selects / waves_per_simd;
    printf("%-34s %d waves/SIMD: %6.3f counter ticks per 64-bit select and SIMD (slowest wave %6.3f); wall %.3f ms = %6.3f cycles at the nominal %d MHz\n",
           name, waves_per_simd, per, mx / selects / waves_per_simd, ms, wall, clock_khz / 1000);
    fflush(stdout);
    CHECK(hipEventDestroy(e0));
    CHECK(hipEventDestroy(e1));
    return per;
}

int main() {
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount;
    const int lanes = cus * 768;
    double* in;
    int* key;
    unsigned long long* cycles;
    double* out;
    CHECK(hipMalloc(&in, (size_t)lanes * 10 * sizeof(double)));
    CHECK(hipMalloc(&key, (size_t)lanes * sizeof(int)));
    CHECK(hipMalloc(&cycles, (size_t)(lanes / 64) * sizeof(unsigned long long)));
    CHECK(hipMalloc(&out, (size_t)lanes * sizeof(double)));
    double* h_in = (double*)malloc((size_t)lanes * 10 * sizeof(double));
    int* h_key = (int*)malloc((size_t)lanes * sizeof(int));
    unsigned long long* h_cycles = (unsigned long long*)malloc((size_t)(lanes / 64) * sizeof(unsigned long long));
    unsigned x = 12345u;
    for (int i = 0; i < lanes; ++i) {
        for (int k = 0; k < 10; ++k) h_in[(size_t)i * 10 + k] = 1.0 + (double)((i * 10 + k) % 977) / 977.0;
        x = x * 1664525u + 1013904223u;
        h_key[i] = (int)(x >> 13) & 0xFF;   // per-lane masks: about half of the lanes in each of the 8
    }
    CHECK(hipMemcpy(in, h_in, (size_t)lanes * 10 * sizeof(double), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(key, h_key, (size_t)lanes * sizeof(int), hipMemcpyHostToDevice));
    Params p{in, key, cycles, out, kIters};
    printf("%s, %d CUs, %d selects per wave\n", prop.name, cus, kIters * kGroups * kPerGroup);
    for (int w = 1; w <= 3; ++w) {
        const double a = run<0>("(i)   2 x v_cndmask_b32", p, cus, w, prop.clockRate, h_cycles);
        const double b = run<1>("(ii)  v_mov_b64, mask set per five", p, cus, w, prop.clockRate, h_cycles);
        run<2>("(iii) v_mov_b64, mask untouched", p, cus, w, prop.clockRate, h_cycles);
        printf("   %d waves/SIMD: (ii) / (i) = %.3f\n", w, b / a);
    }
    return 0;
}
