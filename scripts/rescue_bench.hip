// Bring-up microbenchmark (not part of the product): the Rp64_256 kernels against register-only loops of the permutation.
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -I starkpack-winterfell_amd/csrc scripts/rescue_bench.hip -o /tmp/rescue_bench
// Two yardsticks, one per form of the permutation (csrc/rescue_dev.hpp): permutations chained in registers, one store per
// lane at the end -- what the vector ALU gives the instruction sequence with nothing else in the way.
//   form 1  rp::permute       one lane per permutation
//   form 2  rp::permute_lane  one state element per lane, 16 lanes per permutation
// Then: one tree level of 2^8 .. 2^18 parents in either form (MERKLE_PLAN_RP64.level_min_log, csrc/merkle_plan.hpp, is read off this
// table), the tree over 2^23 leaves, and the row kernel, each as permutations per second and as a fraction of form 1's loop.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "keccak_kernels.hpp"
#include "rescue_kernels.hpp"

using namespace wf;

#define CHECK(x)                                                            \
    do {                                                                    \
        hipError_t e = (x);                                                 \
        if (e != hipSuccess) {                                              \
            printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); \
            return 1;                                                       \
        }                                                                   \
    } while (0)

__global__ void __launch_bounds__(256) k_perm_loop(uint64_t *out, uint32_t iters) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t s[rp::STATE];
#pragma unroll
    for (int i = 0; i < rp::STATE; i++) s[i] = rp::elem_new(g * 0x9E3779B97F4A7C15ull + i);
    for (uint32_t it = 0; it < iters; it++) rp::permute(s);
    uint64_t acc = 0;
#pragma unroll
    for (int i = 0; i < rp::STATE; i++) acc ^= s[i];
    out[g] = acc;
}

__global__ void __launch_bounds__(256) k_lane_loop(uint64_t *out, uint32_t iters) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t x = rp::elem_new(g * 0x9E3779B97F4A7C15ull);
    for (uint32_t it = 0; it < iters; it++) x = rp::permute_lane(x);
    out[g] = x;
}

template <class K>
static float timeit(K launch, int reps) {
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    launch();
    hipDeviceSynchronize();
    hipEventRecord(e0);
    for (int i = 0; i < reps; i++) launch();
    hipEventRecord(e1);
    hipEventSynchronize(e1);
    float ms;
    hipEventElapsedTime(&ms, e0, e1);
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    return ms / reps;
}

static void level_form1(const void *children, void *nodes, uint64_t n_par) {
    hipLaunchKernelGGL(k_merkle_level<rp::Merge>, dim3((uint32_t)((n_par + 255) / 256)), dim3(256), 0, 0, (const uint64_t *)children,
                       (uint64_t *)nodes + n_par * 4, n_par);
}

static void subtree(const void *children, void *nodes, uint64_t n_children, uint32_t levels) {
    const uint64_t n_par = n_children >> 1;
    constexpr MerklePlan P = MERKLE_PLAN_RP64;
    hipLaunchKernelGGL(k_merkle_subtree_lanes<rp::Lanes>, dim3((uint32_t)((n_par + P.subtree_span - 1) / P.subtree_span)),
                       dim3(P.subtree_threads), 0, 0, (const uint64_t *)children, (uint64_t *)nodes, n_children, levels);
}

static void tree(const void *leaves, uint64_t n_leaves, void *nodes, uint32_t level_min_log) {  // the Rp64 plan of run_merkle with the switch at 2^level_min_log
    const uint64_t *children = (const uint64_t *)leaves;
    uint64_t n_children = n_leaves;
    while (n_children > 1) {
        const uint64_t n_par = n_children >> 1;
        if (n_par >= (1ull << level_min_log)) {
            level_form1(children, nodes, n_par);
            n_children = n_par;
        } else {
            uint32_t total = 0;
            for (uint64_t t = n_children; t > 1; t >>= 1) total++;
            const uint32_t levels = std::min<uint32_t>(MERKLE_PLAN_RP64.subtree_levels, total);
            subtree(children, nodes, n_children, levels);
            n_children >>= levels;
        }
        children = (const uint64_t *)nodes + n_children * 4;
    }
}

int main(int argc, char **argv) {
    const bool quick = argc > 1;  // any argument: the yardsticks, the wide level and the row kernel only
    int cus = 0;
    CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0));
    // yardsticks: 16 work-groups of 256 per CU (the register budget holds 4 waves per SIMD: four rounds of them), 8 chained
    // permutations per lane -- some tens of milliseconds per launch, as long as the kernels they are compared with
    const uint32_t blocks = (uint32_t)cus * 16;
    uint64_t *sink;
    CHECK(hipMalloc(&sink, (size_t)blocks * 256 * 8));
    float ms = timeit([&] { hipLaunchKernelGGL(k_perm_loop, dim3(blocks), dim3(256), 0, 0, sink, 8u); }, 3);
    const double yard = (double)blocks * 256 * 8 / ms / 1e3;  // Mperm/s
    printf("%-56s %9.3f ms  %8.2f Mperm/s  (yardstick, %d CUs)\n", "form 1: register-only permute loop", ms, yard, cus);
    ms = timeit([&] { hipLaunchKernelGGL(k_lane_loop, dim3(blocks), dim3(256), 0, 0, sink, 128u); }, 3);
    const double yard2 = (double)blocks * 16 * 128 / ms / 1e3;
    printf("%-56s %9.3f ms  %8.2f Mperm/s  %5.1f %% of form 1\n", "form 2: register-only permute_lane loop", ms, yard2, 100.0 * yard2 / yard);
    // one chained permutation of a single wave: the latency of a narrow level
    ms = timeit([&] { hipLaunchKernelGGL(k_perm_loop, dim3(1), dim3(64), 0, 0, sink, 4u); }, 3);
    printf("%-56s %9.3f ms per permutation\n", "form 1: one wave alone", ms / 4);
    ms = timeit([&] { hipLaunchKernelGGL(k_lane_loop, dim3(1), dim3(64), 0, 0, sink, 16u); }, 3);
    printf("%-56s %9.3f ms per permutation\n", "form 2: one wave alone", ms / 16);

    const uint64_t n = 1ull << 23;
    void *leaves, *nodes;
    CHECK(hipMalloc(&leaves, n * 32));
    CHECK(hipMalloc(&nodes, n * 32));
    {
        std::vector<uint64_t> h(n * 4);
        for (uint64_t i = 0; i < h.size(); i++) h[i] = i * 0x9E3779B97F4A7C15ull;
        CHECK(hipMemcpy(leaves, h.data(), n * 32, hipMemcpyHostToDevice));
    }
    if (!quick) {
        printf("one tree level, milliseconds (form 1 = k_merkle_level<rp::Merge>, form 2 = k_merkle_subtree_lanes<rp::Lanes> with one level)\n");
        for (uint32_t lg = 8; lg <= 18; lg++) {
            const uint64_t n_par = 1ull << lg;
            const float m1 = timeit([&] { level_form1(leaves, nodes, n_par); }, 3);
            const float m2 = timeit([&] { subtree(leaves, nodes, 2 * n_par, 1); }, 3);
            printf("  2^%-2u parents   form 1 %8.3f   form 2 %8.3f\n", lg, m1, m2);
        }
        for (uint32_t sw : {14u, 15u, 16u, 17u}) {
            ms = timeit([&] { tree(leaves, 1ull << 18, nodes, sw); }, 2);
            printf("tree over 2^18 leaves, form 1 from 2^%u parents up %17.3f ms\n", sw, ms);
        }
    }
    {
        ms = timeit([&] { tree(leaves, n, nodes, 16); }, 2);
        const double r = (double)(n - 1) / ms / 1e3;
        printf("%-56s %9.3f ms  %8.2f Mperm/s  %5.1f %% of the yardstick\n", "tree, 2^23 leaves (the product's sequence)", ms, r, 100.0 * r / yard);
        ms = timeit([&] { level_form1(leaves, nodes, n / 2); }, 2);
        const double r1 = (double)(n / 2) / ms / 1e3;
        printf("%-56s %9.3f ms  %8.2f Mperm/s  %5.1f %% of the yardstick\n", "k_merkle_level<rp::Merge>, 2^22 parents", ms, r1, 100.0 * r1 / yard);
    }
    CHECK(hipFree(leaves));
    CHECK(hipFree(nodes));
    // row kernel: permutations per row = ceil(elements / 8)
    struct Shape { uint32_t log_rows, cols; const char *name; };
    const Shape shapes[] = {{23, 8, "k_hash_rows_sponge<F64, rp::Absorb>, 2^23 rows x 8"}, {20, 64, "k_hash_rows_sponge<F64, rp::Absorb>, 2^20 rows x 64"}};
    for (const Shape &sh : shapes) {
        const uint64_t rows = 1ull << sh.log_rows;
        uint64_t *lde;
        uint32_t *lv;
        CHECK(hipMalloc(&lde, rows * sh.cols * 8));
        CHECK(hipMalloc(&lv, rows * 32));
        CHECK(hipMemset(lde, 0x5A, rows * sh.cols * 8));
        HashArgs<F64> a;
        a.lde = lde;
        a.trace_elems = rows * sh.cols;
        a.n_rows = rows;
        a.row_width = sh.cols;
        a.epr = sh.cols;
        a.n_traces = 1;
        a.leaves = lv;
        a.digest_words = 8;
        ms = timeit([&] { hipLaunchKernelGGL((k_hash_rows_sponge<F64, rp::Absorb>), dim3((uint32_t)(rows / 256)), dim3(256), 0, 0, a); }, 2);
        const double perms = (double)rows * ((sh.cols + 7) / 8), r = perms / ms / 1e3;
        printf("%-56s %9.3f ms  %8.2f Mperm/s  %5.1f %% of the yardstick\n", sh.name, ms, r, 100.0 * r / yard);
        CHECK(hipFree(lde));
        CHECK(hipFree(lv));
    }
    CHECK(hipFree(sink));
    return 0;
}
