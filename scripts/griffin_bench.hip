// Bring-up microbenchmark (not part of the product): the GriffinJive64_256 kernels against register-only loops of the
// permutation; the sibling of scripts/rescue_jive_bench.hip, whose RpJive64_256 loop is repeated here for the ratio of the two.
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -I starkpack-winterfell_amd/csrc scripts/griffin_bench.hip -o /tmp/griffin_bench
//   single  gfj::permute       one lane, one permutation           (five runs: their spread is what the pair form must beat)
//   pair    gfj::permute_n<2>  one lane, two interleaved states    (the two inverse S-boxes of a round walk together)
// Then: one tree level of 2^10 .. 2^22 parents in k_merkle_level<gfj::Merge> and in k_merkle_subtree<gfj::Merge> with one level,
// the trees over 2^18 and 2^23 leaves with the level / sub-tree switch moved (MERKLE_PLAN_GRIFFIN.level_min_log,
// csrc/merkle_plan.hpp, is read off these), the wide level and the row kernel, each as permutations per second and as a
// fraction of the single form's loop.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "griffin_dev.hpp"
#include "keccak_kernels.hpp"
#include "kernels.hpp"
#include "merkle_plan.hpp"

using namespace wf;

#define CHECK(x)                                                            \
    do {                                                                    \
        hipError_t e = (x);                                                 \
        if (e != hipSuccess) {                                              \
            printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); \
            return 1;                                                       \
        }                                                                   \
    } while (0)

template <int N>
__global__ void __launch_bounds__(256) k_perm_loop(uint64_t *out, uint32_t iters) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t s[N][gfj::STATE];
#pragma unroll
    for (int n = 0; n < N; n++)
#pragma unroll
        for (int i = 0; i < gfj::STATE; i++) s[n][i] = rp::elem_new((g * N + n) * 0x9E3779B97F4A7C15ull + i);
    for (uint32_t it = 0; it < iters; it++) gfj::permute_n<N>(s);
    uint64_t acc = 0;
#pragma unroll
    for (int n = 0; n < N; n++)
#pragma unroll
        for (int i = 0; i < gfj::STATE; i++) acc ^= s[n][i];
    out[g] = acc;
}

__global__ void __launch_bounds__(256) k_perm_loop_rpjive(uint64_t *out, uint32_t iters) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t s[rpj::STATE];
#pragma unroll
    for (int i = 0; i < rpj::STATE; i++) s[i] = rp::elem_new(g * 0x9E3779B97F4A7C15ull + i);
    for (uint32_t it = 0; it < iters; it++) rpj::permute(s);
    uint64_t acc = 0;
#pragma unroll
    for (int i = 0; i < rpj::STATE; i++) acc ^= s[i];
    out[g] = acc;
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

static void level(const void *children, void *nodes, uint64_t n_par) {
    hipLaunchKernelGGL(k_merkle_level<gfj::Merge>, dim3((uint32_t)((n_par + 255) / 256)), dim3(256), 0, 0, (const uint64_t *)children,
                       (uint64_t *)nodes + n_par * 4, n_par);
}

static void subtree(const void *children, void *nodes, uint64_t n_children, uint32_t levels) {
    const uint64_t n_par = n_children >> 1;
    hipLaunchKernelGGL(k_merkle_subtree<gfj::Merge>, dim3((uint32_t)((n_par + 255) / 256)), dim3(256), 0, 0, (const uint64_t *)children,
                       (uint64_t *)nodes, n_children, levels);
}

static void tree(const void *leaves, uint64_t n_leaves, void *nodes, uint32_t level_min_log) {  // the plan of run_merkle with the switch at 2^level_min_log
    const uint64_t *children = (const uint64_t *)leaves;
    uint64_t n_children = n_leaves;
    while (n_children > 1) {
        const uint64_t n_par = n_children >> 1;
        if (n_par >= (1ull << level_min_log)) {
            level(children, nodes, n_par);
            n_children = n_par;
        } else {
            uint32_t total = 0;
            for (uint64_t t = n_children; t > 1; t >>= 1) total++;
            const uint32_t levels = std::min<uint32_t>(MERKLE_PLAN_GRIFFIN.subtree_levels, total);
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
    const uint32_t blocks = (uint32_t)cus * 16;
    uint64_t *sink;
    CHECK(hipMalloc(&sink, (size_t)blocks * 256 * 8));
    float ms, lo = 1e30f, hi = 0, sum = 0;
    for (int run = 0; run < 5; run++) {
        ms = timeit([&] { hipLaunchKernelGGL(k_perm_loop<1>, dim3(blocks), dim3(256), 0, 0, sink, 32u); }, 3);
        printf("%-60s %9.3f ms  %8.2f Mperm/s  (run %d, %d CUs)\n", "single: register-only gfj::permute loop", ms, (double)blocks * 256 * 32 / ms / 1e3, run, cus);
        lo = std::min(lo, ms), hi = std::max(hi, ms), sum += ms;
    }
    const double yard = (double)blocks * 256 * 32 / (sum / 5) / 1e3;  // Mperm/s
    printf("%-60s %9.3f ms  %8.2f Mperm/s  (yardstick; spread %.2f %%)\n", "single: mean of the five runs", sum / 5, yard, 100.0 * (hi - lo) / (sum / 5));
    for (int run = 0; run < 3; run++) {
        ms = timeit([&] { hipLaunchKernelGGL(k_perm_loop<2>, dim3(blocks), dim3(256), 0, 0, sink, 32u); }, 3);
        const double y2 = (double)blocks * 256 * 2 * 32 / ms / 1e3;
        printf("%-60s %9.3f ms  %8.2f Mperm/s  %5.1f %% of single (run %d)\n", "pair: register-only gfj::permute_n<2> loop", ms, y2, 100.0 * y2 / yard, run);
    }
    ms = timeit([&] { hipLaunchKernelGGL(k_perm_loop_rpjive, dim3(blocks), dim3(256), 0, 0, sink, 8u); }, 3);
    const double yardj = (double)blocks * 256 * 8 / ms / 1e3;
    printf("%-60s %9.3f ms  %8.2f Mperm/s  (Griffin / RpJive = %.2f)\n", "RpJive64_256: register-only rpj::permute loop", ms, yardj, yard / yardj);
    ms = timeit([&] { hipLaunchKernelGGL(k_perm_loop<1>, dim3(1), dim3(64), 0, 0, sink, 16u); }, 3);
    printf("%-60s %9.4f ms per permutation\n", "single: one wave alone", ms / 16);
    ms = timeit([&] { hipLaunchKernelGGL(k_perm_loop<2>, dim3(1), dim3(64), 0, 0, sink, 16u); }, 3);
    printf("%-60s %9.4f ms per pair of permutations\n", "pair: one wave alone", ms / 16);

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
        printf("one tree level, milliseconds (level = k_merkle_level<gfj::Merge>, sub-tree = k_merkle_subtree<gfj::Merge> with one level)\n");
        for (uint32_t lg = 10; lg <= 22; lg += (lg < 18 ? 1 : 2)) {
            const uint64_t n_par = 1ull << lg;
            const float m1 = timeit([&] { level(leaves, nodes, n_par); }, 5);
            const float m2 = timeit([&] { subtree(leaves, nodes, 2 * n_par, 1); }, 5);
            printf("  2^%-2u parents   level %8.3f   sub-tree %8.3f\n", lg, m1, m2);
        }
        for (int round = 0; round < 3; round++) {
            for (uint32_t sw : {10u, 12u, 13u, 14u, 15u, 16u, 17u}) {
                ms = timeit([&] { tree(leaves, 1ull << 18, nodes, sw); }, 5);
                printf("tree over 2^18 leaves, level kernel from 2^%u parents up (round %d) %10.3f ms\n", sw, round, ms);
            }
            for (uint32_t sw : {10u, 12u, 13u, 14u, 15u, 16u, 17u, 18u}) {
                ms = timeit([&] { tree(leaves, n, nodes, sw); }, 3);
                printf("tree over 2^23 leaves, level kernel from 2^%u parents up (round %d) %10.3f ms\n", sw, round, ms);
            }
        }
    }
    {
        ms = timeit([&] { tree(leaves, n, nodes, MERKLE_PLAN_GRIFFIN.level_min_log); }, 3);
        const double r = (double)(n - 1) / ms / 1e3;
        printf("%-60s %9.3f ms  %8.2f Mperm/s  %5.1f %% of the yardstick\n", "tree, 2^23 leaves (the product's sequence)", ms, r, 100.0 * r / yard);
        ms = timeit([&] { level(leaves, nodes, n / 2); }, 3);
        const double r1 = (double)(n / 2) / ms / 1e3;
        printf("%-60s %9.3f ms  %8.2f Mperm/s  %5.1f %% of the yardstick\n", "k_merkle_level<gfj::Merge>, 2^22 parents", ms, r1, 100.0 * r1 / yard);
    }
    CHECK(hipFree(leaves));
    CHECK(hipFree(nodes));
    // row kernel: permutations per row = ceil(elements / 4)
    struct Shape { uint32_t log_rows, cols; const char *name; };
    const Shape shapes[] = {{23, 8, "k_hash_rows_sponge<F64, gfj::Absorb>, 2^23 rows x 8"}, {20, 64, "k_hash_rows_sponge<F64, gfj::Absorb>, 2^20 rows x 64"}};
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
        ms = timeit([&] { hipLaunchKernelGGL((k_hash_rows_sponge<F64, gfj::Absorb>), dim3((uint32_t)(rows / 256)), dim3(256), 0, 0, a); }, 3);
        const double perms = (double)rows * ((sh.cols + 3) / 4), r = perms / ms / 1e3;
        printf("%-60s %9.3f ms  %8.2f Mperm/s  %5.1f %% of the yardstick\n", sh.name, ms, r, 100.0 * r / yard);
        CHECK(hipFree(lde));
        CHECK(hipFree(lv));
    }
    CHECK(hipFree(sink));
    return 0;
}
