// Bring-up microbenchmark (not part of the product): the Sha3_256 kernels against a register-only Keccak-f[1600] loop.
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -I starkpack-winterfell_amd/csrc scripts/keccak_bench.hip -o /tmp/keccak_bench
// The yardstick chains permutations in registers (one store per lane at the end): what the vector ALU gives this instruction
// sequence with nothing else in the way.  The tree (the launch sequence of run_merkle with the Sha3 plan, csrc/path.hip, on 2^23 leaves)
// and the row kernel are reported as permutations per second and as a fraction of it.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "keccak_dev.hpp"
#include "keccak_kernels.hpp"
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

__global__ void __launch_bounds__(256) k_perm_loop(uint64_t *out, uint32_t iters) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t s[25];
#pragma unroll
    for (int i = 0; i < 25; i++) s[i] = g * 0x9E3779B97F4A7C15ull + i;
    for (uint32_t it = 0; it < iters; it++) k3::keccak_f(s);
    uint64_t acc = 0;
#pragma unroll
    for (int i = 0; i < 25; i++) acc ^= s[i];
    out[g] = acc;
}

template <class K>
static float timeit(K launch, int reps) {
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    launch();
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

static int tree(const void *leaves, uint64_t n_leaves, void *nodes) {  // run_merkle_plan<k3::Merge, MERKLE_PLAN_SHA3>, csrc/path.hip
    const uint64_t *children = (const uint64_t *)leaves;
    uint64_t *out = (uint64_t *)nodes, n_children = n_leaves;
    while (n_children > 1) {
        const MerkleStep s = merkle_next_launch(n_children, MERKLE_PLAN_SHA3, 0, 0);
        const uint64_t n_par = n_children >> 1;
        if (s.kind == MERKLE_LEVEL)
            hipLaunchKernelGGL(k_merkle_level<k3::Merge>, dim3((uint32_t)s.grid), dim3(s.block), 0, 0, children, out + n_par * 4, n_par);
        else
            hipLaunchKernelGGL(k_merkle_subtree<k3::Merge>, dim3((uint32_t)s.grid), dim3(s.block), 0, 0, children, out, n_children, s.levels);
        n_children = s.n_children;
        children = out + n_children * 4;
    }
    return 0;
}

int main() {
    int cus = 0;
    CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0));
    // yardstick: 16 work-groups of 256 per CU, 64 chained permutations per lane
    const uint32_t blocks = (uint32_t)cus * 16, iters = 64;
    uint64_t *sink;
    CHECK(hipMalloc(&sink, (size_t)blocks * 256 * 8));
    float ms = timeit([&] { hipLaunchKernelGGL(k_perm_loop, dim3(blocks), dim3(256), 0, 0, sink, iters); }, 10);
    const double yard = (double)blocks * 256 * iters / ms / 1e6;  // Gperm/s
    printf("%-52s %8.3f ms  %7.2f Gperm/s  (yardstick, %d CUs)\n", "register-only keccak_f loop", ms, yard, cus);

    {   // tree over 2^23 leaves
        const uint64_t n = 1ull << 23;
        void *leaves, *nodes;
        CHECK(hipMalloc(&leaves, n * 32));
        CHECK(hipMalloc(&nodes, n * 32));
        std::vector<uint64_t> h(n * 4);
        for (uint64_t i = 0; i < h.size(); i++) h[i] = i * 0x9E3779B97F4A7C15ull;
        CHECK(hipMemcpy(leaves, h.data(), n * 32, hipMemcpyHostToDevice));
        ms = timeit([&] { tree(leaves, n, nodes); }, 10);
        const double r = (double)(n - 1) / ms / 1e6;
        printf("%-52s %8.3f ms  %7.2f Gperm/s  %5.1f %% of the yardstick\n", "Sha3 tree, 2^23 leaves (the product's sequence)", ms, r, 100.0 * r / yard);
        ms = timeit([&] { hipLaunchKernelGGL(k_merkle_level<k3::Merge>, dim3((uint32_t)(n / 2 / 256)), dim3(256), 0, 0, (const uint64_t *)leaves, (uint64_t *)nodes + 2 * n, n / 2); }, 10);
        const double r1 = (double)(n / 2) / ms / 1e6;
        printf("%-52s %8.3f ms  %7.2f Gperm/s  %5.1f %% of the yardstick\n", "k_merkle_level<k3::Merge>, 2^22 parents", ms, r1, 100.0 * r1 / yard);
        CHECK(hipFree(leaves));
        CHECK(hipFree(nodes));
    }
    // row kernel: permutations per row = floor(row bytes / 136) + 1
    struct Shape { uint32_t log_rows, cols; const char *name; };
    const Shape shapes[] = {{23, 8, "k_hash_rows_sponge<F64, k3::Absorb>, 2^23 rows x 8 (64 bytes)"},
                            {16, 64, "k_hash_rows_sponge<F64, k3::Absorb>, 2^16 rows x 64 (512 bytes)"},
                            {20, 64, "k_hash_rows_sponge<F64, k3::Absorb>, 2^20 rows x 64 (512 bytes)"}};
    for (const Shape &sh : shapes) {
        const uint64_t rows = 1ull << sh.log_rows;
        uint64_t *lde;
        uint32_t *leaves;
        CHECK(hipMalloc(&lde, rows * sh.cols * 8));
        CHECK(hipMalloc(&leaves, rows * 32));
        CHECK(hipMemset(lde, 0x5A, rows * sh.cols * 8));
        HashArgs<F64> a;
        a.lde = lde;
        a.trace_elems = rows * sh.cols;
        a.n_rows = rows;
        a.row_width = sh.cols;
        a.epr = sh.cols;
        a.n_traces = 1;
        a.leaves = leaves;
        a.digest_words = 8;
        ms = timeit([&] { hipLaunchKernelGGL((k_hash_rows_sponge<F64, k3::Absorb>), dim3((uint32_t)(rows / 256)), dim3(256), 0, 0, a); }, 10);
        const double perms = (double)rows * (sh.cols * 8 / 136 + 1), r = perms / ms / 1e6;
        printf("%-52s %8.3f ms  %7.2f Gperm/s  %5.1f %% of the yardstick  (%.0f GB/s read)\n", sh.name, ms, r, 100.0 * r / yard,
               (double)rows * sh.cols * 8 / ms / 1e6);
        CHECK(hipFree(lde));
        CHECK(hipFree(leaves));
    }
    CHECK(hipFree(sink));
    return 0;
}
