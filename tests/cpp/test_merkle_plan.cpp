// CPU: merkle_next_launch (csrc/merkle_plan.hpp, the launch sequence of every hasher's tree) against the three per-hasher
// host loops it replaced, restated here as they stood (run_merkle_dw, run_merkle_sha3, run_merkle_rp64 of csrc/path.hip;
// a launch is recorded where they launched).  Every n_leaves = 2^1 .. 2^34, every merkle_l2_min the context accepts
// (10 .. 30) and several CU counts (the two-level kernel's grid cap).  Plain C++: the header needs no HIP.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../../starkpack-winterfell_amd/csrc/merkle_plan.hpp"

using namespace wf;

struct Launch {
    uint32_t kind, levels, block;
    uint64_t grid, before, after;
    bool operator==(const Launch &o) const {
        return kind == o.kind && levels == o.levels && block == o.block && grid == o.grid && before == o.before && after == o.after;
    }
};
typedef std::vector<Launch> Seq;

// ---- the loops as they stood
static Seq old_blake3(uint64_t n_leaves, uint32_t l2_min, uint32_t num_cus) {  // run_merkle_dw<DW>, either DW
    Seq seq;
    uint64_t n_children = n_leaves;
    while (n_children > 1) {
        const uint64_t before = n_children;
        const uint64_t n_par = n_children >> 1;
        const uint32_t threads = 256;
        const uint64_t grid = (n_par + threads - 1) / threads;
        if (n_par >= ((uint64_t)1 << l2_min)) {
            const uint64_t n_grand = n_par >> 1;
            const uint64_t blocks2 = std::min<uint64_t>((n_grand + threads - 1) / threads, (uint64_t)num_cus * 8);
            n_children = n_grand;
            seq.push_back({MERKLE_LEVEL2, 2, threads, blocks2, before, n_children});
        } else if (n_par >= (1u << 15) && l2_min == 16) {
            n_children = n_par;
            seq.push_back({MERKLE_LEVEL, 1, threads, grid, before, n_children});
        } else {
            uint32_t total_levels = 0;
            for (uint64_t t = n_children; t > 1; t >>= 1) total_levels++;
            const uint32_t levels = std::min<uint32_t>(9, total_levels);
            n_children >>= levels;
            seq.push_back({MERKLE_SUBTREE, levels, threads, grid, before, n_children});
        }
    }
    return seq;
}

static Seq old_sha3(uint64_t n_leaves) {  // run_merkle_sha3
    const uint32_t SHA3_LEVEL_MIN_LOG = 15;
    Seq seq;
    uint64_t n_children = n_leaves;
    while (n_children > 1) {
        const uint64_t before = n_children;
        const uint64_t n_par = n_children >> 1;
        const uint32_t threads = 256;
        const uint64_t grid = (n_par + threads - 1) / threads;
        if (n_par >= ((uint64_t)1 << SHA3_LEVEL_MIN_LOG)) {
            n_children = n_par;
            seq.push_back({MERKLE_LEVEL, 1, threads, grid, before, n_children});
        } else {
            uint32_t total_levels = 0;
            for (uint64_t t = n_children; t > 1; t >>= 1) total_levels++;
            const uint32_t levels = std::min<uint32_t>(9, total_levels);
            n_children >>= levels;
            seq.push_back({MERKLE_SUBTREE, levels, threads, grid, before, n_children});
        }
    }
    return seq;
}

static Seq old_rp64(uint64_t n_leaves) {  // run_merkle_rp64
    const uint32_t RP64_LEVEL_MIN_LOG = 16, RP64_SUBTREE_THREADS = 1024, RP64_SUBTREE_SPAN = RP64_SUBTREE_THREADS / 16,
                   RP64_SUBTREE_LEVELS = 7;
    Seq seq;
    uint64_t n_children = n_leaves;
    while (n_children > 1) {
        const uint64_t before = n_children;
        const uint64_t n_par = n_children >> 1;
        if (n_par >= ((uint64_t)1 << RP64_LEVEL_MIN_LOG)) {
            const uint32_t threads = 256;
            const uint64_t grid = (n_par + threads - 1) / threads;
            n_children = n_par;
            seq.push_back({MERKLE_LEVEL, 1, threads, grid, before, n_children});
        } else {
            uint32_t total_levels = 0;
            for (uint64_t t = n_children; t > 1; t >>= 1) total_levels++;
            const uint32_t levels = std::min<uint32_t>(RP64_SUBTREE_LEVELS, total_levels);
            const uint64_t grid = (n_par + RP64_SUBTREE_SPAN - 1) / RP64_SUBTREE_SPAN;
            n_children >>= levels;
            seq.push_back({MERKLE_SUBTREE, levels, RP64_SUBTREE_THREADS, grid, before, n_children});
        }
    }
    return seq;
}

// ---- the driver loop of run_merkle_plan
static Seq planned(uint64_t n_leaves, const MerklePlan &plan, uint32_t l2_min, uint32_t num_cus) {
    Seq seq;
    uint64_t n_children = n_leaves;
    while (n_children > 1 && seq.size() < 64) {  // (a step that did not shrink the level would otherwise never end)
        const MerkleStep s = merkle_next_launch(n_children, plan, l2_min, num_cus);
        seq.push_back({s.kind, s.levels, s.block, s.grid, n_children, s.n_children});
        n_children = s.n_children;
    }
    return seq;
}

static int compare(const char *what, uint64_t n_leaves, uint32_t l2_min, uint32_t num_cus, const Seq &want, const Seq &got) {
    if (want == got) return 0;
    printf("MISMATCH %s n_leaves=%llu l2_min=%u num_cus=%u\n", what, (unsigned long long)n_leaves, l2_min, num_cus);
    for (int side = 0; side < 2; side++)
        for (const Launch &l : side ? got : want)
            printf("  %s kind=%u levels=%u grid=%llu block=%u children %llu -> %llu\n", side ? "new" : "old", l.kind, l.levels,
                   (unsigned long long)l.grid, l.block, (unsigned long long)l.before, (unsigned long long)l.after);
    return 1;
}

int main() {
    const uint32_t cus[] = {1, 64, 256, 304};
    int bad = 0;
    uint64_t compared = 0, launches = 0;
    for (uint32_t log_n = 1; log_n <= 34; log_n++) {
        const uint64_t n = (uint64_t)1 << log_n;
        for (uint32_t l2_min = 10; l2_min <= 30; l2_min++) {
            for (uint32_t num_cus : cus) {
                const Seq want = old_blake3(n, l2_min, num_cus);
                bad += compare("BLAKE3", n, l2_min, num_cus, want, planned(n, MERKLE_PLAN_BLAKE3, l2_min, num_cus));
                // the other two loops never saw the tuning value or the CU count
                bad += compare("Sha3_256", n, l2_min, num_cus, old_sha3(n), planned(n, MERKLE_PLAN_SHA3, l2_min, num_cus));
                bad += compare("Rp64_256", n, l2_min, num_cus, old_rp64(n), planned(n, MERKLE_PLAN_RP64, l2_min, num_cus));
                compared += 3;
                launches += want.size();
                if (bad > 8) return 1;
            }
        }
    }
    printf("%s: %llu sequences compared (%llu BLAKE3 launches), %d mismatches\n", bad ? "FAIL" : "ok",
           (unsigned long long)compared, (unsigned long long)launches, bad);
    return bad ? 1 : 0;
}
