// The launch sequence of a Merkle tree build (run_merkle, path.hip) as a pure host function: no HIP in this header, so
// tests/cpp/test_merkle_plan.cpp checks it against the three per-hasher loops it replaced.
#pragma once
#include <stdint.h>

namespace wf {

// How one hasher's tree goes from the leaves to the root: wide levels one (or, where a two-level kernel exists, two) per
// launch with one lane per node, then the LDS sub-tree kernel, up to subtree_levels levels per launch.
struct MerklePlan {
    bool two_level;            // k_merkle_level2 exists: taken by levels of >= 2^l2_min parents (l2_min: the context's tuning value)
    uint32_t level_min_log;    // k_merkle_level: levels of >= 2^level_min_log parents ("a level still fills the chip") ..
    uint32_t level_l2_min;     // .. and only under this l2_min (0: under any)
    uint32_t subtree_levels;   // most levels of one sub-tree launch
    uint32_t subtree_span;     // parents of the first produced level per sub-tree work-group
    uint32_t subtree_threads;  // its work-group size
};

// BLAKE3: levels of >= 2^18 parents two per launch; below that k_merkle_subtree folds 9 levels per launch (one launch less
// than switching at 2^16, 5 us at 2^23 leaves).  One level per launch only with WF_EXP_MERKLE_L2_MIN=16.
constexpr MerklePlan MERKLE_PLAN_BLAKE3 = {true, 15, 16, 9, 256, 256};
// Sha3_256: the one-lane-per-node rule of BLAKE3 without a two-level kernel.
constexpr MerklePlan MERKLE_PLAN_SHA3 = {false, 15, 0, 9, 256, 256};
// Rp64_256: the sub-tree kernel is the lane form (k_merkle_subtree_lanes<rp::Lanes>: 16 lanes per parent, rp::permute_lane).  The switch is measured
// (docs/EXPERIMENTS.md "Rp64_256", scripts/rescue_bench.hip): a level of up to 2^16 parents costs one permutation's latency
// with one lane per parent (0.33 ms), the lane form's latency is a ninth of that and its throughput 73 %, so it wins up to
// 2^15 parents.
constexpr MerklePlan MERKLE_PLAN_RP64 = {false, 16, 0, 7, 64, 1024};
// RpJive64_256: the sub-tree kernel is the same lane form (<rpj::Lanes>) with 8 lanes per parent and none idle (rpj::merge_lane), so a
// work-group of 1024 lanes spans 128 parents and folds 8 levels.  The switch is measured (docs/EXPERIMENTS.md
// "RpJive64_256", scripts/rescue_jive_bench.hip, profiles/rpjive_rescue_bench.txt).  One level, ms, lane per parent / lane
// form: 2^13 0.219 / 0.068, 2^14 0.219 / 0.071, 2^15 0.224 / 0.075, 2^16 0.230 / 0.131, 2^17 0.297 / 0.238, 2^18 0.507 / 0.443,
// 2^20 1.694 / 1.649, 2^22 6.491 / 6.505: with no idle lanes the lane form runs at 97-98 % of the other form's register-only
// rate (Rp64_256: 73 %), so a single level only crosses over at 2^22.  What a launch of eight levels loses on its idle waves
// moves the best switch of a whole tree down: 2^23 leaves 14.23 / 13.99 / 14.16 / 14.51 ms with the lane-per-parent kernel
// from 2^16 / 2^17 / 2^18 / 2^19 parents up, 2^18 leaves 1.170 / 1.086 ms from 2^16 / 2^17; two earlier sessions order them
// the same way (14.49 / 14.26 / 14.46 / 14.77; 1.165 / 1.090 and 1.192 / 1.105).
constexpr MerklePlan MERKLE_PLAN_RPJIVE = {false, 17, 0, 8, 128, 1024};
// GriffinJive64_256: one lane per parent throughout (gfj::merge has no lane-split form), so Sha3_256's shape -- the generic
// LDS sub-tree kernel, 9 levels per launch -- with the switch one level up.  Measured (docs/EXPERIMENTS.md
// "GriffinJive64_256", scripts/griffin_bench.hip, profiles/griffin_bench.txt): a level of up to 2^15 parents costs one
// permutation's latency in either kernel (0.049 ms; 2^16: 0.052, 2^17: 0.065, 2^18: 0.107), so the switch moves little.  Whole
// trees, ms, three rounds each, with k_merkle_level from 2^14 / 2^15 / 2^16 / 2^17 / 2^18 parents up: 2^23 leaves
// 3.514 3.508 3.562 / 3.519 3.510 3.517 / 3.495 3.493 3.503 / 3.478 3.516 3.487 / 3.585 3.572 3.617; 2^18 leaves
// 0.970 0.958 0.939 / 0.951 0.952 0.948 / 0.947 0.936 0.934 / 0.943 0.949 0.945.  2^16 is the only value that is first or
// second in all six columns.  (From 2^10 up the small tree gains 5 %, 0.874 .. 0.909, and the large one loses 5 %, 3.66 .. 3.72.)
constexpr MerklePlan MERKLE_PLAN_GRIFFIN = {false, 16, 0, 9, 256, 256};

enum MerkleLaunch : uint32_t { MERKLE_LEVEL2, MERKLE_LEVEL, MERKLE_SUBTREE };

struct MerkleStep {
    MerkleLaunch kind;
    uint32_t levels;      // levels this launch produces
    uint64_t grid;        // work-groups (the caller refuses a grid above 2^31 - 1)
    uint32_t block;       // threads per work-group
    uint64_t n_children;  // nodes of the last level produced: the next launch's children, 1 = the root
};

// The next launch of a tree whose lowest level not yet folded has n_children (a power of two, >= 2) nodes.  num_cus: the
// two-level kernel walks its level with a grid-stride loop on at most 8 work-groups per CU.
inline MerkleStep merkle_next_launch(uint64_t n_children, const MerklePlan &p, uint32_t l2_min, uint32_t num_cus) {
    const uint64_t n_par = n_children >> 1;
    const uint32_t threads = 256;
    const uint64_t grid = (n_par + threads - 1) / threads;  // one lane per parent
    if (p.two_level && n_par >= ((uint64_t)1 << l2_min)) {  // one lane per grandparent
        const uint64_t n_grand = n_par >> 1, all = (n_grand + threads - 1) / threads, cap = (uint64_t)num_cus * 8;
        return {MERKLE_LEVEL2, 2, all < cap ? all : cap, threads, n_grand};
    }
    if (n_par >= ((uint64_t)1 << p.level_min_log) && (p.level_l2_min == 0 || p.level_l2_min == l2_min))
        return {MERKLE_LEVEL, 1, grid, threads, n_par};
    uint32_t total_levels = 0;
    for (uint64_t t = n_children; t > 1; t >>= 1) total_levels++;
    const uint32_t levels = total_levels < p.subtree_levels ? total_levels : p.subtree_levels;
    return {MERKLE_SUBTREE, levels, (n_par + p.subtree_span - 1) / p.subtree_span, p.subtree_threads, n_children >> levels};
}

}  // namespace wf
