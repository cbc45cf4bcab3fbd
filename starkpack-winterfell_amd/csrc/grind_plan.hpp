// The window schedule of the nonce search (wf_grind_seeds, grind.hip) as a pure host function: no HIP in this header, so
// tests/cpp/test_grind_plan.cpp checks it under plain g++.
#pragma once
#include <stdint.h>

namespace wf {

// How one hasher's search walks its range.  All three numbers come from profiles/grind_rates.txt (scripts/time_grind.py on
// one MI355X; docs/STATUS.md "Grinding" has the table):
//   first_log2  the first window: the largest one whose launch still costs about what the host's look at the result costs
//               (~20 us), so that small grinding factors end in one launch and larger ones skip the launches that would be
//               all overhead;
//   cap_log2    the largest window: 1 to 3 ms of one seed's search, which bounds the work behind the answer and what
//               anything else queued on the stream waits for;
//   lane_iters  nonces one lane tests at most in a large window (<= GRIND_LANE_ITERS, the loop bound of k_grind).  Several
//               per lane let a lane stop once a smaller nonce has been found and keep the grid small.
struct GrindPlan {
    uint32_t first_log2, cap_log2, lane_iters;
};
constexpr uint32_t GRIND_LANE_ITERS = 8;
// BLAKE3: 2^20 nonces are 22 us (2^16: 7 us, the launch floor), 2^26 are 0.99 ms (67.5 G nonces/s).
constexpr GrindPlan GRIND_PLAN_BLAKE3 = {20, 26, GRIND_LANE_ITERS};
// Sha3_256: 2^16 nonces are 15 us, 2^24 are 2.56 ms (6.55 G nonces/s; 2^26 would be 10.2 ms).
constexpr GrindPlan GRIND_PLAN_SHA3 = {16, 24, GRIND_LANE_ITERS};
// Rp64_256: any launch is at least one permutation's latency, 0.32 ms, which 2^16 nonces still cost (2^17: 0.41 ms); 2^20
// are 2.61 ms (0.400 G nonces/s).  One nonce per lane: a chip-full of lanes (2^18) costs 0.74 ms when its work-groups start
// together, and as much again for every further iteration of the same lanes (2^20 nonces as 1024 work-groups x 4
// iterations: 2.93 ms; 2048 x 2: 2.72 ms), but 0.62 ms when fresh work-groups take the place of finished ones one by one
// (4096 x 1: 2.61 ms) -- presumably the waves of a SIMD then sit in different phases of the permutation; the cause was not
// examined further.  A work-group that starts behind the answer leaves at once, so nothing is lost for the early exit.
constexpr GrindPlan GRIND_PLAN_RP64 = {16, 20, 1};
// RpJive64_256 (scripts/time_grind.py rpjive64_256, profiles/rpjive_rescue_bench.txt): one permutation's latency is 0.22 ms,
// which 2^16 nonces still cost (0.219 ms; 2^17: 0.277, 2^18: 0.487, 2^19: 0.896); 2^20 are 1.71 ms (0.614 G nonces/s, 100 % of
// the register-only loop of the width-8 permutation; 2^21 would be 3.4 ms).  The same three numbers as Rp64_256 come out; one
// nonce per lane is taken over from it and was not measured again.
constexpr GrindPlan GRIND_PLAN_RPJIVE = {16, 20, 1};
// GriffinJive64_256 (scripts/time_grind.py griffin, profiles/griffin_grind.txt): one permutation's latency is 0.044 ms, which
// 2^16 nonces still cost (0.049 ms; 2^17: 0.059, 2^18: 0.096, 2^19: 0.169, 2^20: 0.315, 2^21: 0.611): that launch is the
// smallest there is, 2.5 looks of the host.  2^22 are 1.19 ms (3.48 G nonces/s, 103 % of the register-only loop of the
// permutation); 2^23 would be 2.4 ms and was not timed.  One nonce per lane: the same library with 8 per lane gives 1.31 ms for
// 2^22 (3.18 G nonces/s) in the same session, as Rp64_256 found.
constexpr GrindPlan GRIND_PLAN_GRIFFIN = {16, 22, 1};

struct GrindWindow {
    uint64_t base, count;  // nonces base .. base + count - 1; count == 0: the range is spent
};

// The window behind `done` nonces of the range [begin, begin + max_nonces) clipped to end at 2^64 - 1 (`done` = the sum of
// the windows before it).  Sizes 2^first_log2, 2^(first_log2 + 1), .. up to 2^cap_log2, then 2^cap_log2 each; the last one
// is clipped to the range.  Range ends are differences: nothing here can wrap.  first_log2 <= cap_log2 <= 63.
inline GrindWindow grind_next_window(uint64_t begin, uint64_t max_nonces, uint64_t done, uint32_t first_log2, uint32_t cap_log2) {
    const uint64_t room = (uint64_t)0 - begin;  // nonces from begin to 2^64 - 1 (0 stands for 2^64: begin == 0)
    const uint64_t total = (begin != 0 && room < max_nonces) ? room : max_nonces;
    if (done >= total) return {begin, 0};
    const uint64_t first = (uint64_t)1 << first_log2, cap = (uint64_t)1 << cap_log2;
    // the doubling windows sum to 2^k * first - first: behind them the next size is done + first, until that reaches the cap
    const uint64_t size = done < cap - first ? done + first : cap;
    const uint64_t left = total - done;
    return {begin + done, size < left ? size : left};
}

// Work-groups of `threads` lanes for a window of count <= 2^62 nonces: one lane per nonce while that stays within
// max_groups (a few work-groups per CU), then the same grid with more nonces per lane, and more work-groups where
// lane_iters nonces per lane do not cover the window.  groups * threads * lane_iters >= count always.
inline uint64_t grind_groups(uint64_t count, uint32_t threads, uint64_t max_groups, uint32_t lane_iters) {
    const uint64_t one_each = (count + threads - 1) / threads;
    const uint64_t per = (uint64_t)threads * lane_iters, fewest = (count + per - 1) / per;
    const uint64_t g = one_each < max_groups ? one_each : max_groups;
    return g > fewest ? g : fewest;
}

}  // namespace wf
