// The window schedule of the nonce search (grind_next_window, csrc/grind_plan.hpp), checked from its statement alone:
// windows are contiguous from `begin`, sum to min(max_nonces, 2^64 - begin), follow the doubling rule up to the cap, the
// last one is clipped and nothing wraps past 2^64 - 1.  Ranges too long to walk window by window (2^40 nonces and up at
// 2^12 per window) are walked through the doubling part and 40 capped windows, and again through the last 40 windows
// (`done` placed on the window boundaries the schedule itself would reach).  Plain g++: the header needs no HIP.
#include <cinttypes>
#include <cstdio>
#include <initializer_list>

#include "../../starkpack-winterfell_amd/csrc/grind_plan.hpp"

using wf::grind_next_window;
using wf::GrindWindow;
typedef unsigned __int128 u128;

static long g_bad = 0, g_windows = 0;

static void bad(const char *what, uint64_t begin, uint64_t max_nonces, uint32_t f, uint32_t c, uint64_t done) {
    if (g_bad++ < 20)
        printf("MISMATCH %s: begin %" PRIu64 " max_nonces %" PRIu64 " first 2^%u cap 2^%u done %" PRIu64 "\n", what, begin, max_nonces, f, c, done);
}

// walks at most `limit` windows from `done` (a boundary: index k of the schedule); returns the new `done`
static uint64_t walk(uint64_t begin, uint64_t max_nonces, uint32_t f, uint32_t c, u128 total, uint64_t done, int limit) {
    const uint64_t first = (uint64_t)1 << f, cap = (uint64_t)1 << c;
    for (int n = 0; n < limit; n++) {
        const GrindWindow w = grind_next_window(begin, max_nonces, done, f, c);
        g_windows++;
        if ((u128)done >= total) {
            if (w.count != 0) bad("a window behind the end of the range", begin, max_nonces, f, c, done);
            return done;
        }
        // the size the rule gives this window: first * 2^k while that is below the cap, k = windows before it
        const uint64_t doubling_sum = cap - first;  // the sum of all windows smaller than the cap
        uint64_t want;
        if (done < doubling_sum) {
            want = first;
            for (uint64_t sum = 0; sum < done; sum += want, want *= 2) {}
            uint64_t sum = 0;
            for (uint64_t s = first; s < want; s *= 2) sum += s;
            if (sum != done) bad("the test's own boundary", begin, max_nonces, f, c, done);
        } else {
            want = cap;
            if ((done - doubling_sum) % cap != 0) bad("the test's own boundary", begin, max_nonces, f, c, done);
        }
        const u128 left = total - done;
        const bool last = (u128)want >= left;
        if (last) want = (uint64_t)left;  // the clip
        if (w.count != want) bad("window size", begin, max_nonces, f, c, done);
        if (w.count == 0) return done;  // (reported above; do not loop on it)
        if (w.base != begin + done) bad("window base (not contiguous)", begin, max_nonces, f, c, done);
        // nothing wraps: the window's last nonce, as a wide integer, is at most 2^64 - 1 and inside the range
        const u128 end = (u128)w.base + w.count;  // one past the last nonce
        if (end > ((u128)1 << 64)) bad("the window runs past 2^64 - 1", begin, max_nonces, f, c, done);
        if (end > (u128)begin + total) bad("the window runs past the range", begin, max_nonces, f, c, done);
        if (w.base < begin) bad("the base wrapped", begin, max_nonces, f, c, done);
        done += w.count;
        if (last && (u128)done != total) bad("the windows do not sum to the range", begin, max_nonces, f, c, done);
    }
    return done;
}

int main() {
    const uint64_t begins[] = {0, 1, 0xFFFFFFFFull, (uint64_t)1 << 63, (uint64_t)0 - 70, ~(uint64_t)0};
    const uint64_t counts[] = {1, 2, 63, 64, 65, 1000, (uint64_t)1 << 40, ~(uint64_t)0};
    long schedules = 0;
    for (uint32_t f = 2; f <= 12; f++)
        for (uint32_t c = f; c <= 12; c++)
            for (uint64_t begin : begins)
                for (uint64_t max_nonces : counts) {
                    const u128 room = ((u128)1 << 64) - begin;
                    const u128 total = (u128)max_nonces < room ? (u128)max_nonces : room;
                    const GrindWindow w0 = grind_next_window(begin, max_nonces, 0, f, c);
                    if (w0.base != begin || w0.count == 0) bad("the first window does not start at begin", begin, max_nonces, f, c, 0);
                    const int head = (int)(c - f) + 40;
                    uint64_t done = walk(begin, max_nonces, f, c, total, 0, head);
                    if ((u128)done < total) {
                        // the last 40 windows: boundaries of the capped part are doubling_sum + k * cap
                        const uint64_t cap = (uint64_t)1 << c, doubling_sum = cap - ((uint64_t)1 << f);
                        const u128 capped = (total - doubling_sum + cap - 1) / cap;  // capped windows in all (the last one clipped)
                        const u128 k = capped > 40 ? capped - 40 : 0;
                        const uint64_t from = (uint64_t)(doubling_sum + k * cap);
                        if (from > done) done = from;
                        done = walk(begin, max_nonces, f, c, total, done, 41);
                    }
                    if ((u128)done != total) bad("the walk did not reach the end of the range", begin, max_nonces, f, c, done);
                    if (grind_next_window(begin, max_nonces, done, f, c).count != 0) bad("a window behind the last", begin, max_nonces, f, c, done);
                    schedules++;
                }
    // grind_groups: enough lanes for the window, one nonce per lane while the grid stays small
    for (uint64_t count : {(uint64_t)1, (uint64_t)255, (uint64_t)256, (uint64_t)257, (uint64_t)1 << 16, ((uint64_t)1 << 22) + 1, (uint64_t)1 << 30})
        for (uint64_t max_groups : {(uint64_t)1, (uint64_t)8, (uint64_t)2048})
            for (uint32_t iters : {1u, 2u, wf::GRIND_LANE_ITERS}) {
                const uint64_t g = wf::grind_groups(count, 256, max_groups, iters);
                if (g == 0 || g * 256 * iters < count) bad("grind_groups: the grid does not cover the window", count, max_groups, iters, 0, g);
                if (g > (count + 255) / 256) bad("grind_groups: more lanes than nonces", count, max_groups, iters, 0, g);
                if ((g - 1) * 256 * iters >= count && g > max_groups) bad("grind_groups: above max_groups without need", count, max_groups, iters, 0, g);
            }
    printf("%s: %ld schedules checked, %ld windows, %ld mismatches\n", g_bad ? "FAILED" : "ok", schedules, g_windows, g_bad);
    return g_bad ? 1 : 0;
}
