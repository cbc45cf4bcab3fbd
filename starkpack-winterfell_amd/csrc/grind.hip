// libwf_lde.so, unit 7 of 8 -- the proof-of-work of the query seed: wf_grind_seeds (ProverChannel::grind_query_seed,
// prover/src/channel.rs:182-198) on the kernels of grind_kernels.hpp and the window schedule of grind_plan.hpp.
#include "wf_internal.hpp"

#include "grind_kernels.hpp"

using namespace wf;

namespace {

// device layout of one call (ctx->grind), and the same in pinned host memory (ctx->qpin): the inputs in front, so that one
// copy takes them up; the outputs behind, so that one copy brings them back
struct GrindLayout {
    size_t seeds, best, nonces, new_seeds, found, bytes;
    explicit GrindLayout(size_t n) {
        seeds = 0;
        best = seeds + n * 32;
        nonces = best + n * 8;
        new_seeds = nonces + n * 8;
        found = new_seeds + n * 32;
        bytes = (found + n + 15) & ~(size_t)15;
    }
};

template <class G>
int grind_run(wf_ctx *ctx, hipStream_t st, char *dev, char *pin, const GrindLayout &L, uint32_t n_seeds, uint32_t factor,
              uint64_t begin, uint64_t max_nonces, const GrindPlan &plan) {
    const uint32_t mask = factor >= 32 ? 0xFFFFFFFFu : (((uint32_t)1 << factor) - 1);
    const uint64_t *d_seeds = (const uint64_t *)(dev + L.seeds);
    uint64_t *d_best = (uint64_t *)(dev + L.best);
    const volatile uint64_t *h_best = (const volatile uint64_t *)(pin + L.best);
    uint64_t done = 0;
    for (;;) {
        const GrindWindow w = grind_next_window(begin, max_nonces, done, plan.first_log2, plan.cap_log2);
        if (w.count == 0) break;
        const uint64_t groups = grind_groups(w.count, GRIND_THREADS, (uint64_t)ctx->num_cus * 8, plan.lane_iters);
        prof_mark(ctx, st, "grind.window");
        hipLaunchKernelGGL((k_grind<G>), dim3((uint32_t)groups, n_seeds), dim3(GRIND_THREADS), 0, st, d_seeds, d_best, w.base, w.count, mask);
        HIP_TRY(hipGetLastError());
        prof_mark(ctx, st, "grind.readback");
        HIP_TRY(hipMemcpyAsync(pin + L.best, d_best, (size_t)n_seeds * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        done += w.count;
        bool all = true;
        for (uint32_t i = 0; i < n_seeds; i++) all = all && h_best[i] != GRIND_NONE;
        if (all) break;
    }
    // is 2^64 - 1, which best[] cannot tell from "nothing found", a nonce of the range?
    const uint32_t last_in_range = begin != 0 && max_nonces >= (uint64_t)0 - begin;
    prof_mark(ctx, st, "grind.finish");
    hipLaunchKernelGGL((k_grind_finish<G>), dim3((n_seeds + GRIND_THREADS - 1) / GRIND_THREADS), dim3(GRIND_THREADS), 0, st, d_seeds,
                       d_best, n_seeds, mask, last_in_range, (uint64_t *)(dev + L.nonces), (uint64_t *)(dev + L.new_seeds),
                       (uint8_t *)(dev + L.found));
    HIP_TRY(hipGetLastError());
    prof_mark(ctx, st, "between_calls");
    HIP_TRY(hipMemcpyAsync(pin + L.nonces, dev + L.nonces, L.bytes - L.nonces, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

}  // namespace

extern "C" int wf_grind_seeds(wf_ctx *ctx, const uint8_t *seeds, size_t n_seeds, uint32_t grinding_factor, uint64_t nonce_begin,
                              uint64_t max_nonces, uint64_t *nonces_out, uint8_t *new_seeds_out, uint8_t *found_out) {
    if (!ctx) return fail(WF_ERR_ARG, "ctx is null");
    if (!seeds || !nonces_out || !new_seeds_out || !found_out) return fail(WF_ERR_ARG, "null argument");
    if (n_seeds < 1 || n_seeds > 256) return fail(WF_ERR_ARG, "n_seeds must be 1..256, got %zu", n_seeds);
    if (grinding_factor > 32) return fail(WF_ERR_ARG, "grinding_factor must be at most 32, got %u", grinding_factor);
    if (max_nonces == 0) return fail(WF_ERR_ARG, "max_nonces is 0: there is no nonce to test");
    int rc = check_hasher_pair(ctx->hasher, ctx->digest_bytes);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    WF_ENTER(ctx, st);
    const GrindLayout L(n_seeds);
    if ((rc = ensure(ctx, ctx->grind, L.bytes))) return rc;
    if (ctx->qpin_cap < L.bytes) {
        if (ctx->qpin) (void)hipHostFree(ctx->qpin);
        ctx->qpin = nullptr;
        ctx->qpin_cap = 0;
        const size_t want = std::max<size_t>(L.bytes, (size_t)1 << 20);
        if (hipHostMalloc(&ctx->qpin, want, hipHostMallocDefault) != hipSuccess)
            return fail(WF_ERR_HIP, "hipHostMalloc failed: %s", hipGetErrorString(hipGetLastError()));
        ctx->qpin_cap = want;
    }
    char *dev = (char *)ctx->grind.p, *pin = (char *)ctx->qpin;
    // a 24-byte digest sits in front of its slot with zeros behind: whatever the caller left there is not part of the seed
    for (size_t i = 0; i < n_seeds; i++) {
        memcpy(pin + L.seeds + i * 32, seeds + i * 32, ctx->digest_bytes);
        memset(pin + L.seeds + i * 32 + ctx->digest_bytes, 0, 32 - ctx->digest_bytes);
    }
    memset(pin + L.best, 0xFF, n_seeds * 8);
    HIP_TRY(hipMemcpyAsync(dev, pin, L.nonces, hipMemcpyHostToDevice, st));
    GrindPlan plan = hasher_row(ctx->hasher)->grind;
    if (ctx->tune.grind_window_cap_log2) plan.cap_log2 = ctx->tune.grind_window_cap_log2;
    if (ctx->tune.grind_window_log2) plan.first_log2 = ctx->tune.grind_window_log2;
    plan.first_log2 = std::min(plan.first_log2, plan.cap_log2);
    const uint32_t n = (uint32_t)n_seeds;
    rc = dispatch_hasher(ctx->hasher, ctx->digest_bytes, [&](auto tag) {
        typedef typename GrindOf<typename decltype(tag)::Merge>::type G;
        return grind_run<G>(ctx, st, dev, pin, L, n, grinding_factor, nonce_begin, max_nonces, plan);
    });
    if (rc) return rc;
    memcpy(nonces_out, pin + L.nonces, n_seeds * 8);
    memcpy(new_seeds_out, pin + L.new_seeds, n_seeds * 32);
    memcpy(found_out, pin + L.found, n_seeds);
    return 0;
}
