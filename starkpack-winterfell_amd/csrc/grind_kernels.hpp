// The nonce search of ProverChannel::grind_query_seed (prover/src/channel.rs:182-198): for every seed the SMALLEST nonce of a
// window whose merge_with_int(seed, nonce) has the asked number of trailing zero bits in its first little-endian u64
// (DefaultRandomCoin::check_leading_zeros, crypto/src/random/default.rs:181-186).  One kernel template over a per-hasher
// policy, like the tree kernels over their Merge and the row kernel over its Absorb:
//   G::prepare(slot, seed)      the seed's 32-byte slot (four u64 words, as they arrive) -> what the loop keeps of it
//   G::wave_uniform(seed)       called where every lane of the wave holds the same seed: may move it to scalar registers
//   G::head32(seed, nonce)      the low 32 bits of the digest's first u64: grinding factors end at 32 (air/src/options.rs:22),
//                               so this is all the test reads and the compiler drops whatever else the last round produces
//   G::digest(seed, nonce, out) the whole digest as four u64 words of a 32-byte slot (k_grind_finish)
// No memory traffic beyond the seed (wave-uniform: scalar loads), one relaxed load of best[] per iteration and one atomic
// per wave that found something.
#pragma once
#include "grind_plan.hpp"
#include "hasher_dispatch.hpp"

namespace wf {

template <int DW>
struct GrindBlake3 {  // Blake3_256 (DW = 8) / Blake3_192 (DW = 6)
    struct Seed {
        uint32_t w[8];
    };
    static __device__ __forceinline__ void prepare(const uint64_t *slot, Seed &s) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            s.w[2 * i] = (uint32_t)slot[i];
            s.w[2 * i + 1] = (uint32_t)(slot[i] >> 32);
        }
    }
    static __device__ __forceinline__ void wave_uniform(Seed &) {}
    static __device__ __forceinline__ uint32_t head32(const Seed &s, uint64_t nonce) {
        uint32_t d[8];
        b3::merge_with_int<DW>(s.w, nonce, d);
        return d[0];
    }
    static __device__ __forceinline__ void digest(const Seed &s, uint64_t nonce, uint64_t (&out)[4]) {
        uint32_t d[8];
        b3::merge_with_int<DW>(s.w, nonce, d);
#pragma unroll
        for (int i = 0; i < 4; i++) out[i] = ((uint64_t)d[2 * i + 1] << 32) | d[2 * i];
    }
};

struct GrindSha3 {
    struct Seed {
        uint64_t w[4];
    };
    static __device__ __forceinline__ void prepare(const uint64_t *slot, Seed &s) {
#pragma unroll
        for (int i = 0; i < 4; i++) s.w[i] = slot[i];
    }
    static __device__ __forceinline__ void wave_uniform(Seed &) {}
    static __device__ __forceinline__ uint32_t head32(const Seed &s, uint64_t nonce) {
        uint64_t d[4];
        k3::merge_with_int(s.w, nonce, d);
        return (uint32_t)d[0];
    }
    static __device__ __forceinline__ void digest(const Seed &s, uint64_t nonce, uint64_t (&out)[4]) {
        k3::merge_with_int(s.w, nonce, out);
    }
};

// The element-digest hashers (Rp64_256, RpJive64_256, GriffinJive64_256), each in its one-lane-per-permutation form, as the
// row and wide-level kernels; M = the hasher's Merge.  The seed's words are read as BaseElement::new reads them (reduced mod p)
// and kept as Montgomery residues; M::merge_with_int_mont is the hasher's merge_with_int on such a seed (Rp64_256: the sponge
// of seed || nonce; the Jive hashers: the compression of seed || nonce); the test reads the CANONICAL value of digest element
// 0 (ElementDigest::as_bytes).
template <class M>
struct GrindElem {
    struct Seed {
        uint64_t w[4];
    };
    static __device__ __forceinline__ void prepare(const uint64_t *slot, Seed &s) {
#pragma unroll
        for (int i = 0; i < 4; i++) s.w[i] = rp::elem_new(slot[i]);
    }
    // the conversion is vector arithmetic on words that the scalar unit loaded: where every lane holds the same seed
    // (k_grind) the residues go back to scalar registers
    static __device__ __forceinline__ void wave_uniform(Seed &s) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)s.w[i]), hi = __builtin_amdgcn_readfirstlane((uint32_t)(s.w[i] >> 32));
            s.w[i] = ((uint64_t)hi << 32) | lo;
        }
    }
    static __device__ __forceinline__ uint32_t head32(const Seed &s, uint64_t nonce) {
        uint64_t d[4];
        M::merge_with_int_mont(s.w, nonce, d);
        return (uint32_t)d[0];
    }
    static __device__ __forceinline__ void digest(const Seed &s, uint64_t nonce, uint64_t (&out)[4]) {
        M::merge_with_int_mont(s.w, nonce, out);
    }
};
// (named structs: k_grind / k_grind_finish are instantiated on, and their traces keyed by, these names)
struct GrindRp64 : GrindElem<rp::Merge> {};
struct GrindRpJive : GrindElem<rpj::Merge> {};
struct GrindGriffin : GrindElem<gfj::Merge> {};

// The search policy of a hasher, by its Merge (the tag of dispatch_hasher carries that).
template <class M> struct GrindOf;
template <int DW> struct GrindOf<b3::Merge<DW>> { typedef GrindBlake3<DW> type; };
template <> struct GrindOf<k3::Merge> { typedef GrindSha3 type; };
template <> struct GrindOf<rp::Merge> { typedef GrindRp64 type; };
template <> struct GrindOf<rpj::Merge> { typedef GrindRpJive type; };
template <> struct GrindOf<gfj::Merge> { typedef GrindGriffin type; };

constexpr uint32_t GRIND_THREADS = 256;
constexpr uint64_t GRIND_NONE = ~(uint64_t)0;  // best[seed] before anything is found

static __device__ __forceinline__ uint64_t grind_best(const uint64_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One window [base, base + count) for every seed (blockIdx.y); base + count - 1 <= 2^64 - 1 (grind_next_window).  With T
// lanes in a row of the grid, lane t tests base + t + i T for i < GRIND_LANE_ITERS (grind_groups sizes the grid so that this
// covers the window) and never a nonce at or beyond base + count.  mask = 2^g - 1: a nonce qualifies when (head & mask) == 0.
//
// The loop is bounded by GRIND_LANE_ITERS and waits for nothing: every launch finishes, whatever it finds.  Everything that
// ends it early is wave-uniform and only saves work:
//   - a lane's nonces grow with i, and every nonce of iteration i + 1 of a wave is above every nonce of its iteration i: the
//     wave stops behind the first iteration in which one of its lanes qualifies;
//   - `seen` is a relaxed look at best[seed], taken one iteration ahead of its use (the load's latency runs under the hash):
//     a lane whose nonce is above it cannot lower it any more.  A stale value only means a hash more; a window that lies
//     above an answer already found ends in front of its first hash.
// The result goes through a minimum over the wave and one agent-scope atomicMin per wave, so the smallest qualifying nonce
// wins whatever the order of waves -- the serial reference's (1..u64::MAX).find, not the concurrent find_any.
template <class G>
__global__ void __launch_bounds__(GRIND_THREADS) k_grind(const uint64_t *__restrict__ seeds, uint64_t *best, uint64_t base,
                                                         uint64_t count, uint32_t mask) {
    const uint32_t s = blockIdx.y;
    typename G::Seed seed;
    G::prepare(seeds + (uint64_t)s * 4, seed);
    G::wave_uniform(seed);
    const uint64_t T = (uint64_t)gridDim.x * GRIND_THREADS;
    uint64_t off = (uint64_t)blockIdx.x * GRIND_THREADS + threadIdx.x;
    uint64_t found = GRIND_NONE, seen = grind_best(best + s);
#pragma unroll 1
    for (uint32_t i = 0; i < GRIND_LANE_ITERS; i++, off += T) {
        const uint64_t nonce = base + off;  // (wraps only in a lane that is not `live`)
        const bool live = off < count && !(seen < nonce);
        if (!__any(live)) break;
        seen = grind_best(best + s);
        const bool hit = live && (G::head32(seed, nonce) & mask) == 0;
        if (hit) found = nonce;
        if (__any(hit)) break;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint64_t o = __shfl_xor(found, d, 64);
        found = o < found ? o : found;
    }
    if ((threadIdx.x & 63) == 0 && found != GRIND_NONE)
        __hip_atomic_fetch_min(best + s, found, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One lane per seed: the outputs of the call.  new_seeds[i] = merge_with_int(seed_i, nonce_i), the coin's seed after
// reseed_with_int, as a 32-byte slot.  A nonce of 2^64 - 1 cannot be told from "nothing found" in best[]: when the searched
// range ends there (last_in_range) and best[] is still all ones, that one nonce is tested here.
template <class G>
__global__ void __launch_bounds__(GRIND_THREADS) k_grind_finish(const uint64_t *__restrict__ seeds, const uint64_t *__restrict__ best,
                                                                uint32_t n_seeds, uint32_t mask, uint32_t last_in_range,
                                                                uint64_t *__restrict__ nonces, uint64_t *__restrict__ new_seeds,
                                                                uint8_t *__restrict__ found_out) {
    const uint32_t i = blockIdx.x * GRIND_THREADS + threadIdx.x;
    if (i >= n_seeds) return;
    typename G::Seed seed;
    G::prepare(seeds + (uint64_t)i * 4, seed);
    const uint64_t nonce = best[i];
    uint64_t d[4];
    G::digest(seed, nonce, d);
    const bool found = nonce != GRIND_NONE || (last_in_range && ((uint32_t)d[0] & mask) == 0);
    nonces[i] = found ? nonce : 0;
#pragma unroll
    for (int k = 0; k < 4; k++) new_seeds[(uint64_t)i * 4 + k] = found ? d[k] : 0;
    found_out[i] = found ? 1 : 0;
}

}  // namespace wf
