// SHA3-256 (FIPS 202) for the second hasher of the commitment path: Sha3_256::hash_elements / merge of the reference
// (crypto/src/hash/sha/mod.rs:17-57).  Host- and device-compilable like field.hpp (tests/cpp/test_keccak_host.cpp runs it
// under plain g++ against hashlib).
//
//   Keccak-f[1600]: 24 rounds, fully unrolled (the round is a template over its index: every rotation count and round
//   constant is an immediate), the 25 lanes in registers as uint64_t.
//   Sponge: rate 136 bytes = 17 lanes, domain byte 0x06 behind the message, 0x80 in the last byte of the rate block,
//   digest = lanes 0..3 little endian.
//
// Everything the library hashes is a whole number of 8-byte lanes (field elements, digests), so absorption is lane-granular:
// sha3_256_lanes pulls the message lane by lane from a callable.  sha3_256_bytes (any byte length) exists for the host test.
#pragma once
#include "field.hpp"

namespace wf {
namespace k3 {

constexpr int RATE_LANES = 17;  // 136 bytes

constexpr uint64_t round_constant(int i) {
    constexpr uint64_t rc[24] = {
        0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull, 0x000000000000808bull,
        0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008aull, 0x0000000000000088ull,
        0x0000000080008009ull, 0x000000008000000aull, 0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull,
        0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800aull, 0x800000008000000aull,
        0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
    return rc[i];
}

// Rotation of a lane by a compile-time count.  On the device a 64-bit rotate is two v_alignbit_b32, one per 32-bit half
// (the compiler's own expansion of the shift-or form is 64-bit shifts and ors: docs/EXPERIMENTS.md has both counts);
// a rotation by 32 is a swap of the halves and costs nothing.  WF_KECCAK_PLAIN_ROT keeps the shift-or form (the "before").
template <int N>
WF_HD uint64_t rotl(uint64_t x) {
    static_assert(N > 0 && N < 64, "rotation count");
#if defined(__HIP_DEVICE_COMPILE__) && !defined(WF_KECCAK_PLAIN_ROT)
    const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
    // alignbit(a, b, s) = low 32 bits of ((a:b) >> s)
    if constexpr (N == 32) {
        return ((uint64_t)lo << 32) | hi;
    } else if constexpr (N < 32) {
        const uint32_t nh = __builtin_amdgcn_alignbit(hi, lo, 32 - N), nl = __builtin_amdgcn_alignbit(lo, hi, 32 - N);
        return ((uint64_t)nh << 32) | nl;
    } else {
        const uint32_t nh = __builtin_amdgcn_alignbit(lo, hi, 64 - N), nl = __builtin_amdgcn_alignbit(hi, lo, 64 - N);
        return ((uint64_t)nh << 32) | nl;
    }
#else
    return (x << N) | (x >> (64 - N));
#endif
}

template <int R>
WF_HD void keccak_round(uint64_t (&s)[25]) {
    // theta
    uint64_t c[5];
#pragma unroll
    for (int x = 0; x < 5; x++) c[x] = s[x] ^ s[x + 5] ^ s[x + 10] ^ s[x + 15] ^ s[x + 20];
#pragma unroll
    for (int x = 0; x < 5; x++) {
        const uint64_t d = c[(x + 4) % 5] ^ rotl<1>(c[(x + 1) % 5]);
#pragma unroll
        for (int y = 0; y < 25; y += 5) s[y + x] ^= d;
    }
    // rho and pi: one chain through the 24 lanes other than lane 0
    uint64_t t = s[1], u;
#define WF_K3_STEP(J, N) u = s[J]; s[J] = rotl<N>(t); t = u;
    WF_K3_STEP(10, 1) WF_K3_STEP(7, 3) WF_K3_STEP(11, 6) WF_K3_STEP(17, 10) WF_K3_STEP(18, 15) WF_K3_STEP(3, 21)
    WF_K3_STEP(5, 28) WF_K3_STEP(16, 36) WF_K3_STEP(8, 45) WF_K3_STEP(21, 55) WF_K3_STEP(24, 2) WF_K3_STEP(4, 14)
    WF_K3_STEP(15, 27) WF_K3_STEP(23, 41) WF_K3_STEP(19, 56) WF_K3_STEP(13, 8) WF_K3_STEP(12, 25) WF_K3_STEP(2, 43)
    WF_K3_STEP(20, 62) WF_K3_STEP(14, 18) WF_K3_STEP(22, 39) WF_K3_STEP(9, 61) WF_K3_STEP(6, 20) WF_K3_STEP(1, 44)
#undef WF_K3_STEP
    // chi
#pragma unroll
    for (int y = 0; y < 25; y += 5) {
        uint64_t b[5];
#pragma unroll
        for (int x = 0; x < 5; x++) b[x] = s[y + x];
#pragma unroll
        for (int x = 0; x < 5; x++) s[y + x] = b[x] ^ (~b[(x + 1) % 5] & b[(x + 2) % 5]);
    }
    // iota
    s[0] ^= round_constant(R);
}

template <int R>
WF_HD void rounds_from(uint64_t (&s)[25]) {
    if constexpr (R < 24) {
        keccak_round<R>(s);
        rounds_from<R + 1>(s);
    }
}

WF_HD void keccak_f(uint64_t (&s)[25]) { rounds_from<0>(s); }

// Sha3_256::merge: SHA3-256 of two digests = 64 message bytes in lanes 0..7, the padding in the same (only) block.
WF_HD void sha3_merge(const uint64_t (&in)[8], uint64_t (&out)[4]) {
    uint64_t s[25];
#pragma unroll
    for (int i = 0; i < 8; i++) s[i] = in[i];
    s[8] = 0x06;
#pragma unroll
    for (int i = 9; i < 25; i++) s[i] = 0;
    s[16] = 0x80ull << 56;
    keccak_f(s);
#pragma unroll
    for (int i = 0; i < 4; i++) out[i] = s[i];
}

// Sha3_256::merge_with_int (sha/mod.rs:32-37): SHA3-256 of the seed's 32 bytes followed by the value as 8 little-endian
// bytes = five message lanes, the padding in the same block.
WF_HD void merge_with_int(const uint64_t (&seed)[4], uint64_t value, uint64_t (&out)[4]) {
    uint64_t s[25];
#pragma unroll
    for (int i = 0; i < 4; i++) s[i] = seed[i];
    s[4] = value;
    s[5] = 0x06;
#pragma unroll
    for (int i = 6; i < 25; i++) s[i] = 0;
    s[16] = 0x80ull << 56;
    keccak_f(s);
#pragma unroll
    for (int i = 0; i < 4; i++) out[i] = s[i];
}

// SHA3-256 of a message of n_lanes 8-byte lanes; next() returns them in order (each a little-endian 64-bit word of the
// message).  One permutation call site: the loop runs once per rate block, the last block carries the padding -- a message
// that fills its last block exactly (n_lanes a multiple of 17) gets a further block that holds only the padding.  State
// lanes are addressed with compile-time indices only (the unrolled loop compares against the count), so they stay in
// registers.
template <class Next>
WF_HD void sha3_256_lanes(uint64_t n_lanes, Next &&next, uint64_t (&out)[4]) {
    uint64_t s[25];
#pragma unroll
    for (int i = 0; i < 25; i++) s[i] = 0;
    uint64_t rem = n_lanes;
    for (;;) {
        const bool last = rem < (uint64_t)RATE_LANES;
        const uint32_t take = last ? (uint32_t)rem : (uint32_t)RATE_LANES;
#pragma unroll
        for (int i = 0; i < RATE_LANES; i++) {
            if ((uint32_t)i < take) s[i] ^= next();
            else if ((uint32_t)i == take) s[i] ^= 0x06;  // (only reached in the last block: take == 17 otherwise)
        }
        if (last) s[16] ^= 0x80ull << 56;
        keccak_f(s);
        if (last) break;
        rem -= RATE_LANES;
    }
#pragma unroll
    for (int i = 0; i < 4; i++) out[i] = s[i];
}

// The hasher as the tree kernels (Merge) and the lane-per-row leaf kernel (Absorb) of the *_kernels.hpp headers take it:
// digests are four 64-bit words; the message lanes are the canonical values of the elements.
struct Merge {
    using W = uint64_t;
    static constexpr int NW = 4;
    static constexpr bool HAS_QUAD = false;
    static WF_HD void merge(const W (&in)[2 * NW], W (&out)[NW]) { sha3_merge(in, out); }
};
struct Absorb {
    static constexpr bool CANONICAL = true;
    template <class Next>
    static WF_HD void absorb(uint64_t n_lanes, Next &&next, uint64_t (&out)[4]) { sha3_256_lanes(n_lanes, next, out); }
};

// Any byte length (host test only: the library itself never hashes a partial lane).
static inline void sha3_256_bytes(const unsigned char *msg, size_t len, unsigned char digest[32]) {
    uint64_t s[25] = {0};
    unsigned char block[136];
    for (;;) {
        const bool last = len < 136;
        const size_t take = last ? len : 136;
        for (size_t i = 0; i < 136; i++) block[i] = i < take ? msg[i] : 0;
        if (last) {
            block[take] ^= 0x06;
            block[135] ^= 0x80;
        }
        for (int i = 0; i < RATE_LANES; i++) {
            uint64_t w = 0;
            for (int b = 7; b >= 0; b--) w = (w << 8) | block[8 * i + b];
            s[i] ^= w;
        }
        keccak_f(s);
        if (last) break;
        msg += 136;
        len -= 136;
    }
    for (int i = 0; i < 4; i++)
        for (int b = 0; b < 8; b++) digest[8 * i + b] = (unsigned char)(s[i] >> (8 * b));
}

}  // namespace k3
}  // namespace wf
