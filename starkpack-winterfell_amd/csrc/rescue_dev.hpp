// Rp64_256 (Rescue Prime over p = 2^64 - 2^32 + 1) for the third hasher of the commitment path: Rp64_256::hash_elements /
// merge of the reference (crypto/src/hash/rescue/rp64_256/mod.rs).  Host- and device-compilable like field.hpp and
// keccak_dev.hpp (tests/cpp/test_rescue_host.cpp runs it under plain g++ against tests/rp64_util.py).
//
//   State: 12 elements of F64 (Montgomery residues, the library's in-memory form), capacity 0..4, rate 4..12, digest 4..8.
//   Permutation: 7 rounds of  x^7 | MDS | + ARK1[r] | x^(1/7) | MDS | + ARK2[r];  x^(1/7) = x^10540996611094048183 by the
//   addition chain below: 72 products, so a permutation is 7 * 12 * 76 = 6384 field products plus 14 MDS products.
//   MDS: circulant, out[i] = sum_k ROW[k] * in[(i + k) mod 12] (the same sum as sum_j ROW[(j - i) mod 12] * in[j]).  The
//   entries are at most 26 and sum to 160, so a row product is 24 small multiply-adds into two 64-bit accumulators (low and
//   high words of the inputs apart) and ONE reduction; the coefficients are plain integers, which keeps the Montgomery form.
//   Sponge: state[0] = the number of base elements hashed, elements added into the rate eight at a time, a permutation
//   behind every full block and behind a partial last block; no other padding.  merge = hash_elements of the 8 digest
//   elements (state[0] = 8).  A digest leaves the library as 4 canonical little-endian u64 (ElementDigest::as_bytes) and
//   digest words coming in are read as BaseElement::new reads them (any u64, reduced mod p).
//
// Two forms of the permutation:
//   permute()       one lane per permutation: the state in 24 VGPRs, the rounds and the long squaring runs as rolled loops
//                   (the fully unrolled permutation would be ~1 MB of code), the inverse S-box on GROUP elements at a time
//                   so that independent carry chains interleave; the state is rotated by GROUP places per step, which keeps
//                   every index a compile-time constant (no scratch).
//   permute_lane()  one state element per lane, groups of 16 lanes with 12 active: the S-boxes are the same code on one
//                   element, the MDS gathers the other elements of the group (ds_bpermute on the device).  One twelfth of
//                   the serial chain: for tree levels too narrow to fill the chip.
// The round constants are the published parameters of the function in Montgomery form (x * 2^64 mod p);
// tests/test_rescue_host.py pins them to tests/golden/rp64_256_params.json, scripts/gen_rp64_fixtures.py --header prints them.
#pragma once
#include "field.hpp"
#include "merkle_plan.hpp"

namespace wf {
namespace rp {

constexpr int STATE = 12, RATE = 8, RATE_AT = 4, DIGEST = 4, ROUNDS = 7;
#ifndef WF_RP64_GROUP
#define WF_RP64_GROUP 2  // (2, 3 and 4 are measured in docs/EXPERIMENTS.md)
#endif
constexpr int GROUP = WF_RP64_GROUP;  // elements of the inverse S-box walked together in permute(); STATE % GROUP == 0

constexpr uint32_t mds_coef(int k) {
    constexpr uint32_t row[STATE] = {7, 23, 8, 26, 13, 10, 9, 7, 6, 22, 21, 8};
    return row[k];
}

// ARK1 (half 0) / ARK2 (half 1) of round r for state element i.  r (and in the lane form i) is a run-time index: the table
// is a constant in memory (scalar loads where the index is uniform).
WF_HD uint64_t ark(int half, int r, uint32_t i) {
    constexpr uint64_t t[2][ROUNDS][STATE] = {
        {   // ARK1
            {0x3f05bc91ffd5316full, 0xd4bc8d4e4d2ff139ull, 0xed513ba9d10ab322ull, 0xf15414058310b66eull,
             0x71f566fb05f8eca9ull, 0x6eb551ebb7df3286ull, 0xe08fab9d929232abull, 0xcae6b66577f91c3bull,
             0x4d88558f9237eb1cull, 0xfec7d213f8aea764ull, 0xd4f885b5afec945full, 0x804371c6ed8bacf9ull},
            {0x583875b0dd8cdbb6ull, 0x42c884ae3a226dd0ull, 0xac7929b4f8686c3aull, 0xa7f1687da8425ab7ull,
             0xfbe31a86a047727aull, 0xb20eecb8a92544b4ull, 0xb450b28f532d53dbull, 0x4afa6d28a3d9fcdaull,
             0xdd3749edc4001829ull, 0xa5c8bf243c846750ull, 0xb08a571838eab47dull, 0xc319607d3c319886ull},
            {0x56ca1c4bc72b0531ull, 0xa71e24d6a060cc0aull, 0x7b3be59ecb363407ull, 0x334ec938c4349c7eull,
             0x4b1411ca02617b4dull, 0x410f62fe14aa9991ull, 0xc1d9ad86cbec6c13ull, 0xb2d2866e924a885bull,
             0x779b93befb287f03ull, 0x1dd1769c12b0479cull, 0xcd3daa47e11fd4b5ull, 0xaeea1583558c77f5ull},
            {0xcadcd8ece0cd653aull, 0xff57abf8990992a3ull, 0xaee29b8a04a7e26dull, 0xa5d15d768e48875bull,
             0x82a9e9d0c9328926ull, 0xfb9ad100f1814675ull, 0xdf12422fcc5baa01ull, 0xd4caf605e44788e4ull,
             0x0d1b6fc27bd8bf3full, 0xca3132bbb494d2d2ull, 0x94d0d2337fbe8798ull, 0x9587068f1ab5ea28ull},
            {0x96a5e3f9ab7205a4ull, 0xa1305ab85e8a8f78ull, 0x44d828cbd4861db1ull, 0x79ccf88182569277ull,
             0x075d20a8b34915f6ull, 0x92eb1cb362387b39ull, 0x59ac1beac266f278ull, 0xee8b348886cdafe0ull,
             0x9de0619f79925dbfull, 0xf8091d2eeac4783bull, 0xfda7951a240a92b2ull, 0xd3302a85d2e2e071ull},
            {0x6a3106b7d41b5210ull, 0x89ce3255ef8a7665ull, 0xbb878c5945b622d3ull, 0x8e435eda47b1da33ull,
             0x1878cbccce6b32ceull, 0xf99d7a1d5979ff34ull, 0xd67cd480832f8f2dull, 0x7cc878bad0a057dbull,
             0x645dfbe02e62650aull, 0x95613650d634be9bull, 0x20e2e7516723e77dull, 0x8c89044b5fb7c171ull},
            {0x79c6850691b460daull, 0x27280b3c832aa04dull, 0xe3b7f0e64b448a32ull, 0xf78ccbe5c9f2a851ull,
             0x3f0d224c20d1d225ull, 0x4e69a7220043b0cfull, 0x1d17daefeb49bb9eull, 0x2dfa643b177b1ca1ull,
             0xe8c11c0bc4a9b82cull, 0x3de3d60ed5a05279ull, 0x7ece5514073da985ull, 0xb5e0be78e2fea57full},
        },
        {   // ARK2
            {0xad8f4217e39132ceull, 0xf75e2b4e90bc20ebull, 0x62aeeb6e434513f6ull, 0x7add4628388ab1f9ull,
             0xcf706afc07504d21ull, 0x025b035a2eddfef3ull, 0x8e143a04ad68f9eaull, 0x7de7fc5c2f3f3e67ull,
             0x8d718ebf2b8e9437ull, 0x91ebe0f1c5e1395eull, 0xef4993ea1f2d521cull, 0xb26d63db27d9be51ull},
            {0x41e99fb19b988ab1ull, 0x275a53bc11607b9bull, 0x8cead63f44e93d14ull, 0xb181d3e2fb331864ull,
             0x6fa7b59d9e9b0125ull, 0x99c88f95c24f54a3ull, 0x16b19d251be14c08ull, 0xf22b0e2703656f31ull,
             0x4ff71f402d70391dull, 0xcd19c3e84f3a04cbull, 0x5796ab54491b81b8ull, 0x1a71babb23839469ull},
            {0x06f8103c683086c4ull, 0x855352fac2f78d85ull, 0x1fda04d1d6df9346ull, 0xa7988c0f374c60a4ull,
             0x58fb6320713eef30ull, 0x241b5425282461baull, 0x911f457e537f4785ull, 0xe26dd6c15b470e49ull,
             0xc807ce192a6b6758ull, 0x8776a02d03ddb3b0ull, 0x7587568d85c50dafull, 0xd2be5045f2db1df1ull},
            {0x759fffdd6aac357eull, 0xd80c33f2e97ecad6ull, 0x046f6154c462b9a1ull, 0x9806e0d343d85c50ull,
             0x0920a719a6eecbc3ull, 0xdeec635ef8ab9a15ull, 0x15649638eb08dae3ull, 0xcc1f063bd1db9a2bull,
             0xd57d19ec43c71294ull, 0xcde946672fd1e880ull, 0xe4f7a8787a1aeb59ull, 0x3c5d83929a529ed9ull},
            {0x9f64ebbc8f305e23ull, 0x1ab28cb6b4c65e1aull, 0xf6bcb87e9143e781ull, 0x19980c74c443f5e9ull,
             0x4d27fa417c19b8b3ull, 0xf672da693c69ff48ull, 0xf817f0b5e03f4b51ull, 0x9d144d03ece257d7ull,
             0x6748f87e9ecd39e7ull, 0xa1fcf662540474caull, 0xdb0c05c3c345a822ull, 0x1ea370a5668bf215ull},
            {0x08a064250583a8d4ull, 0x1ee57776d1030144ull, 0x70aba5249644ffb5ull, 0x4c8b5e815b7cb65eull,
             0xd7939f0e32922402ull, 0x2f1f419d96779529ull, 0x3d2175e616f8e26aull, 0x75e6973dff2bd7a9ull,
             0x3bf34b4c76cdf12full, 0xa390ac3baeaed4cfull, 0xb563a74e059a4f2dull, 0x3ac1aed4779181baull},
            {0x782f2dbe89501715ull, 0xdf3223a61f34d7b3ull, 0xc771ab08fb1cba5eull, 0x0a5d0c235e7f511cull,
             0x15f62b0187952168ull, 0x3623021a63ec45f4ull, 0xd125955ed002cdb0ull, 0xefc5109a4de6f163ull,
             0xd58541e54d473814ull, 0xd446c6bd7b3c43d5ull, 0x3f44fcb98767bc3bull, 0xca0b3634cb030873ull},
        },
    };
    return t[half][r][i];
}

WF_HD uint64_t sq(uint64_t x) { return F64::mul(x, x); }

WF_HD uint64_t pow7(uint64_t x) {
    const uint64_t x2 = sq(x), x3 = F64::mul(x2, x), x4 = sq(x2);
    return F64::mul(x4, x3);
}

// base^(2^N) * tail on G independent elements
template <int N, int G>
WF_HD void exp_acc(const uint64_t (&base)[G], const uint64_t (&tail)[G], uint64_t (&out)[G]) {
    uint64_t t[G];
#pragma unroll
    for (int g = 0; g < G; g++) t[g] = base[g];
    if constexpr (N <= 3) {
#pragma unroll
        for (int k = 0; k < N; k++) {
#pragma unroll
            for (int g = 0; g < G; g++) t[g] = sq(t[g]);
        }
    } else {
#pragma unroll 1
        for (int k = 0; k < N; k++) {
#pragma unroll
            for (int g = 0; g < G; g++) t[g] = sq(t[g]);
        }
    }
#pragma unroll
    for (int g = 0; g < G; g++) out[g] = F64::mul(t[g], tail[g]);
}

// x^10540996611094048183 (= x^(1/7)) on G independent elements; the exponent in binary is
// 1001001001001001001001001001000110110110110110110110110110110111, built from runs of "100" and "110".
template <int G>
WF_HD void inv_sbox(uint64_t (&x)[G]) {
    uint64_t t1[G], t2[G], t3[G], t4[G], t5[G], t6[G], t7[G];
#pragma unroll
    for (int g = 0; g < G; g++) {
        t1[g] = sq(x[g]);   // 10
        t2[g] = sq(t1[g]);  // 100
    }
    exp_acc<3, G>(t2, t2, t3);    // 100100
    exp_acc<6, G>(t3, t3, t4);    // (100)^4
    exp_acc<12, G>(t4, t4, t5);   // (100)^8
    exp_acc<6, G>(t5, t3, t6);    // (100)^10
    exp_acc<31, G>(t6, t6, t7);   // (100)^10 0 (100)^10
#pragma unroll
    for (int g = 0; g < G; g++) {
        const uint64_t a = sq(sq(F64::mul(sq(t7[g]), t6[g])));
        const uint64_t b = F64::mul(F64::mul(t1[g], t2[g]), x[g]);
        x[g] = F64::mul(a, b);
    }
}

// One row of the MDS product, get(j) = state element j: sum_k ROW[k] * get((i + k) mod 12), reduced once.  With
// lo = sum ROW[k] * low word and hi = sum ROW[k] * high word (both < 160 * 2^32) the sum is
//     lo + (hi mod 2^32) * 2^32 + (hi >> 32) * 2^64,   2^64 = 2^32 - 1 (mod p):
// b = (hi mod 2^32) << 32 <= ffffffff00000000 < p and a = lo + (hi >> 32) * (2^32 - 1) < 2^41, so one canonical addition ends it.
template <class Get>
WF_HD uint64_t mds_row(uint32_t i, Get &&get) {
    uint64_t lo = 0, hi = 0;
#pragma unroll
    for (int k = 0; k < STATE; k++) {
        uint32_t j = i + (uint32_t)k;
        j -= j >= (uint32_t)STATE ? (uint32_t)STATE : 0u;
        const uint64_t v = get(j);
        lo += (uint64_t)mds_coef(k) * (uint32_t)v;
        hi += (uint64_t)mds_coef(k) * (uint32_t)(v >> 32);
    }
    const uint64_t top = hi >> 32;
    return F64::add(hi << 32, lo + ((top << 32) - top));
}

// ------------------------------------------------------------------------------------ form 1: one lane per permutation
WF_HD void mds_ark(uint64_t (&s)[STATE], int half, int r) {
    uint64_t o[STATE];
#pragma unroll
    for (int i = 0; i < STATE; i++) o[i] = mds_row((uint32_t)i, [&](uint32_t j) { return s[j]; });
#pragma unroll
    for (int i = 0; i < STATE; i++) s[i] = F64::add(o[i], ark(half, r, (uint32_t)i));
}

WF_HD void permute(uint64_t (&s)[STATE]) {
#pragma unroll 1
    for (int r = 0; r < ROUNDS; r++) {
#pragma unroll
        for (int i = 0; i < STATE; i++) s[i] = pow7(s[i]);
        mds_ark(s, 0, r);
#pragma unroll 1
        for (int it = 0; it < STATE / GROUP; it++) {  // GROUP elements per step, the state rotated by GROUP places
            uint64_t g[GROUP];
#pragma unroll
            for (int k = 0; k < GROUP; k++) g[k] = s[k];
            inv_sbox<GROUP>(g);
#pragma unroll
            for (int i = 0; i + GROUP < STATE; i++) s[i] = s[i + GROUP];
#pragma unroll
            for (int k = 0; k < GROUP; k++) s[STATE - GROUP + k] = g[k];
        }
        mds_ark(s, 1, r);
    }
}

// ------------------------------------------------------------------------------------ form 2: one state element per lane
// One half round of lane i (i < 12): the S-box on its own element is done by the caller (pow7 / inv_sbox<1>), this is the
// linear layer: get(j) returns element j of the same state.
template <class Get>
WF_HD uint64_t lane_mds_ark(uint32_t i, int half, int r, Get &&get) {
    return F64::add(mds_row(i, get), ark(half, r, i));
}

WF_HD uint64_t lane_inv_sbox(uint64_t x) {
    uint64_t g[1] = {x};
    inv_sbox<1>(g);
    return g[0];
}

#if defined(__HIPCC__)
// the 64-bit value x of wave lane src_lane (two ds_bpermute_b32; every lane of the wave must be active)
__device__ __forceinline__ uint64_t lane_value(uint64_t x, uint32_t src_lane) {
#if defined(__HIP_DEVICE_COMPILE__)
    const int addr = (int)(src_lane << 2);
    const uint32_t l = (uint32_t)__builtin_amdgcn_ds_bpermute(addr, (int)(uint32_t)x);
    const uint32_t h = (uint32_t)__builtin_amdgcn_ds_bpermute(addr, (int)(uint32_t)(x >> 32));
    return ((uint64_t)h << 32) | l;
#else
    return x;  // (the host pass of a HIP compilation only parses this)
#endif
}

// x = element i of the state held by the 16-lane group this lane belongs to (i = lane % 16; lanes 12..15 of a group carry
// no element: they run along on a clamped index and their result is ignored).  Every lane of the wave must be active.
__device__ __forceinline__ uint64_t permute_lane(uint64_t x) {
    const uint32_t lane = __lane_id();
    const uint32_t i = min(lane & 15u, (uint32_t)STATE - 1), base = lane & ~15u;
    auto get = [&](uint32_t j) { return lane_value(x, base + j); };
#pragma unroll 1
    for (int r = 0; r < ROUNDS; r++) {
        x = pow7(x);
        x = lane_mds_ark(i, 0, r, get);
        x = lane_inv_sbox(x);
        x = lane_mds_ark(i, 1, r, get);
    }
    return x;
}
#endif

// The same lane form on the host: the 12 lanes of one group in lockstep (what tests/cpp/test_rescue_host.cpp runs).
static inline void permute_lanes_host(uint64_t (&s)[STATE]) {
    uint64_t o[STATE];
    for (int r = 0; r < ROUNDS; r++) {
        for (int half = 0; half < 2; half++) {
            for (int i = 0; i < STATE; i++) s[i] = half == 0 ? pow7(s[i]) : lane_inv_sbox(s[i]);
            for (int i = 0; i < STATE; i++) o[i] = lane_mds_ark((uint32_t)i, half, r, [&](uint32_t j) { return s[j]; });
            for (int i = 0; i < STATE; i++) s[i] = o[i];
        }
    }
}

// ------------------------------------------------------------------------------------ sponge
// BaseElement::new(v) for any 64-bit v: v * 2^64 mod p (mont_reduce takes any product below p * 2^64)
WF_HD uint64_t elem_new(uint64_t v) { return F64::mul(v, F64::R2); }

// hash_elements of n base elements; next() returns them in order as Montgomery residues (the stored form).  One
// permutation call site; state elements are addressed with compile-time indices only.  out = the canonical digest words.
template <class Next>
WF_HD void hash_elements(uint64_t n, Next &&next, uint64_t (&out)[DIGEST]) {
    uint64_t s[STATE];
#pragma unroll
    for (int i = 0; i < STATE; i++) s[i] = 0;
    s[0] = elem_new(n);
    uint64_t rem = n;
    while (rem) {
        const uint32_t take = rem < (uint64_t)RATE ? (uint32_t)rem : (uint32_t)RATE;
#pragma unroll
        for (int i = 0; i < RATE; i++) {
            if ((uint32_t)i < take) s[RATE_AT + i] = F64::add(s[RATE_AT + i], next());
        }
        permute(s);
        rem -= take;
    }
#pragma unroll
    for (int i = 0; i < DIGEST; i++) out[i] = F64::to_canonical(s[RATE_AT + i]);
}

// merge: the digest words of the two children (4 + 4, as stored: canonical, or any u64 from a caller) -> canonical digest.
WF_HD void merge(const uint64_t (&in)[8], uint64_t (&out)[DIGEST]) {
    uint64_t s[STATE];
    s[0] = elem_new(RATE);
#pragma unroll
    for (int i = 1; i < RATE_AT; i++) s[i] = 0;
#pragma unroll
    for (int i = 0; i < RATE; i++) s[RATE_AT + i] = elem_new(in[i]);
    permute(s);
#pragma unroll
    for (int i = 0; i < DIGEST; i++) out[i] = F64::to_canonical(s[RATE_AT + i]);
}

// merge_with_int (rescue/rp64_256/mod.rs:194-215) on a seed already in Montgomery form (the search kernel converts its
// seed once): the seed in rate places 0..3, BaseElement::new(value) in place 4 and state[0] = 5 when value < p; otherwise
// value / p in place 5 as well and state[0] = 6.  p <= value < 2^64 < 2 p, so that quotient is 1.  Equal to hash_elements
// of those 5 or 6 elements.  out = the canonical digest words.
WF_HD void merge_with_int_mont(const uint64_t (&seed)[DIGEST], uint64_t value, uint64_t (&out)[DIGEST]) {
    const bool wide = value >= F64::P;
    uint64_t s[STATE];
    s[0] = elem_new(wide ? 6 : 5);
#pragma unroll
    for (int i = 1; i < RATE_AT; i++) s[i] = 0;
#pragma unroll
    for (int i = 0; i < DIGEST; i++) s[RATE_AT + i] = seed[i];
    s[RATE_AT + 4] = elem_new(value);
    s[RATE_AT + 5] = wide ? F64::one() : 0;
    s[RATE_AT + 6] = s[RATE_AT + 7] = 0;
    permute(s);
#pragma unroll
    for (int i = 0; i < DIGEST; i++) out[i] = F64::to_canonical(s[RATE_AT + i]);
}

// The same on the seed's digest words as stored (canonical, or any u64 from a caller: read as BaseElement::new reads them).
WF_HD void merge_with_int(const uint64_t (&seed)[DIGEST], uint64_t value, uint64_t (&out)[DIGEST]) {
    uint64_t m[DIGEST];
#pragma unroll
    for (int i = 0; i < DIGEST; i++) m[i] = elem_new(seed[i]);
    merge_with_int_mont(m, value, out);
}

// The hasher as the tree kernels (Merge) and the lane-per-row leaf kernel (Absorb) take it: digests are four canonical
// 64-bit words; the sponge absorbs the elements as they are stored (Montgomery residues), nothing is converted on the way in.
struct Merge {
    using W = uint64_t;
    static constexpr int NW = DIGEST;
    static constexpr bool HAS_QUAD = false;
    static WF_HD void merge(const W (&in)[2 * NW], W (&out)[NW]) { rp::merge(in, out); }
    static WF_HD void merge_with_int_mont(const W (&seed)[NW], uint64_t value, W (&out)[NW]) { rp::merge_with_int_mont(seed, value, out); }
};
struct Absorb {
    static constexpr bool CANONICAL = false;
    template <class Next>
    static WF_HD void absorb(uint64_t n, Next &&next, uint64_t (&out)[DIGEST]) { hash_elements(n, next, out); }
};

// The lane form's start value of a merge: element i of the state before the permutation (w = the digest word i - 4).
WF_HD uint64_t merge_lane_init(uint32_t i, uint64_t w) {
    return i == 0 ? elem_new(RATE) : (i >= (uint32_t)RATE_AT && i < (uint32_t)STATE) ? elem_new(w) : 0;
}

#if defined(__HIPCC__)
// The hasher as k_merkle_subtree_lanes (rescue_kernels.hpp) takes it: groups of 16 lanes, lane e holds state element e.
// Lanes 4..11 load / carry one digest word each, lane 0 the element count, lanes 12..15 nothing; lanes 4..7 end with the
// parent's digest word e - 4.  merge_lane runs inside the kernel's wave-uniform branch (every lane of the wave active),
// digest_word behind it.
struct Lanes {
    static constexpr const MerklePlan &PLAN = MERKLE_PLAN_RP64;
    static constexpr uint32_t LOG_LANES = 4, WORD_AT = RATE_AT, DIGEST_AT = RATE_AT;
    static __device__ __forceinline__ uint64_t merge_lane(uint32_t e, uint64_t w) { return permute_lane(merge_lane_init(e, w)); }
    static __device__ __forceinline__ uint64_t digest_word(uint64_t x) { return F64::to_canonical(x); }
};
#endif

}  // namespace rp
}  // namespace wf
