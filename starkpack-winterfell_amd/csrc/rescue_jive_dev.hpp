// RpJive64_256 (Rescue Prime of state width 8 over p = 2^64 - 2^32 + 1, 2-to-1 compression in Jive mode) for hasher 18 of
// the commitment path: RpJive64_256::hash_elements / merge / merge_with_int of the reference
// (crypto/src/hash/rescue/rp64_256_jive/mod.rs).  Host- and device-compilable like rescue_dev.hpp, whose S-boxes, element
// conversion and lane gather it reuses (tests/cpp/test_rpjive_host.cpp runs it under plain g++ against tests/rpjive_util.py).
//
//   State: 8 elements of F64 (Montgomery residues), capacity 0..4, rate 4..8, digest 4..8.
//   Permutation: 7 rounds of  x^7 | MDS | + ARK1[r] | x^(1/7) | MDS | + ARK2[r]:  7 * 8 * 76 = 4256 field products.
//   MDS: circulant, out[i] = sum_k ROW[k] * in[(i + k) mod 8] (the same sum as sum_j ROW[(j - i) mod 8] * in[j]); the entries
//   are at most 23 and sum to 96.
//   Sponge: state[0] = 1 iff the number of base elements is no multiple of 4 (NOT the count, as in Rp64_256); elements added
//   into the rate four at a time, a permutation behind every full block; behind a partial last block of i elements rate place
//   i is SET to 1 and the places behind it SET to 0 (assignments: from the second block on they overwrite the previous
//   permutation's output), then one more permutation.  No element: the zero digest, no permutation.
//   merge(a, b): init = a || b fills the whole state, fin = permute(init), out[i] = init[i] + init[4+i] + fin[i] + fin[4+i].
//   NOT hash_elements of the same eight elements.  merge_with_int(seed, v): init = seed || new(v), [v / p], 0, 5 [6].
//   Digests leave as 4 canonical little-endian u64; digest words coming in are read as BaseElement::new reads them.
//
// Two forms of the permutation, as in rescue_dev.hpp:
//   permute()       one lane per permutation: the state in 16 VGPRs, rolled rounds, the inverse S-box on GROUP elements at a
//                   time with the state rotated by GROUP places per step (every index a compile-time constant, no scratch).
//   permute_lane()  one state element per lane in groups of 8 lanes, none idle: a wave holds 8 permutations.  The Jive sum
//                   costs one more gather (merge_lane).
// The round constants are the published parameters in Montgomery form (x * 2^64 mod p); tests/test_rpjive_host.py pins them
// to tests/golden/rpjive64_256_params.json, scripts/gen_rpjive_fixtures.py --header prints them.
#pragma once
#include "jive_dev.hpp"

namespace wf {
namespace rpj {

constexpr int STATE = 8, RATE = 4, RATE_AT = 4, DIGEST = 4, ROUNDS = 7;
#ifndef WF_RPJIVE_GROUP
#define WF_RPJIVE_GROUP 2
#endif
constexpr int GROUP = WF_RPJIVE_GROUP;  // elements of the inverse S-box walked together in permute(); STATE % GROUP == 0
static_assert(STATE % GROUP == 0, "the rotation of permute() needs a GROUP that divides the state width");

constexpr uint32_t mds_coef(int k) {
    constexpr uint32_t row[STATE] = {23, 8, 13, 10, 7, 6, 21, 8};
    return row[k];
}

// ARK1 (half 0) / ARK2 (half 1) of round r for state element i (r, and in the lane form i, is a run-time index).
WF_HD uint64_t ark(int half, int r, uint32_t i) {
    constexpr uint64_t t[2][ROUNDS][STATE] = {
        {   // ARK1
            {0x99f9ea501d29c867ull, 0xb671c2a04fe00d7full, 0xc6e931fb63dfc49cull, 0x1712cb978024d40dull,
             0x60c7e35b956ccd56ull, 0xecb7184c4707c7e0ull, 0xdc74caaa4adedba0ull, 0x89849735fbf96c6dull},
            {0xe97dedf0e17e5535ull, 0x3dc769b8933d07dfull, 0x53ec2f55ccb7ebceull, 0x13b12db90a0dbc8bull,
             0xacdb1e6adab4aa94ull, 0x1155e79ce7bfe24eull, 0xf803cd3112ade09cull, 0xd496aa635b553552ull},
            {0x85efbce6b42eec73ull, 0x2803c593c101084eull, 0x4cbc4b8f50a9a115ull, 0x7c6122f1df22c31cull,
             0x343a393cd486114bull, 0xc7c0acd600fce6b4ull, 0x0bcd1598cd3cc7f9ull, 0xb232a6ae7dfe39dfull},
            {0x790109a3a9aedf98ull, 0x0514b1232ef0d1c1ull, 0x284bdcbd14585046ull, 0x661fee66722fffb4ull,
             0xe872f171d2ec3b46ull, 0xf83e6f51350baff5ull, 0xa6be0428efc30d3eull, 0x424b686963d0ddf0ull},
            {0xa9787ba359c35661ull, 0x3e2b8bbc369cc481ull, 0xe86667d3c4b90aa7ull, 0xb7e37af303e0650bull,
             0x2816de95a5c2473cull, 0x987ef7eb7f892fadull, 0x46922f14eec54539ull, 0xfd84396eaeb14d32ull},
            {0xef2138e576ee68b3ull, 0x9f5b8d75973caaa9ull, 0xd3434cfe7c9e5694ull, 0x44f20d3f7856cac0ull,
             0x283c9d008f7ef705ull, 0x37ba4ee67568d4ecull, 0x1b35f4c4ef46a83cull, 0xe5994789f47d1698ull},
            {0x71c206f40ce329e0ull, 0x98e9aedbf3b872f3ull, 0xea7571d73ffb563bull, 0xebe244522a972401ull,
             0x941897c405bb7342ull, 0x71c2ebaa41e39e4aull, 0x23eb4bcff0b8f055ull, 0xeb85738742897621ull},
        },
        {   // ARK2
            {0x340065aa43299a46ull, 0xbb76ba17b45344c6ull, 0x7a8d352a403edfc3ull, 0x66615df0a2d85bf8ull,
             0xdaf81431c56d8e50ull, 0xd68ba563ad3c9c94ull, 0x14346551ff31ed7full, 0x65c7fe59d5e63ae1ull},
            {0x88a5e3496d8851f2ull, 0x181b71c98a91159eull, 0x34643523ecd4d64aull, 0x07a6b18ddd109ca8ull,
             0x89fb1bdbf3587094ull, 0xdfee154e17091e20ull, 0x248352015084538dull, 0xf7bc0ea7406c6089ull},
            {0x6cff8d652fc92925ull, 0x9faa99e0fdda8a91ull, 0xd97b58877d3e6ba2ull, 0xd03e444e7e0f71a8ull,
             0x0c2b9af102392d02ull, 0xc47577c614682ef6ull, 0xa65f774c7deb3865ull, 0xdc9d71d44a7a8cd7ull},
            {0x7629c05590aef6d2ull, 0xe396cfa9c662f139ull, 0x191adfeb67ce5802ull, 0x109879086ba86e48ull,
             0xade7997e73a03983ull, 0xe4854f95d9b3db9eull, 0x37246848cb120bb8ull, 0xe43a9293a1abd568ull},
            {0xd9dd9a0284cedc24ull, 0xc9debd2182c4ac4cull, 0x1d08be5047a3eac6ull, 0xca5b569f6e7c0560ull,
             0x5a450c694974d0b4ull, 0x581c96b88aa7610full, 0xc69739778cd95502ull, 0x2aeb6c9064a6b3c2ull},
            {0x7b91f8a8c32b9857ull, 0x70fdb6c3b139e247ull, 0x4c912844c1fc0a5aull, 0xfcdd3eb911f8fca8ull,
             0x3d89477b7aa9015cull, 0xc517fc6a07b8e9eaull, 0xd93d1ae44642a0bfull, 0xfb1fa509aae8de33ull},
            {0x7cf6329603674213ull, 0x4c1f7de09b35c9baull, 0x691d51c45064bb65ull, 0xa7464cdc8772329aull,
             0xe55c301ddf425595ull, 0xffa2eef5a4a2300aull, 0xfd19db1af9db0972ull, 0x704e2142c7614ad9ull},
        },
    };
    return t[half][r][i];
}

// One row of the MDS product, get(j) = state element j: sum_k ROW[k] * get((i + k) mod 8), reduced once.  The bound of
// rp::mds_row holds with room: lo = sum ROW[k] * low word and hi = sum ROW[k] * high word are both < 96 * 2^32 < 2^39, the
// sum is lo + (hi mod 2^32) * 2^32 + (hi >> 32) * 2^64 with 2^64 = 2^32 - 1 (mod p): b = (hi mod 2^32) << 32 <= ffffffff00000000
// < p and a = lo + (hi >> 32) * (2^32 - 1) < 2^39 + 96 * 2^32 < 2^40, so one canonical addition ends it.
template <class Get>
WF_HD uint64_t mds_row(uint32_t i, Get &&get) {
    uint64_t lo = 0, hi = 0;
#pragma unroll
    for (int k = 0; k < STATE; k++) {
        const uint32_t j = (i + (uint32_t)k) & (uint32_t)(STATE - 1);
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
        for (int i = 0; i < STATE; i++) s[i] = rp::pow7(s[i]);
        mds_ark(s, 0, r);
#pragma unroll 1
        for (int it = 0; it < STATE / GROUP; it++) {  // GROUP elements per step, the state rotated by GROUP places
            uint64_t g[GROUP];
#pragma unroll
            for (int k = 0; k < GROUP; k++) g[k] = s[k];
            rp::inv_sbox<GROUP>(g);
#pragma unroll
            for (int i = 0; i + GROUP < STATE; i++) s[i] = s[i + GROUP];
#pragma unroll
            for (int k = 0; k < GROUP; k++) s[STATE - GROUP + k] = g[k];
        }
        mds_ark(s, 1, r);
    }
}

// ------------------------------------------------------------------------------------ form 2: one state element per lane
// The linear layer of lane i (i < 8); the S-box on its own element is the caller's (rp::pow7 / rp::lane_inv_sbox).
template <class Get>
WF_HD uint64_t lane_mds_ark(uint32_t i, int half, int r, Get &&get) {
    return F64::add(mds_row(i, get), ark(half, r, i));
}

#if defined(__HIPCC__)
// x = element i of the state held by the 8-lane group this lane belongs to (i = lane % 8).  Every lane of the wave must be
// active: the gathers read other lanes.
__device__ __forceinline__ uint64_t permute_lane(uint64_t x) {
    const uint32_t lane = __lane_id();
    const uint32_t i = lane & 7u, base = lane & ~7u;
    auto get = [&](uint32_t j) { return rp::lane_value(x, base + j); };
#pragma unroll 1
    for (int r = 0; r < ROUNDS; r++) {
        x = rp::pow7(x);
        x = lane_mds_ark(i, 0, r, get);
        x = rp::lane_inv_sbox(x);
        x = lane_mds_ark(i, 1, r, get);
    }
    return x;
}

// merge in the lane form: lane i of a group hands in digest word i of a || b as stored; lanes 0..3 of the group return the
// canonical digest word i (the other lanes' value is of no use).  Each lane forms t = init + fin, lanes 0..3 add the t of
// lane + 4: the one gather the Jive sum costs.  Every lane of the wave must be active.
__device__ __forceinline__ uint64_t merge_lane(uint64_t w) {
    const uint64_t init = rp::elem_new(w);
    const uint64_t t = F64::add(init, permute_lane(init));
    const uint64_t u = rp::lane_value(t, (__lane_id() + 4u) & 63u);
    return F64::to_canonical(F64::add(t, u));
}

// The hasher as k_merkle_subtree_lanes (rescue_kernels.hpp) takes it: groups of 8 lanes, lane e loads / carries word e of the
// child pair and none idles; lanes 0..3 end with the parent's digest word e, canonical as merge_lane leaves it.
struct Lanes {
    static constexpr const MerklePlan &PLAN = MERKLE_PLAN_RPJIVE;
    static constexpr uint32_t LOG_LANES = 3, WORD_AT = 0, DIGEST_AT = 0;
    static __device__ __forceinline__ uint64_t merge_lane(uint32_t, uint64_t w) { return rpj::merge_lane(w); }
    static __device__ __forceinline__ uint64_t digest_word(uint64_t x) { return x; }
};
#endif

// The same lane form on the host: the 8 lanes of one group in lockstep (what tests/cpp/test_rpjive_host.cpp runs).
static inline void permute_lanes_host(uint64_t (&s)[STATE]) {
    uint64_t o[STATE];
    for (int r = 0; r < ROUNDS; r++) {
        for (int half = 0; half < 2; half++) {
            for (int i = 0; i < STATE; i++) s[i] = half == 0 ? rp::pow7(s[i]) : rp::lane_inv_sbox(s[i]);
            for (int i = 0; i < STATE; i++) o[i] = lane_mds_ark((uint32_t)i, half, r, [&](uint32_t j) { return s[j]; });
            for (int i = 0; i < STATE; i++) s[i] = o[i];
        }
    }
}
// merge_lane on the host: t per lane, then lanes 0..3 add lane + 4's.
static inline void merge_lanes_host(const uint64_t (&in)[STATE], uint64_t (&out)[DIGEST]) {
    uint64_t init[STATE], s[STATE];
    for (int i = 0; i < STATE; i++) s[i] = init[i] = rp::elem_new(in[i]);
    permute_lanes_host(s);
    for (int i = 0; i < STATE; i++) s[i] = F64::add(init[i], s[i]);
    for (int i = 0; i < DIGEST; i++) out[i] = F64::to_canonical(F64::add(s[i], s[i + 4]));
}

// ------------------------------------------------------------------------------------ sponge and compression
// jive_dev.hpp on this permutation: the rate (and the digest) in places 4..7, the "partial block" flag in place 0.
struct Perm {
    static constexpr int RATE_AT = rpj::RATE_AT, FLAG_AT = 0;
    static WF_HD void permute(uint64_t (&s)[STATE]) { rpj::permute(s); }
};
template <class Next>
WF_HD void hash_elements(uint64_t n, Next &&next, uint64_t (&out)[DIGEST]) { jive::hash_elements<Perm>(n, next, out); }
WF_HD void merge(const uint64_t (&in)[8], uint64_t (&out)[DIGEST]) { jive::merge<Perm>(in, out); }
WF_HD void merge_with_int_mont(const uint64_t (&seed)[DIGEST], uint64_t value, uint64_t (&out)[DIGEST]) { jive::merge_with_int_mont<Perm>(seed, value, out); }
WF_HD void merge_with_int(const uint64_t (&seed)[DIGEST], uint64_t value, uint64_t (&out)[DIGEST]) { jive::merge_with_int<Perm>(seed, value, out); }
struct Merge : jive::Merge<Perm> {};
struct Absorb : jive::Absorb<Perm> {};

}  // namespace rpj
}  // namespace wf
