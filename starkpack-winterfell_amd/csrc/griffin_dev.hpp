// GriffinJive64_256 (Griffin of state width 8 over p = 2^64 - 2^32 + 1, 2-to-1 compression in Jive mode) for hasher 20 of the
// commitment path: GriffinJive64_256::hash_elements / merge / merge_with_int of the reference
// (crypto/src/hash/griffin/griffin64_256_jive/mod.rs).  Host- and device-compilable like rescue_jive_dev.hpp, whose S-boxes,
// element conversion and MDS row it reuses (tests/cpp/test_griffin_host.cpp runs it under plain g++ against
// tests/griffin_util.py and tests/cpp/griffin_ref.c).
//
//   State: 8 elements of F64 (Montgomery residues), rate 0..4, capacity 4..8, digest 0..4 -- the other way round from
//   RpJive64_256.
//   Permutation: 7 rounds of  non-linear layer | MDS | + ARK[r], the last round without constants (6 rows of them).
//   Non-linear layer, in this order: s0 = s0^(1/7) (72 products); s1 = s1^7 (4); for i = 2..7
//       l_i = (i - 1) * s0 + s1 + t,   s_i *= l_i^2 + ALPHA[i-2] * l_i + BETA[i-2]     (3 products each)
//   with the NEW s0 and s1, t = 0 for i = 2 and the NEW s_{i-1} from i = 3 on: one dependency chain of 94 products a round,
//   658 a permutation (RpJive64_256: 4256).
//   MDS: the matrix of RpJive64_256 (mds_f64_8x8 of the reference, first row 23 8 13 10 7 6 21 8): rpj::mds_row.
//   Sponge: state[4] = 1 iff the number of base elements is no multiple of 4; elements ADDED into places 0..3 four at a time,
//   a permutation behind every full block; behind a partial last block of i elements place i is SET to 1 and the places
//   behind it up to 3 SET to 0, then one more permutation.  No element: the zero digest, no permutation.
//   merge(a, b): init = a || b fills the whole state, fin = permute(init), out[i] = init[i] + init[4+i] + fin[i] + fin[4+i].
//   NOT hash_elements of the same eight elements.  merge_with_int(seed, v): init = seed || new(v), [v / p], 0, 5 [6].
//   Digests leave as 4 canonical little-endian u64; digest words coming in are read as BaseElement::new reads them.
//
// One form of the permutation: one lane per permutation.  The non-linear layer is a single chain, so spreading a state over
// lanes would leave them idle; permute_n<N> instead walks N independent states of one lane together (N = 1 in every kernel;
// scripts/griffin_bench.hip measures N = 2, docs/EXPERIMENTS.md "GriffinJive64_256" has the outcome).
// The constants are the published parameters in Montgomery form (x * 2^64 mod p); tests/test_griffin_host.py pins them to
// tests/golden/griffinjive64_256_params.json, scripts/gen_griffin_fixtures.py --header prints them.
#pragma once
#include "rescue_jive_dev.hpp"

namespace wf {
namespace gfj {

constexpr int STATE = 8, RATE = 4, DIGEST = 4, ROUNDS = 7;

// ARK of round r (r < ROUNDS - 1; a run-time index) for state element i.
WF_HD uint64_t ark(int r, uint32_t i) {
    constexpr uint64_t t[ROUNDS - 1][STATE] = {
        {0x478a7bc431f215a8ull, 0x3bc3667e5a83fff8ull, 0x217ca64495ae97dcull, 0x92c32cc13f01cca0ull,
         0x7b04b2bd790b42a8ull, 0xd6e614dc9951ef81ull, 0x55aba13e64bc03ceull, 0xab5942fd1ae7d40aull},
        {0xa297474f38a26a35ull, 0x76cff911b8868017ull, 0x9dde0b439de645a0ull, 0xa2d3489158359fe4ull,
         0xb0c078994b731b59ull, 0x508e2d7faa9b83c3ull, 0xcb77d4e59a40e995ull, 0xf9448eede4613499ull},
        {0xb70d6f34c4eb1db8ull, 0x4cb8c1321069227cull, 0x210f9dd62c1398b9ull, 0xafa3f12f7d7f4925ull,
         0x5c28cb02d75a560bull, 0x9061a914edd44500ull, 0x3c37c2b3a09583c7ull, 0xab9fe6173ed759bdull},
        {0x10047af3018ddb4dull, 0x248be39e432b8bdfull, 0xf90a9d8730867420ull, 0xa4b05a49bf751eb7ull,
         0x49ac1e38ee425e2bull, 0x087977863be277adull, 0x8028c7b9bc065627ull, 0x013b525e95d24100ull},
        {0xb99ff7336d86ce75ull, 0x59b6d439f3b24d42ull, 0xe51f747cd4dc7a1full, 0xcc661e63d4ef3cb0ull,
         0xa1684e6b8dbc5aa7ull, 0x0e03639ae89860a6ull, 0x16064c601cdeda78ull, 0x6ff6e89fa29a03e1ull},
        {0xcb25e7e64194b0e1ull, 0xc48b993d7bec3a6dull, 0xd20f0ebd7e2919d6ull, 0x505ec63620d72bb6ull,
         0xcfbceaa72f9cd4a5ull, 0x8877014a005199bbull, 0x8628d7c416479827ull, 0x050b2cdfaa2fb994ull},
    };
    return t[r][i];
}
// ALPHA[i] / BETA[i] of the quadratic step on state element i + 2.
constexpr uint64_t alpha(int i) {
    constexpr uint64_t t[STATE - 2] = {0xf696723eb1ef621eull, 0xed2ce47e63dec43bull, 0xe3c356be15ce2658ull,
                                       0xda59c8fdc7bd8875ull, 0xd0f03b3d79acea92ull, 0xc786ad7d2b9c4cafull};
    return t[i];
}
constexpr uint64_t beta(int i) {
    constexpr uint64_t t[STATE - 2] = {0x824ccfb82e9d97ddull, 0x09333ee2ba765f72ull, 0x94b34d7da38a56c1ull,
                                       0x24ccfb8ae9d97dc8ull, 0xb98049088d63d489ull, 0x52cd35f88e295b02ull};
    return t[i];
}

// l_i = (i - 1) * z0 + z1 + t on residues below p (i = 2..7; linear_function of the reference, which forms the same sum in
// 128 bits).  The sum is formed on 32-bit halves: lo = sum of the low words and hi = sum of the high words are both at most
// 8 * (2^32 - 1) < 2^35, and the whole sum lo + hi * 2^32 <= 8 * (p - 1) < 2^67.  Its low 64 bits are s_lo = lo + (hi << 32)
// (which can carry: c) and its high word is s_hi = (hi >> 32) + c <= 7.  With 2^64 = 2^32 - 1 (mod p) the sum is
// s_lo + z, z = s_hi * (2^32 - 1) < 2^35: s_lo is any u64 and z < 2^35, so s_lo + z < 2^64 + 2^35 < 2 p and the one
// correction of a canonical addition (the 64-bit sum wrapped, or landed in [p, 2^64)) ends it below p.
WF_HD uint64_t linear(int i, uint64_t z0, uint64_t z1, uint64_t t) {
    const uint64_t k = (uint64_t)(i - 1);
    const uint64_t lo = k * (uint32_t)z0 + (uint32_t)z1 + (uint32_t)t;
    const uint64_t hi = k * (uint32_t)(z0 >> 32) + (uint32_t)(z1 >> 32) + (uint32_t)(t >> 32);
    const uint64_t s_lo = lo + (hi << 32);
    const uint64_t s_hi = (hi >> 32) + (s_lo < lo ? 1u : 0u);
    return F64::add(s_lo, (s_hi << 32) - s_hi);
}

// The non-linear layer on N independent states walked together (the inverse S-boxes of the N states interleave).
template <int N>
WF_HD void nonlinear_n(uint64_t (&s)[N][STATE]) {
    uint64_t g[N];
#pragma unroll
    for (int n = 0; n < N; n++) g[n] = s[n][0];
    rp::inv_sbox<N>(g);
#pragma unroll
    for (int n = 0; n < N; n++) {
        s[n][0] = g[n];
        s[n][1] = rp::pow7(s[n][1]);
    }
#pragma unroll
    for (int i = 2; i < STATE; i++) {
#pragma unroll
        for (int n = 0; n < N; n++) {
            const uint64_t l = linear(i, s[n][0], s[n][1], i == 2 ? 0 : s[n][i - 1]);
            const uint64_t q = F64::add(F64::mul(F64::add(l, alpha(i - 2)), l), beta(i - 2));  // l^2 + ALPHA l + BETA
            s[n][i] = F64::mul(s[n][i], q);
        }
    }
}
WF_HD void nonlinear(uint64_t (&s)[STATE]) {
    uint64_t t[1][STATE];
#pragma unroll
    for (int i = 0; i < STATE; i++) t[0][i] = s[i];
    nonlinear_n<1>(t);
#pragma unroll
    for (int i = 0; i < STATE; i++) s[i] = t[0][i];
}

// One lane per permutation(s): the states in 16 N VGPRs, rolled rounds, every state index a compile-time constant (no
// scratch).  The last round adds no constants.
template <int N>
WF_HD void permute_n(uint64_t (&s)[N][STATE]) {
#pragma unroll 1
    for (int r = 0; r < ROUNDS; r++) {
        nonlinear_n<N>(s);
        const bool last = r == ROUNDS - 1;
#pragma unroll
        for (int n = 0; n < N; n++) {
            uint64_t o[STATE];
#pragma unroll
            for (int i = 0; i < STATE; i++) o[i] = rpj::mds_row((uint32_t)i, [&](uint32_t j) { return s[n][j]; });
#pragma unroll
            for (int i = 0; i < STATE; i++) s[n][i] = F64::add(o[i], last ? 0 : ark(last ? 0 : r, (uint32_t)i));
        }
    }
}
WF_HD void permute(uint64_t (&s)[STATE]) {
    uint64_t t[1][STATE];
#pragma unroll
    for (int i = 0; i < STATE; i++) t[0][i] = s[i];
    permute_n<1>(t);
#pragma unroll
    for (int i = 0; i < STATE; i++) s[i] = t[0][i];
}

// ------------------------------------------------------------------------------------ sponge and compression
// jive_dev.hpp on this permutation: the rate (and the digest) in places 0..3, the "partial block" flag in place 4.
struct Perm {
    static constexpr int RATE_AT = 0, FLAG_AT = 4;
    static WF_HD void permute(uint64_t (&s)[STATE]) { gfj::permute(s); }
};
template <class Next>
WF_HD void hash_elements(uint64_t n, Next &&next, uint64_t (&out)[DIGEST]) { jive::hash_elements<Perm>(n, next, out); }
WF_HD void merge(const uint64_t (&in)[8], uint64_t (&out)[DIGEST]) { jive::merge<Perm>(in, out); }
WF_HD void merge_with_int_mont(const uint64_t (&seed)[DIGEST], uint64_t value, uint64_t (&out)[DIGEST]) { jive::merge_with_int_mont<Perm>(seed, value, out); }
WF_HD void merge_with_int(const uint64_t (&seed)[DIGEST], uint64_t value, uint64_t (&out)[DIGEST]) { jive::merge_with_int<Perm>(seed, value, out); }
struct Merge : jive::Merge<Perm> {};
struct Absorb : jive::Absorb<Perm> {};

}  // namespace gfj
}  // namespace wf
