// What RpJive64_256 and GriffinJive64_256 share around their permutations: the rate-4 sponge with the padding SET into the
// rate, the 2-to-1 compression in Jive mode, merge_with_int, and the Merge / Absorb policies of the tree and row kernels.
// Host- and device-compilable like its neighbours.  Everything is a template over a permutation policy P:
//   P::RATE_AT     the first of the four rate places (the digest is read from the same places)
//   P::FLAG_AT     the capacity place that holds 1 iff the number of hashed elements is no multiple of 4
//   P::permute(s)  the permutation of the 8-element state (Montgomery residues)
// rescue_jive_dev.hpp and griffin_dev.hpp define their P and keep their own names as one-line forwards.  Rp64_256 is not of
// this shape (it adds its padding, keeps the element count in place 0 and has no Jive sum): it stays in rescue_dev.hpp.
#pragma once
#include "rescue_dev.hpp"

namespace wf {
namespace jive {

constexpr int STATE = 8, RATE = 4, DIGEST = 4;

// hash_elements of n base elements; next() returns them in order as Montgomery residues (the stored form).  One permutation
// call site; state elements are addressed with compile-time indices only.  Elements are ADDED into the rate four at a time,
// a permutation behind every full block.  Only the last block can be partial (take < RATE exactly when fewer than RATE
// elements remain): behind its i elements rate place i is SET to 1 and the places behind it SET to 0 (assignments: from the
// second block on they overwrite the previous permutation's output), then one more permutation.  No element: the zero
// digest, no permutation.  out = the canonical digest words.
template <class P, class Next>
WF_HD void hash_elements(uint64_t n, Next &&next, uint64_t (&out)[DIGEST]) {
    uint64_t s[STATE];
#pragma unroll
    for (int i = 0; i < STATE; i++) s[i] = 0;
    s[P::FLAG_AT] = (n % RATE) != 0 ? F64::one() : 0;
    uint64_t rem = n;
    while (rem) {
        const uint32_t take = rem < (uint64_t)RATE ? (uint32_t)rem : (uint32_t)RATE;
#pragma unroll
        for (int i = 0; i < RATE; i++) {
            if ((uint32_t)i < take) s[P::RATE_AT + i] = F64::add(s[P::RATE_AT + i], next());
            else s[P::RATE_AT + i] = (uint32_t)i == take ? F64::one() : 0;
        }
        P::permute(s);
        rem -= take;
    }
#pragma unroll
    for (int i = 0; i < DIGEST; i++) out[i] = F64::to_canonical(s[P::RATE_AT + i]);
}

// The Jive compression of a state already in Montgomery form: out[i] = init[i] + init[4+i] + fin[i] + fin[4+i], canonical.
// (The sums of the initial state are formed before the permutation: 4 values live across it, not 8.)
template <class P>
WF_HD void compress(uint64_t (&s)[STATE], uint64_t (&out)[DIGEST]) {
    uint64_t pre[DIGEST];
#pragma unroll
    for (int i = 0; i < DIGEST; i++) pre[i] = F64::add(s[i], s[DIGEST + i]);
    P::permute(s);
#pragma unroll
    for (int i = 0; i < DIGEST; i++) out[i] = F64::to_canonical(F64::add(pre[i], F64::add(s[i], s[DIGEST + i])));
}

// merge: the digest words of the two children (4 + 4, as stored: canonical, or any u64 from a caller) -> canonical digest.
// init = a || b fills the whole state: NOT hash_elements of the same eight elements.
template <class P>
WF_HD void merge(const uint64_t (&in)[8], uint64_t (&out)[DIGEST]) {
    uint64_t s[STATE];
#pragma unroll
    for (int i = 0; i < STATE; i++) s[i] = rp::elem_new(in[i]);
    compress<P>(s, out);
}

// merge_with_int (rescue/rp64_256_jive/mod.rs:201-224, griffin/griffin64_256_jive/mod.rs:183-206) on a seed already in
// Montgomery form (the search kernel converts its seed once): the seed in places 0..3, BaseElement::new(value) in place 4 and
// 5 in place 7 when value < p; otherwise value / p in place 5 as well and 6 in place 7.  p <= value < 2^64 < 2 p, so that
// quotient is 1.
template <class P>
WF_HD void merge_with_int_mont(const uint64_t (&seed)[DIGEST], uint64_t value, uint64_t (&out)[DIGEST]) {
    const bool wide = value >= F64::P;
    uint64_t s[STATE];
#pragma unroll
    for (int i = 0; i < DIGEST; i++) s[i] = seed[i];
    s[4] = rp::elem_new(value);
    s[5] = wide ? F64::one() : 0;
    s[6] = 0;
    s[7] = rp::elem_new(wide ? 6 : 5);
    compress<P>(s, out);
}

// The same on the seed's digest words as stored (canonical, or any u64 from a caller: read as BaseElement::new reads them).
template <class P>
WF_HD void merge_with_int(const uint64_t (&seed)[DIGEST], uint64_t value, uint64_t (&out)[DIGEST]) {
    uint64_t m[DIGEST];
#pragma unroll
    for (int i = 0; i < DIGEST; i++) m[i] = rp::elem_new(seed[i]);
    merge_with_int_mont<P>(m, value, out);
}

// The hasher as the tree kernels (Merge), the nonce search (merge_with_int_mont) and the lane-per-row leaf kernel (Absorb)
// take it, as rp::Merge / rp::Absorb.  rpj:: and gfj:: derive named structs from these: kernels are instantiated on, and
// their traces keyed by, those names.
template <class P>
struct Merge {
    using W = uint64_t;
    static constexpr int NW = DIGEST;
    static constexpr bool HAS_QUAD = false;
    static WF_HD void merge(const W (&in)[2 * NW], W (&out)[NW]) { jive::merge<P>(in, out); }
    static WF_HD void merge_with_int_mont(const W (&seed)[NW], uint64_t value, W (&out)[NW]) { jive::merge_with_int_mont<P>(seed, value, out); }
};
template <class P>
struct Absorb {
    static constexpr bool CANONICAL = false;
    template <class Next>
    static WF_HD void absorb(uint64_t n, Next &&next, uint64_t (&out)[DIGEST]) { jive::hash_elements<P>(n, next, out); }
};

}  // namespace jive
}  // namespace wf
