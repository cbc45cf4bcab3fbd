// From a hasher id to the code that implements it: the one chain over hasher ids in the units that launch kernels.
#pragma once
#include "blake3_dev.hpp"
#include "griffin_dev.hpp"
#include "hasher_table.hpp"
#include "keccak_dev.hpp"
#include "rescue_dev.hpp"
#include "rescue_jive_dev.hpp"

namespace wf {

// A hasher at compile time.  M: the merge policy of the tree kernels (grind_kernels.hpp maps it to the search's policy);
// A: the absorb policy of k_hash_rows_sponge, void where the rows are not hashed by a sponge (BLAKE3: chunks); L: the lane
// policy of k_merkle_subtree_lanes, void where the sub-tree kernel is the generic k_merkle_subtree<M>; P: the tree's plan.
template <class M, class A, class L, const MerklePlan &P, bool F64_ONLY_>
struct HasherTag {
    typedef M Merge;
    typedef A Absorb;
    typedef L Lanes;
    static constexpr const MerklePlan &PLAN = P;
    static constexpr bool F64_ONLY = F64_ONLY_;
};

// fn(tag) for the tag of (hasher, digest_bytes): enum wf_hasher and the digest size in bytes -- 32, or 24 for Blake3_192
// (48-byte merge inputs; the slots' last two words are zeros).  The pair has passed check_hasher_pair: an id that is none
// of the others is BLAKE3.
template <class Fn>
int dispatch_hasher(uint32_t hasher, uint32_t digest_bytes, Fn &&fn) {
    switch (hasher) {
    case WF_HASH_SHA3_256: return fn(HasherTag<k3::Merge, k3::Absorb, void, MERKLE_PLAN_SHA3, false>());
    case WF_HASH_RP64_256: return fn(HasherTag<rp::Merge, rp::Absorb, rp::Lanes, MERKLE_PLAN_RP64, true>());
    case WF_HASH_RPJIVE64_256: return fn(HasherTag<rpj::Merge, rpj::Absorb, rpj::Lanes, MERKLE_PLAN_RPJIVE, true>());
    case WF_HASH_GRIFFINJIVE64_256: return fn(HasherTag<gfj::Merge, gfj::Absorb, void, MERKLE_PLAN_GRIFFIN, true>());
    default:
        return digest_bytes == 24 ? fn(HasherTag<b3::Merge<6>, void, void, MERKLE_PLAN_BLAKE3, false>())
                                  : fn(HasherTag<b3::Merge<8>, void, void, MERKLE_PLAN_BLAKE3, false>());
    }
}

}  // namespace wf
