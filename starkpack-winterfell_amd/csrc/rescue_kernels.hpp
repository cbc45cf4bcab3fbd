// Rp64_256 and RpJive64_256 as commitment hashers (crypto/src/hash/rescue/rp64_256/mod.rs, rp64_256_jive/mod.rs): leaf
// hashing and the Merkle tree on rescue_dev.hpp / rescue_jive_dev.hpp.  The same arguments, device layouts and roles as the
// BLAKE3 and Sha3 kernels (32-byte digest slots, nodes[1] = root, a level of n nodes at nodes[n .. 2n), nodes[0] = zero
// digest written by the launch that produces the root).  A digest is its four elements as canonical little-endian u64
// (ElementDigest::as_bytes); f64 only.
//   k_hash_rows_sponge<F64, rp::Absorb / rpj::Absorb> (keccak_kernels.hpp), k_merkle_level<rp::Merge / rpj::Merge> (kernels.hpp)
//                             one lane per permutation (rp::permute, rpj::permute): the throughput form
//   k_merkle_subtree_lanes<L> one state element per lane (L = rp::Lanes: 16 lanes per node, rp::permute_lane; rpj::Lanes: 8
//                             lanes per node, rpj::merge_lane): the top of the tree, where a level is one permutation's
//                             latency -- a different algorithm from k_merkle_subtree<M>
#pragma once
#include "kernels.hpp"
#include "merkle_plan.hpp"
#include "rescue_jive_dev.hpp"

namespace wf {

// The top of the tree in the lane form.  A work-group of THREADS lanes is SPAN groups of 2^L::LOG_LANES: it folds 2 * SPAN
// children through up to `levels` levels (levels <= log2(SPAN) + 1), group g of a level merging children 2g and 2g + 1.
// Lane e of a group holds state element e: lanes L::WORD_AT .. + 7 load / carry one word of the child pair each, lanes
// L::DIGEST_AT .. + 3 end with a word of the parent's digest (the lane policies say what the other lanes do).  Intermediate
// digests go through LDS (canonical words, as they are stored), every level is written to `nodes` (8-byte words: node i at
// nodes[4 i]).  No lane leaves a wave that still permutes: the gathers of the lane form need the whole wave.
template <class L>
__global__ void __launch_bounds__(L::PLAN.subtree_threads) k_merkle_subtree_lanes(const uint64_t *__restrict__ children,
                                                                                  uint64_t *__restrict__ nodes,
                                                                                  uint64_t n_children, uint32_t levels) {
    constexpr uint32_t THREADS = L::PLAN.subtree_threads, SPAN = L::PLAN.subtree_span, LANES = 1u << L::LOG_LANES;
    static_assert(THREADS == LANES * SPAN && SPAN == 1u << (L::PLAN.subtree_levels - 1));
    static_assert(THREADS <= 1024 && THREADS % 64 == 0);
    __shared__ uint64_t sh[SPAN * 4];
    const uint32_t g = threadIdx.x >> L::LOG_LANES, e = threadIdx.x & (LANES - 1);
    const bool word = e >= L::WORD_AT && e < L::WORD_AT + 8;  // this lane carries word e - WORD_AT of a child pair
    uint64_t n_par = n_children >> 1;              // nodes in the first produced level
    uint64_t first = (uint64_t)blockIdx.x * SPAN;  // this group's slice of that level
    uint32_t width = (uint32_t)min((uint64_t)SPAN, n_par - first);
    uint64_t w = 0;
    if (g < width && word) w = children[(first + g) * 8 + (e - L::WORD_AT)];
    for (uint32_t lv = 0;; lv++) {
        // a wave none of whose groups has a node at this level sits the permutation out (a whole wave: uniform branch)
        uint64_t x = 0;
        if (((threadIdx.x >> 6) << (6 - L::LOG_LANES)) < width) x = L::merge_lane(e, w);
        const bool out = g < width && e >= L::DIGEST_AT && e < L::DIGEST_AT + 4;
        const uint64_t d = L::digest_word(x);
        if (out) nodes[(n_par + first + g) * 4 + (e - L::DIGEST_AT)] = d;
        if (lv + 1 == levels) break;
        __syncthreads();  // (the previous level's digests have been read)
        if (out) sh[g * 4 + (e - L::DIGEST_AT)] = d;
        __syncthreads();
        n_par >>= 1;
        first >>= 1;
        width >>= 1;
        w = (g < width && word) ? sh[g * 8 + (e - L::WORD_AT)] : 0;
    }
    // the launch that produces the root also writes nodes[0] = ElementDigest::default() -- by a kernel rather than a memset so
    // that a captured graph of the commitment replays it
    if (blockIdx.x == 0 && threadIdx.x < 4 && (n_children >> levels) == 1) nodes[threadIdx.x] = 0;
}

}  // namespace wf
