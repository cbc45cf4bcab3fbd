// Rp64_256 as the commitment hasher (crypto/src/hash/rescue/rp64_256/mod.rs): leaf hashing and the Merkle tree on
// rescue_dev.hpp.  The same arguments, device layouts and roles as the BLAKE3 and Sha3 kernels (32-byte digest slots,
// nodes[1] = root, a level of n nodes at nodes[n .. 2n), nodes[0] = zero digest written by the launch that produces the
// root).  A digest is its four elements as canonical little-endian u64 (ElementDigest::as_bytes); f64 only.
//   k_hash_rows_sponge<F64, rp::Absorb> (keccak_kernels.hpp), k_merkle_level<rp::Merge> (kernels.hpp)
//                             one lane per permutation (rp::permute): the throughput form
//   k_rp64_merkle_subtree     16 lanes per node, one state element per lane (rp::permute_lane): the top of the tree, where
//                             a level is one permutation's latency -- a different algorithm from k_merkle_subtree<M>
#pragma once
#include "kernels.hpp"
#include "merkle_plan.hpp"
#include "rescue_dev.hpp"

namespace wf {

// The top of the tree in the lane form.  A work-group of RP64_SUBTREE_THREADS lanes is RP64_SUBTREE_SPAN groups of 16: it
// folds 2 * SPAN children through up to `levels` levels (levels <= log2(SPAN) + 1), group g of a level merging children
// 2g and 2g + 1.  Lane e of a group holds state element e: lanes 4..11 load / carry one digest word each, lane 0 the
// element count, lanes 12..15 nothing.  Intermediate digests go through LDS (canonical words, as they are stored), every
// level is written to `nodes` (8-byte words: node i at nodes[4 i]).  No lane leaves a wave that still permutes: the gathers
// of permute_lane need the whole wave.
constexpr uint32_t RP64_SUBTREE_THREADS = MERKLE_PLAN_RP64.subtree_threads, RP64_SUBTREE_SPAN = MERKLE_PLAN_RP64.subtree_span;
static_assert(RP64_SUBTREE_THREADS == 16 * RP64_SUBTREE_SPAN && RP64_SUBTREE_SPAN == 1u << (MERKLE_PLAN_RP64.subtree_levels - 1));
static __global__ void __launch_bounds__(RP64_SUBTREE_THREADS) k_rp64_merkle_subtree(const uint64_t *__restrict__ children,
                                                                                     uint64_t *__restrict__ nodes,
                                                                                     uint64_t n_children, uint32_t levels) {
    __shared__ uint64_t sh[RP64_SUBTREE_SPAN * 4];
    const uint32_t g = threadIdx.x >> 4, e = threadIdx.x & 15;
    const bool word = e >= (uint32_t)rp::RATE_AT && e < (uint32_t)rp::STATE;  // this lane carries digest word e - 4 of a child pair
    uint64_t n_par = n_children >> 1;                            // nodes in the first produced level
    uint64_t first = (uint64_t)blockIdx.x * RP64_SUBTREE_SPAN;   // this group's slice of that level
    uint32_t width = (uint32_t)min((uint64_t)RP64_SUBTREE_SPAN, n_par - first);
    uint64_t w = 0;
    if (g < width && word) w = children[(first + g) * 8 + (e - rp::RATE_AT)];
    for (uint32_t lv = 0;; lv++) {
        // a wave none of whose four groups has a node at this level sits the permutation out (a whole wave: uniform branch)
        uint64_t x = 0;
        if (((threadIdx.x >> 6) << 2) < width) x = rp::permute_lane(rp::merge_lane_init(e, w));
        const bool out = g < width && e >= (uint32_t)rp::RATE_AT && e < (uint32_t)(rp::RATE_AT + rp::DIGEST);
        const uint64_t d = F64::to_canonical(x);
        if (out) nodes[(n_par + first + g) * 4 + (e - rp::RATE_AT)] = d;
        if (lv + 1 == levels) break;
        __syncthreads();  // (the previous level's digests have been read)
        if (out) sh[g * 4 + (e - rp::RATE_AT)] = d;
        __syncthreads();
        n_par >>= 1;
        first >>= 1;
        width >>= 1;
        w = (g < width && word) ? sh[g * 8 + (e - rp::RATE_AT)] : 0;
    }
    // the launch that produces the root also writes nodes[0] = ElementDigest::default() -- by a kernel rather than a memset so
    // that a captured graph of the commitment replays it
    if (blockIdx.x == 0 && threadIdx.x < 4 && (n_children >> levels) == 1) nodes[threadIdx.x] = 0;
}

}  // namespace wf
