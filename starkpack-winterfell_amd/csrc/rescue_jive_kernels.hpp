// RpJive64_256 as the commitment hasher (crypto/src/hash/rescue/rp64_256_jive/mod.rs): leaf hashing and the Merkle tree on
// rescue_jive_dev.hpp.  The same arguments, device layouts and roles as the other hashers' kernels (32-byte digest slots,
// nodes[1] = root, a level of n nodes at nodes[n .. 2n), nodes[0] = zero digest written by the launch that produces the
// root).  A digest is its four elements as canonical little-endian u64 (ElementDigest::as_bytes); f64 only.
//   k_hash_rows_sponge<F64, rpj::Absorb> (keccak_kernels.hpp), k_merkle_level<rpj::Merge> (kernels.hpp)
//                             one lane per permutation (rpj::permute): the throughput form
//   k_rpjive_merkle_subtree   8 lanes per node, one state element per lane (rpj::merge_lane): the top of the tree
#pragma once
#include "kernels.hpp"
#include "merkle_plan.hpp"
#include "rescue_jive_dev.hpp"

namespace wf {

// The top of the tree in the lane form.  A work-group of RPJIVE_SUBTREE_THREADS lanes is RPJIVE_SUBTREE_SPAN groups of 8: it
// folds 2 * SPAN children through up to `levels` levels (levels <= log2(SPAN) + 1), group g of a level merging children 2g
// and 2g + 1.  The state of a merge is the two children's digests and nothing else, so lane e of a group loads / carries
// word e of the child pair and no lane idles; lanes 0..3 end with the parent's digest word e.  Intermediate digests go
// through LDS (canonical words, as they are stored), every level is written to `nodes` (8-byte words: node i at nodes[4 i]).
// No lane leaves a wave that still permutes: the gathers of merge_lane need the whole wave.
constexpr uint32_t RPJIVE_SUBTREE_THREADS = MERKLE_PLAN_RPJIVE.subtree_threads, RPJIVE_SUBTREE_SPAN = MERKLE_PLAN_RPJIVE.subtree_span;
static_assert(RPJIVE_SUBTREE_THREADS == 8 * RPJIVE_SUBTREE_SPAN && RPJIVE_SUBTREE_SPAN == 1u << (MERKLE_PLAN_RPJIVE.subtree_levels - 1));
static_assert(RPJIVE_SUBTREE_THREADS <= 1024 && RPJIVE_SUBTREE_THREADS % 64 == 0);
static __global__ void __launch_bounds__(RPJIVE_SUBTREE_THREADS) k_rpjive_merkle_subtree(const uint64_t *__restrict__ children,
                                                                                         uint64_t *__restrict__ nodes,
                                                                                         uint64_t n_children, uint32_t levels) {
    __shared__ uint64_t sh[RPJIVE_SUBTREE_SPAN * 4];
    const uint32_t g = threadIdx.x >> 3, e = threadIdx.x & 7;
    uint64_t n_par = n_children >> 1;                              // nodes in the first produced level
    uint64_t first = (uint64_t)blockIdx.x * RPJIVE_SUBTREE_SPAN;   // this group's slice of that level
    uint32_t width = (uint32_t)min((uint64_t)RPJIVE_SUBTREE_SPAN, n_par - first);
    uint64_t w = 0;
    if (g < width) w = children[(first + g) * 8 + e];
    for (uint32_t lv = 0;; lv++) {
        // a wave none of whose eight groups has a node at this level sits the permutation out (a whole wave: uniform branch)
        uint64_t d = 0;
        if (((threadIdx.x >> 6) << 3) < width) d = rpj::merge_lane(w);
        const bool out = g < width && e < (uint32_t)rpj::DIGEST;
        if (out) nodes[(n_par + first + g) * 4 + e] = d;
        if (lv + 1 == levels) break;
        __syncthreads();  // (the previous level's digests have been read)
        if (out) sh[g * 4 + e] = d;
        __syncthreads();
        n_par >>= 1;
        first >>= 1;
        width >>= 1;
        w = g < width ? sh[g * 8 + e] : 0;
    }
    // the launch that produces the root also writes nodes[0] = ElementDigest::default() -- by a kernel rather than a memset so
    // that a captured graph of the commitment replays it
    if (blockIdx.x == 0 && threadIdx.x < 4 && (n_children >> levels) == 1) nodes[threadIdx.x] = 0;
}

}  // namespace wf
