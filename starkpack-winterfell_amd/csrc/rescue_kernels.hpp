// Rp64_256 as the commitment hasher (crypto/src/hash/rescue/rp64_256/mod.rs): leaf hashing and the Merkle tree on
// rescue_dev.hpp.  The same arguments, device layouts and roles as the BLAKE3 and Sha3 kernels (32-byte digest slots,
// nodes[1] = root, a level of n nodes at nodes[n .. 2n), nodes[0] = zero digest written by the launch that produces the
// root).  A digest is its four elements as canonical little-endian u64 (ElementDigest::as_bytes); f64 only.
//   k_rp64_hash_rows / k_rp64_merkle_level   one lane per permutation (rp::permute): the throughput form
//   k_rp64_merkle_subtree                    16 lanes per node, one state element per lane (rp::permute_lane): the top
//                                            of the tree, where a level is one permutation's latency
#pragma once
#include "kernels.hpp"
#include "rescue_dev.hpp"

namespace wf {

// The elements of one combined row, in hashing order: trace 0's epr elements, trace 1's, .. (padding lanes of the stored rows
// skipped), as Sha3RowLanes<F64> walks them -- but as they are stored: the sponge adds Montgomery residues, nothing is
// converted on the way in.  16-byte loads when rows start on 16-byte boundaries; the second half waits in `held`.
struct Rp64RowElems {
    const uint64_t *p;
    uint64_t trace_elems, held;
    uint32_t col, epr;
    bool pairs, has_held;
    __device__ __forceinline__ Rp64RowElems(const HashArgs<F64> &a, uint64_t j)
        : p(a.lde + j * a.row_width), trace_elems(a.trace_elems), held(0), col(0), epr(a.epr),
          pairs(a.row_width % 2 == 0 && a.trace_elems % 2 == 0 && (reinterpret_cast<uintptr_t>(a.lde) & 15) == 0), has_held(false) {}
    __device__ __forceinline__ uint64_t operator()() {
        if (has_held) {
            has_held = false;
            return held;
        }
        uint64_t v;
        if (pairs && col + 1 < epr) {  // (col is even here: it advances by two, and the odd last element resets it to 0)
            const ulonglong2 q = *reinterpret_cast<const ulonglong2 *>(p + col);
            v = q.x;
            held = q.y;
            has_held = true;
            col += 2;
        } else {
            v = p[col];
            col += 1;
        }
        if (col == epr) {  // next trace's row (never dereferenced behind the last trace: the absorber stops asking)
            col = 0;
            p += trace_elems;
        }
        return v;
    }
};

// Leaf j = Rp64_256::hash_elements(row j of trace 0 || row j of trace 1 || ..): one lane per row, rows of any length;
// state[0] = the number of base elements of the combined row.
static __global__ void __launch_bounds__(256) k_rp64_hash_rows(HashArgs<F64> a) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= a.n_rows) return;
    Rp64RowElems elems(a, j);
    uint64_t d[4];
    rp::hash_elements((uint64_t)a.n_traces * a.epr, elems, d);
    ulonglong2 *dst = reinterpret_cast<ulonglong2 *>(a.leaves + j * 8);
    dst[0] = make_ulonglong2(d[0], d[1]);
    dst[1] = make_ulonglong2(d[2], d[3]);
}

// One wide Merkle level per launch: parents[i] = merge(children[2i], children[2i+1]); one lane per parent.
static __global__ void __launch_bounds__(256) k_rp64_merkle_level(const ulonglong2 *__restrict__ children,
                                                                  ulonglong2 *__restrict__ parents, uint64_t n_parents) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_parents) return;
    const ulonglong2 q0 = children[4 * i], q1 = children[4 * i + 1], q2 = children[4 * i + 2], q3 = children[4 * i + 3];
    const uint64_t in[8] = {q0.x, q0.y, q1.x, q1.y, q2.x, q2.y, q3.x, q3.y};
    uint64_t d[4];
    rp::merge(in, d);
    parents[2 * i] = make_ulonglong2(d[0], d[1]);
    parents[2 * i + 1] = make_ulonglong2(d[2], d[3]);
}

// The top of the tree in the lane form.  A work-group of RP64_SUBTREE_THREADS lanes is RP64_SUBTREE_SPAN groups of 16: it
// folds 2 * SPAN children through up to `levels` levels (levels <= log2(SPAN) + 1), group g of a level merging children
// 2g and 2g + 1.  Lane e of a group holds state element e: lanes 4..11 load / carry one digest word each, lane 0 the
// element count, lanes 12..15 nothing.  Intermediate digests go through LDS (canonical words, as they are stored), every
// level is written to `nodes` (8-byte words: node i at nodes[4 i]).  No lane leaves a wave that still permutes: the gathers
// of permute_lane need the whole wave.
constexpr uint32_t RP64_SUBTREE_THREADS = 1024, RP64_SUBTREE_SPAN = RP64_SUBTREE_THREADS / 16, RP64_SUBTREE_LEVELS = 7;
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
