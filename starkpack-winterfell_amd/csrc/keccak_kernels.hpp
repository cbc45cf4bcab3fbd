// Leaf hashing of the sponge hashers: Sha3_256 (crypto/src/hash/sha/mod.rs:17-57, on keccak_dev.hpp) and Rp64_256 (on
// rescue_dev.hpp).  The same arguments, device layouts and roles as the BLAKE3 kernels of kernels.hpp (32-byte digest slots).
// A sponge absorbs sequentially: there is no chunk tree, so one kernel hashes rows of any length and nothing passes through
// hash_tmp.  Their trees are k_merkle_level<M> / k_merkle_subtree<M> of kernels.hpp on k3::Merge and rp::Merge (and, for the
// top of the Rp64_256 tree, k_merkle_subtree_lanes of rescue_kernels.hpp).
#pragma once
#include "kernels.hpp"

namespace wf {

// The message lanes of one combined row, in hashing order: trace 0's epr elements, trace 1's, .. (padding lanes of the stored
// rows skipped, as k_hash_rows walks them).  An f64 element is one lane, an f128 element two (lo, hi).  CANONICAL: the lane
// is the element's canonical value, as Sha3_256::hash_elements serialises it; otherwise the element as it is stored (Rp64_256:
// the sponge adds Montgomery residues, f64 only).  Loads are 16 bytes where the layout allows: every f128 element, and f64
// elements two at a time when rows start on 16-byte boundaries (even row width); the second half waits in `held`.
// (Every lane of a wave walks the same (trace, column) sequence: the branches below are uniform.)
template <class F, bool CANONICAL>
struct RowLanes;

template <bool CANONICAL>
struct RowLanes<F64, CANONICAL> {
    const uint64_t *p;
    uint64_t trace_elems, held;
    uint32_t col, epr;
    bool pairs, has_held;
    __device__ __forceinline__ RowLanes(const HashArgs<F64> &a, uint64_t j)
        : p(a.lde + j * a.row_width), trace_elems(a.trace_elems), held(0), col(0), epr(a.epr),
          pairs(a.row_width % 2 == 0 && a.trace_elems % 2 == 0 && (reinterpret_cast<uintptr_t>(a.lde) & 15) == 0), has_held(false) {}
    static __device__ __forceinline__ uint64_t lane(uint64_t v) { return CANONICAL ? F64::to_canonical(v) : v; }
    __device__ __forceinline__ uint64_t operator()() {
        if (has_held) {
            has_held = false;
            return lane(held);
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
        return lane(v);
    }
};

template <>
struct RowLanes<F128, true> {
    const U128 *p;
    uint64_t trace_elems, held;
    uint32_t col, epr;
    bool has_held;
    __device__ __forceinline__ RowLanes(const HashArgs<F128> &a, uint64_t j)
        : p(a.lde + j * a.row_width), trace_elems(a.trace_elems), held(0), col(0), epr(a.epr), has_held(false) {}
    __device__ __forceinline__ uint64_t operator()() {
        if (has_held) {  // (the 9th element of a rate block straddles it: its high lane opens the next block)
            has_held = false;
            return held;
        }
        const ulonglong2 q = *reinterpret_cast<const ulonglong2 *>(p + col);
        held = q.y;
        has_held = true;
        if (++col == epr) {
            col = 0;
            p += trace_elems;
        }
        return q.x;
    }
};

// Leaf j = hash_elements(row j of trace 0 || row j of trace 1 || ..) for a sponge hasher: one lane per row, rows of any length.
// A is the hasher's absorber policy: k3::Absorb (SHA3-256 of the canonical LE bytes) or rp::Absorb (Rp64_256::hash_elements,
// state[0] = the number of base elements of the combined row).
template <class F, class A>
__global__ void __launch_bounds__(256) k_hash_rows_sponge(HashArgs<F> a) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= a.n_rows) return;
    RowLanes<F, A::CANONICAL> lanes(a, j);
    uint64_t d[4];
    A::absorb((uint64_t)a.n_traces * a.epr * (F::BYTES / 8), lanes, d);
    store_digest(reinterpret_cast<uint64_t *>(a.leaves) + j * 4, d);
}

}  // namespace wf
