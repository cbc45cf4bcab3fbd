// Sha3_256 as the commitment hasher (crypto/src/hash/sha/mod.rs:17-57): leaf hashing and the Merkle tree on keccak_dev.hpp.
// The same arguments, device layouts and roles as the BLAKE3 kernels of kernels.hpp (32-byte digest slots, nodes[1] = root,
// a level of n nodes at nodes[n .. 2n), nodes[0] = zero digest written by the launch that produces the root).  SHA3 absorbs
// sequentially: there is no chunk tree, so one kernel hashes rows of any length and nothing passes through hash_tmp.
#pragma once
#include "kernels.hpp"
#include "keccak_dev.hpp"

namespace wf {

// The message lanes of one combined row, in hashing order: trace 0's epr elements, trace 1's, .. (padding lanes of the stored
// rows skipped, as k_hash_rows walks them).  An f64 element is one lane (its canonical value, as hash_elements serialises
// it), an f128 element two (lo, hi).  Loads are 16 bytes where the layout allows: every f128 element, and f64 elements
// two at a time when rows start on 16-byte boundaries (even row width); the second half waits in `held`.
// (Every lane of a wave walks the same (trace, column) sequence: the branches below are uniform.)
template <class F>
struct Sha3RowLanes;

template <>
struct Sha3RowLanes<F64> {
    const uint64_t *p;
    uint64_t trace_elems, held;
    uint32_t col, epr;
    bool pairs, has_held;
    __device__ __forceinline__ Sha3RowLanes(const HashArgs<F64> &a, uint64_t j)
        : p(a.lde + j * a.row_width), trace_elems(a.trace_elems), held(0), col(0), epr(a.epr),
          pairs(a.row_width % 2 == 0 && a.trace_elems % 2 == 0 && (reinterpret_cast<uintptr_t>(a.lde) & 15) == 0), has_held(false) {}
    __device__ __forceinline__ uint64_t operator()() {
        if (has_held) {
            has_held = false;
            return F64::to_canonical(held);
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
        return F64::to_canonical(v);
    }
};

template <>
struct Sha3RowLanes<F128> {
    const U128 *p;
    uint64_t trace_elems, held;
    uint32_t col, epr;
    bool has_held;
    __device__ __forceinline__ Sha3RowLanes(const HashArgs<F128> &a, uint64_t j)
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

// Leaf j = SHA3-256(canonical LE bytes of row j of trace 0 || row j of trace 1 || ..): one lane per row, rows of any length.
template <class F>
__global__ void __launch_bounds__(256) k_sha3_hash_rows(HashArgs<F> a) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= a.n_rows) return;
    Sha3RowLanes<F> lanes(a, j);
    uint64_t d[4];
    k3::sha3_256_lanes((uint64_t)a.n_traces * a.epr * (F::BYTES / 8), lanes, d);
    ulonglong2 *dst = reinterpret_cast<ulonglong2 *>(a.leaves + j * 8);
    dst[0] = make_ulonglong2(d[0], d[1]);
    dst[1] = make_ulonglong2(d[2], d[3]);
}

// One Merkle level per launch: parents[i] = merge(children[2i], children[2i+1]); 64 contiguous bytes in, 32 out.
static __global__ void __launch_bounds__(256) k_sha3_merkle_level(const ulonglong2 *__restrict__ children,
                                                                  ulonglong2 *__restrict__ parents, uint64_t n_parents) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_parents) return;
    const ulonglong2 q0 = children[4 * i], q1 = children[4 * i + 1], q2 = children[4 * i + 2], q3 = children[4 * i + 3];
    const uint64_t in[8] = {q0.x, q0.y, q1.x, q1.y, q2.x, q2.y, q3.x, q3.y};
    uint64_t d[4];
    k3::sha3_merge(in, d);
    parents[2 * i] = make_ulonglong2(d[0], d[1]);
    parents[2 * i + 1] = make_ulonglong2(d[2], d[3]);
}

// The top of the tree, the role of k_merkle_subtree: each work-group folds 2 * blockDim children through up to `levels`
// levels, the intermediate digests in LDS, every level written to `nodes` (in 8-byte words: node i at nodes[4 i]).
static __global__ void __launch_bounds__(256) k_sha3_merkle_subtree(const uint64_t *__restrict__ children,
                                                                    uint64_t *__restrict__ nodes, uint64_t n_children,
                                                                    uint32_t levels) {
    __shared__ uint64_t sh[256 * 4];
    const uint32_t tid = threadIdx.x;
    uint64_t n_par = n_children >> 1;                     // nodes in the first produced level
    uint64_t first = (uint64_t)blockIdx.x * blockDim.x;   // this group's slice of that level
    uint32_t width = (uint32_t)min((uint64_t)blockDim.x, n_par - first);
    uint64_t in[8], d[4];
    if (tid < width) {
        const ulonglong2 *src = reinterpret_cast<const ulonglong2 *>(children + (first + tid) * 8);
        const ulonglong2 q0 = src[0], q1 = src[1], q2 = src[2], q3 = src[3];
        in[0] = q0.x; in[1] = q0.y; in[2] = q1.x; in[3] = q1.y;
        in[4] = q2.x; in[5] = q2.y; in[6] = q3.x; in[7] = q3.y;
        k3::sha3_merge(in, d);
        ulonglong2 *dst = reinterpret_cast<ulonglong2 *>(nodes + (n_par + first + tid) * 4);
        dst[0] = make_ulonglong2(d[0], d[1]);
        dst[1] = make_ulonglong2(d[2], d[3]);
#pragma unroll
        for (int i = 0; i < 4; i++) sh[tid * 4 + i] = d[i];
    }
    for (uint32_t lv = 1; lv < levels; lv++) {
        __syncthreads();
        n_par >>= 1;
        first >>= 1;
        width >>= 1;
        const bool act = tid < width;
        if (act) {
#pragma unroll
            for (int i = 0; i < 8; i++) in[i] = sh[tid * 8 + i];
            k3::sha3_merge(in, d);
        }
        __syncthreads();
        if (act) {
            ulonglong2 *dst = reinterpret_cast<ulonglong2 *>(nodes + (n_par + first + tid) * 4);
            dst[0] = make_ulonglong2(d[0], d[1]);
            dst[1] = make_ulonglong2(d[2], d[3]);
#pragma unroll
            for (int i = 0; i < 4; i++) sh[tid * 4 + i] = d[i];
        }
    }
    // the launch that produces the root also writes nodes[0] = Digest::default() (merkle/mod.rs:355) -- by a kernel rather
    // than a memset so that a captured graph of the commitment replays it
    if (blockIdx.x == 0 && tid == 0 && (n_children >> levels) == 1) {
        ulonglong2 *dst = reinterpret_cast<ulonglong2 *>(nodes);
        dst[0] = make_ulonglong2(0, 0);
        dst[1] = make_ulonglong2(0, 0);
    }
}

}  // namespace wf
