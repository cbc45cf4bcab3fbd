// The two-level power table the kernels read (built by tables.hpp): on its own so that a unit that needs the table and none of
// the kernels of kernels.hpp does not compile their non-template ones a second time.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "field.hpp"

namespace wf {

// Two-level table of powers of one base g: g^e = lo[e & mask] * hi[e >> s].
template <class F>
struct Pow2L {
    const typename F::T *lo;
    const typename F::T *hi;
    uint32_t s;
    uint32_t mask;
    __device__ __forceinline__ typename F::T get(uint64_t e) const {
        typename F::T a = lo[e & mask];
        uint64_t h = e >> s;
        if (h) a = F::mul(a, hi[h]);
        return a;
    }
    // branch-free form for prologues that want all their table reads in flight at once: g^e = a * b (hi[0] = 1)
    __device__ __forceinline__ void fetch(uint64_t e, typename F::T &a, typename F::T &b) const {
        a = lo[e & mask];
        b = hi[e >> s];
    }
};

}  // namespace wf
