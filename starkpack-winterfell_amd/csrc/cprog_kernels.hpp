// The constraint-program interpreter (wf_constraint_evaluate): ConstraintEvaluator::evaluate of the reference
// (prover/src/constraints/evaluator.rs:74-241) for the main trace segment, with Air::evaluate_transition and the boundary
// constraints handed over as a straight-line program (cprog_plan.hpp).  One thread per step of the constraint evaluation
// domain; every lane of a wave executes the same instruction, so the instruction stream, the constants and the table
// descriptors are read through wave-uniform loads and only the data differs per lane.
//
// A lane's state -- the frame columns the program reads, the domain point and the registers -- lives in LDS, laid out
// [slot][lane]: consecutive lanes hit consecutive banks, and the run-time register index of an instruction is an LDS address
// instead of an index into a register array (which would be left in scratch memory).  A lane touches its own column of the
// layout only: no barrier anywhere.
//   frame (trace_lde.rs:78-93): CUR = LDE row step << lde_shift, NEXT = row (that + lde_blowup) mod n; both rows are read
//   from the resident matrix, only the columns the planner found in use.
//   x = offset * g_ce^step (get_ce_x_at, domain.rs:125-132), from the two-level table of the ce domain's generator.
// k_cprog_eval_aux is the same interpreter for an AIR with an auxiliary segment (wf_constraint_evaluate_aux): it also loads
// the columns of E that the program reads from the same two rows of the auxiliary matrix (trace_lde.rs:100-108).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cprog_dev.hpp"
#include "pow2l.hpp"

namespace wf {

template <class F>
struct CprogArgs {
    typedef typename F::T T;
    const T *lde;             // the trace's matrix: n rows of row_width elements
    T *out;                   // [n_out] columns of ce elements of E
    const CpInstr *instrs;    // 16 bytes each, 16-byte aligned
    const uint32_t *frame;    // [n_frame] column | NEXT << 16; entry i goes to slot i
    const uint32_t *outs;     // [n_out] slot | is E << 31
    const CpTable *tables;
    const T *consts;
    const T *table_values;
    uint64_t ce, n_mask;      // n_mask: LDE rows - 1
    uint64_t next_rows;       // lde_blowup: one trace step in LDE rows
    uint32_t n_instrs, n_frame, n_out, x_slot;
    uint32_t lde_shift, row_width;
    T offset;
    Pow2L<F> g;               // powers of the ce domain's generator
};

template <class F>
struct CprogLane {
    typedef typename F::T T;
    // the LDS address space is part of the pointer's type: a generic pointer here lets the optimizer merge the LDS read of a
    // register operand and the read of a constant into ONE load through a flat pointer -- the constants then come through the
    // vector memory path per lane instead of a wave-uniform load
    // (held as 64-bit words: an f128 element is read and written as its two halves)
    typedef __attribute__((address_space(3))) uint64_t LdsWord;
    static constexpr uint32_t W = sizeof(T) / 8;
    LdsWord *lds;  // slot 0 of this lane
    uint32_t stride;
    const T *consts;
    const CpTable *tables;
    const T *table_values;
    uint64_t step;
    __device__ __forceinline__ T slot(uint32_t s) const {
        if constexpr (W == 1) {
            return lds[s * stride];
        } else {
            const LdsWord *p = lds + (size_t)s * stride * 2;
            return T{p[0], p[1]};
        }
    }
    __device__ __forceinline__ void set_slot(uint32_t s, T v) {
        if constexpr (W == 1) {
            lds[s * stride] = v;
        } else {
            LdsWord *p = lds + (size_t)s * stride * 2;
            p[0] = v.lo;
            p[1] = v.hi;
        }
    }
    __device__ __forceinline__ T constant(uint32_t off) const { return consts[off]; }
    __device__ __forceinline__ T table(uint32_t t) const {
        const CpTable d = tables[t];
        return table_values[d.offset + (((uint32_t)step - d.shift) & d.mask)];
    }
};

// the auxiliary segment's frame (wf_constraint_evaluate_aux): a second matrix with its own row width and list of columns
template <class F>
struct CprogAuxArgs {
    typedef typename F::T T;
    const T *lde;             // the auxiliary trace's matrix: n rows of row_width base elements, an element of E WE of them
    const uint32_t *frame;    // [n_frame] column of E | NEXT << 16; entry i goes to slots base + i * WE ..
    uint32_t n_frame, base, row_width;
};

// the auxiliary frame: entries of WE base elements each from the two rows of the auxiliary matrix into slots base + i * WE ..,
// one coordinate at a time (always valid: a row of that matrix is only element-aligned)
template <class F, int WE>
__device__ __forceinline__ void cprog_load_aux_frame(CprogLane<F> &s, const CprogAuxArgs<F> &x, uint64_t row_cur, uint64_t row_next) {
    typedef typename F::T T;
    const T *cur = x.lde + row_cur * x.row_width, *next = x.lde + row_next * x.row_width;
    for (uint32_t i = 0; i < x.n_frame; i++) {
        const uint32_t f = x.frame[i];
        const T *e = ((f >> 16) ? next : cur) + (f & 0xFFFFu) * WE;
#pragma unroll
        for (int w = 0; w < WE; w++) s.set_slot(x.base + i * WE + w, e[w]);
    }
}

// (k_cprog_eval_aux below repeats this body with a second frame load: a fix here belongs there as well)
template <class F, int WE>
__global__ void __launch_bounds__(256) k_cprog_eval(CprogArgs<F> a) {
    typedef typename F::T T;
    extern __shared__ __attribute__((aligned(16))) unsigned char cprog_smem[];
    const uint64_t step = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (step >= a.ce) return;  // (no barriers below: a lane works on its own LDS column)
    CprogLane<F> s;
    s.lds = (typename CprogLane<F>::LdsWord *)cprog_smem + threadIdx.x * CprogLane<F>::W;
    s.stride = blockDim.x;
    s.consts = a.consts;
    s.tables = a.tables;
    s.table_values = a.table_values;
    s.step = step;

    const uint64_t row_cur = step << a.lde_shift, row_next = (row_cur + a.next_rows) & a.n_mask;
    const T *cur = a.lde + row_cur * a.row_width, *next = a.lde + row_next * a.row_width;
    for (uint32_t i = 0; i < a.n_frame; i++) {
        const uint32_t f = a.frame[i];
        s.set_slot(i, ((f >> 16) ? next : cur)[f & 0xFFFFu]);
    }
    if (a.x_slot != CP_NO_SLOT) s.set_slot(a.x_slot, F::mul(a.g.get(step), a.offset));

    // (fetching instruction i + 1 ahead of the step gains nothing: scalar loads return out of order, so the first wait for a
    // constant is a wait for everything outstanding, the prefetch included)
    for (uint32_t i = 0; i < a.n_instrs; i++) {
        const CpInstr in = a.instrs[i];
        cprog_step<F, WE>(in, s);
    }

    for (uint32_t j = 0; j < a.n_out; j++) {
        const uint32_t o = a.outs[j], sl = o & 0x7FFFFFFFu;
        T *dst = a.out + ((uint64_t)j * a.ce + step) * WE;
        dst[0] = s.slot(sl);
#pragma unroll
        for (int w = 1; w < WE; w++) dst[w] = (o >> 31) ? s.slot(sl + w) : F::zero();
    }
}

// The interpreter with the auxiliary frame (wf_constraint_evaluate_aux: evaluate_fragment_full, evaluator.rs:190-241): the
// kernel above with a second frame load behind the first.  From there on an auxiliary element is an E operand in LDS like an E
// register, so the lane (CprogLane) and the step function (cprog_step) are the main kernel's.  The two kernel bodies are kept
// as two texts on purpose: with the common lines moved into an inlined function k_cprog_eval compiles to other code than
// before (docs/EXPERIMENTS.md), and its traces and measurements are keyed by that code.
template <class F, int WE>
__global__ void __launch_bounds__(256) k_cprog_eval_aux(CprogArgs<F> a, CprogAuxArgs<F> x) {
    typedef typename F::T T;
    extern __shared__ __attribute__((aligned(16))) unsigned char cprog_smem[];
    const uint64_t step = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (step >= a.ce) return;  // (no barriers below: a lane works on its own LDS column)
    CprogLane<F> s;
    s.lds = (typename CprogLane<F>::LdsWord *)cprog_smem + threadIdx.x * CprogLane<F>::W;
    s.stride = blockDim.x;
    s.consts = a.consts;
    s.tables = a.tables;
    s.table_values = a.table_values;
    s.step = step;

    const uint64_t row_cur = step << a.lde_shift, row_next = (row_cur + a.next_rows) & a.n_mask;
    const T *cur = a.lde + row_cur * a.row_width, *next = a.lde + row_next * a.row_width;
    for (uint32_t i = 0; i < a.n_frame; i++) {
        const uint32_t f = a.frame[i];
        s.set_slot(i, ((f >> 16) ? next : cur)[f & 0xFFFFu]);
    }
    cprog_load_aux_frame<F, WE>(s, x, row_cur, row_next);
    if (a.x_slot != CP_NO_SLOT) s.set_slot(a.x_slot, F::mul(a.g.get(step), a.offset));

    for (uint32_t i = 0; i < a.n_instrs; i++) {
        const CpInstr in = a.instrs[i];
        cprog_step<F, WE>(in, s);
    }

    for (uint32_t j = 0; j < a.n_out; j++) {
        const uint32_t o = a.outs[j], sl = o & 0x7FFFFFFFu;
        T *dst = a.out + ((uint64_t)j * a.ce + step) * WE;
        dst[0] = s.slot(sl);
#pragma unroll
        for (int w = 1; w < WE; w++) dst[w] = (o >> 31) ? s.slot(sl + w) : F::zero();
    }
}

}  // namespace wf
