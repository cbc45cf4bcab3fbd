// One instruction of a planned constraint program on one lane's state.  Host- and device-compilable like field.hpp and
// rescue_dev.hpp: the interpreter kernel (cprog_kernels.hpp) and tests/cpp/test_cprog_host.cpp run this same function, the
// kernel on a lane's LDS slots, the test on a plain array.
//
// `S` is the lane's view of memory:
//   T    slot(uint32_t s) const         the lane's value in LDS slot s
//   void set_slot(uint32_t s, T v)
//   T    constant(uint32_t off) const   element `off` of the constant buffer (the same for all lanes)
//   T    table(uint32_t t) const        table entry t at the lane's step
// The op is split by operand types (cprog_plan.hpp): a base operand of an E op is embedded -- added to or subtracted from
// coordinate 0, multiplied into every coordinate (mul_base) -- and E x E is ext_mul.
#pragma once
#include "cprog_plan.hpp"
#include "field.hpp"

namespace wf {

template <class F, class S>
WF_HD typename F::T cprog_base_operand(const S &s, uint32_t kind, uint32_t v) {
    if (kind == CPK_LDS) return s.slot(v);
    if (kind == CPK_CONST) return s.constant(v);
    return s.table(v);
}

// an operand of type E: a register (WE consecutive slots) or an extension constant (WE consecutive constants)
template <class F, int WE, class S>
WF_HD Ext<F, WE> cprog_ext_operand(const S &s, uint32_t kind, uint32_t v) {
    Ext<F, WE> r;
#pragma unroll
    for (int w = 0; w < WE; w++) r.c[w] = kind == CPK_LDS ? s.slot(v + w) : s.constant(v + w);
    return r;
}

template <class F, int WE, class S>
WF_HD void cprog_step(const CpInstr &in, S &s) {
    typedef typename F::T T;
    const uint32_t op = in.code() >> 2, typing = in.code() & 3;
    if (WE == 1 || typing == CPT_BB) {
        const T a = cprog_base_operand<F>(s, in.a_kind(), in.a), b = cprog_base_operand<F>(s, in.b_kind(), in.b);
        s.set_slot(in.dst, op == 0 ? F::add(a, b) : op == 1 ? F::sub(a, b) : F::mul(a, b));
        return;
    }
    if constexpr (WE > 1) {
        Ext<F, WE> r;
        if (typing == CPT_EE) {
            const Ext<F, WE> a = cprog_ext_operand<F, WE>(s, in.a_kind(), in.a), b = cprog_ext_operand<F, WE>(s, in.b_kind(), in.b);
            if (op == 2) {
                r = ext_mul<F, WE>(a, b);
            } else {
#pragma unroll
                for (int w = 0; w < WE; w++) r.c[w] = op == 0 ? F::add(a.c[w], b.c[w]) : F::sub(a.c[w], b.c[w]);
            }
        } else if (typing == CPT_EB) {
            r = cprog_ext_operand<F, WE>(s, in.a_kind(), in.a);
            const T b = cprog_base_operand<F>(s, in.b_kind(), in.b);
            if (op == 2) {
#pragma unroll
                for (int w = 0; w < WE; w++) r.c[w] = F::mul(r.c[w], b);
            } else {
                r.c[0] = op == 0 ? F::add(r.c[0], b) : F::sub(r.c[0], b);
            }
        } else {  // CPT_BE
            const T a = cprog_base_operand<F>(s, in.a_kind(), in.a);
            const Ext<F, WE> b = cprog_ext_operand<F, WE>(s, in.b_kind(), in.b);
            if (op == 2) {
#pragma unroll
                for (int w = 0; w < WE; w++) r.c[w] = F::mul(a, b.c[w]);
            } else if (op == 0) {
                r = b;
                r.c[0] = F::add(a, b.c[0]);
            } else {
                r.c[0] = F::sub(a, b.c[0]);
#pragma unroll
                for (int w = 1; w < WE; w++) r.c[w] = F::sub(F::zero(), b.c[w]);
            }
        }
#pragma unroll
        for (int w = 0; w < WE; w++) s.set_slot(in.dst + w, r.c[w]);
    }
}

}  // namespace wf
