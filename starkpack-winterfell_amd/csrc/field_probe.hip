// libwf_field_probe.so -- test helper, NOT part of the product ABI (nothing in include/wf_lde.h, nothing in libwf_lde.so
// uses it; same footing as libwf_yardstick.so): the field primitives of field.hpp, the extension products of
// fri_kernels.hpp, the Rescue S-boxes of rescue_dev.hpp, the MDS rows of both Rescue hashers (one-lane form, every row of
// one state, no round constants) and the linear form and non-linear layer of griffin_dev.hpp as the DEVICE compiler emits them, one element per thread, so
// that tests/test_gpu_field_probe.py can feed the 32-bit carry and borrow chains the operands that make their rare
// branches fire and compare every result with integer arithmetic.
//
// What this shows is the device code of these functions in ONE inlining context (a load, the call, a store).  The
// product kernels inline the same source into other surroundings; tests/test_gpu_field_edges.py covers those.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "field.hpp"
#include "fri_kernels.hpp"
#include "rescue_dev.hpp"
#include "rescue_jive_dev.hpp"
#include "griffin_dev.hpp"

using namespace wf;

namespace {

enum Op {
    OP_F64_MUL = 0,
    OP_F64_ADD = 1,
    OP_F64_SUB = 2,
    OP_F64_MONT_REDUCE = 3,  // a = low word, b = high word
    OP_F64_TO_CANONICAL = 4,
    OP_F64_FROM_CANONICAL = 5,
    OP_F64_SHIFTS = 6,  // SHIFT_COUNT results per input, see shifts()
    OP_F128_ADD = 7,
    OP_F128_SUB = 8,
    OP_F128_MUL = 9,
    OP_EXT_MUL_F64_2 = 10,
    OP_EXT_MUL_F64_3 = 11,
    OP_EXT_MUL_F128_2 = 12,
    OP_RP_POW7 = 13,
    OP_RP_INV_SBOX = 14,
    OP_RP_MDS_ROWS = 15,   // 12 words in, 12 out: out[i] = rp::mds_row(i) of the state
    OP_RPJ_MDS_ROWS = 16,  // 8 words in, 8 out: out[i] = rpj::mds_row(i) of the state
    OP_COUNT = 17,         // ops 0 .. 16 are contiguous; 17 .. 31 are not ops
    OP_GFJ_LINEAR = 32,    // 4 words in (i = 2..7, z0, z1, t as raw residues), 1 out: gfj::linear(i, z0, z1, t); another i gives 0
    OP_GFJ_NONLINEAR = 33  // 8 words in, 8 out: gfj::nonlinear of the state
};
constexpr bool is_op(int op) { return (op >= 0 && op < OP_COUNT) || op == OP_GFJ_LINEAR || op == OP_GFJ_NONLINEAR; }

// mul_pow2<1..63> | div_pow2<1..32> | neg_div_pow2<1..32> | neg_mul_pow2<33..63> | mul_pow2_192<0..191>
constexpr int SHIFT_MUL_AT = 0, SHIFT_DIV_AT = 63, SHIFT_NEG_DIV_AT = 95, SHIFT_NEG_MUL_AT = 127, SHIFT_192_AT = 158;
constexpr int SHIFT_COUNT = 350;

template <int K>
__device__ __forceinline__ void shifts_k(uint64_t x, uint64_t *o) {
    if constexpr (K < 64) {
        o[SHIFT_MUL_AT + K - 1] = F64::mul_pow2<K>(x);
        if constexpr (K <= 32) {
            o[SHIFT_DIV_AT + K - 1] = F64::div_pow2<K>(x);
            o[SHIFT_NEG_DIV_AT + K - 1] = F64::neg_div_pow2<K>(x);
        } else {
            o[SHIFT_NEG_MUL_AT + K - 33] = F64::neg_mul_pow2<K>(x);
        }
        shifts_k<K + 1>(x, o);
    }
}
template <int E>
__device__ __forceinline__ void shifts_e(uint64_t x, uint64_t *o) {
    if constexpr (E < 192) {
        o[SHIFT_192_AT + E] = F64::mul_pow2_192<E>(x);
        shifts_e<E + 1>(x, o);
    }
}

// words (uint64_t) per element of a, b and out
struct Shape {
    int a, b, out;
};
constexpr Shape shape_of(int op) {
    switch (op) {
        case OP_F64_MUL:
        case OP_F64_ADD:
        case OP_F64_SUB:
        case OP_F64_MONT_REDUCE: return {1, 1, 1};
        case OP_F64_TO_CANONICAL:
        case OP_F64_FROM_CANONICAL:
        case OP_RP_POW7:
        case OP_RP_INV_SBOX: return {1, 0, 1};
        case OP_F64_SHIFTS: return {1, 0, SHIFT_COUNT};
        case OP_F128_ADD:
        case OP_F128_SUB:
        case OP_F128_MUL:
        case OP_EXT_MUL_F64_2: return {2, 2, 2};
        case OP_EXT_MUL_F64_3: return {3, 3, 3};
        case OP_EXT_MUL_F128_2: return {4, 4, 4};
        case OP_RP_MDS_ROWS: return {rp::STATE, 0, rp::STATE};
        case OP_RPJ_MDS_ROWS: return {rpj::STATE, 0, rpj::STATE};
        case OP_GFJ_LINEAR: return {4, 0, 1};
        case OP_GFJ_NONLINEAR: return {gfj::STATE, 0, gfj::STATE};
        default: return {0, 0, 0};
    }
}

__device__ __forceinline__ U128 ld128(const uint64_t *p) { return U128{p[0], p[1]}; }
__device__ __forceinline__ void st128(uint64_t *p, U128 v) {
    p[0] = v.lo;
    p[1] = v.hi;
}

template <class F, int W>
__device__ __forceinline__ void probe_ext_mul(const typename F::T *a, const typename F::T *b, typename F::T *o) {
    ext_store<F, W>(o, ext_mul<F, W>(ext_load<F, W>(a), ext_load<F, W>(b)));
}

// one element per thread; threads at or past n touch nothing
template <int OP>
__global__ void __launch_bounds__(256) k_probe(const uint64_t *__restrict__ a, const uint64_t *__restrict__ b,
                                               uint64_t *__restrict__ out, size_t n) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    constexpr Shape s = shape_of(OP);
    const uint64_t *pa = a + i * s.a, *pb = b + i * s.b;
    uint64_t *po = out + i * s.out;
    if constexpr (OP == OP_F64_MUL) po[0] = F64::mul(pa[0], pb[0]);
    else if constexpr (OP == OP_F64_ADD) po[0] = F64::add(pa[0], pb[0]);
    else if constexpr (OP == OP_F64_SUB) po[0] = F64::sub(pa[0], pb[0]);
    else if constexpr (OP == OP_F64_MONT_REDUCE) po[0] = F64::mont_reduce(pa[0], pb[0]);
    else if constexpr (OP == OP_F64_TO_CANONICAL) po[0] = F64::to_canonical(pa[0]);
    else if constexpr (OP == OP_F64_FROM_CANONICAL) po[0] = F64::from_canonical(pa[0]);
    else if constexpr (OP == OP_F64_SHIFTS) {
        shifts_k<1>(pa[0], po);
        shifts_e<0>(pa[0], po);
    } else if constexpr (OP == OP_F128_ADD) st128(po, F128::add(ld128(pa), ld128(pb)));
    else if constexpr (OP == OP_F128_SUB) st128(po, F128::sub(ld128(pa), ld128(pb)));
    else if constexpr (OP == OP_F128_MUL) st128(po, F128::mul(ld128(pa), ld128(pb)));
    else if constexpr (OP == OP_EXT_MUL_F64_2) probe_ext_mul<F64, 2>(pa, pb, po);
    else if constexpr (OP == OP_EXT_MUL_F64_3) probe_ext_mul<F64, 3>(pa, pb, po);
    else if constexpr (OP == OP_EXT_MUL_F128_2)
        probe_ext_mul<F128, 2>((const U128 *)pa, (const U128 *)pb, (U128 *)po);
    else if constexpr (OP == OP_RP_POW7) po[0] = rp::pow7(pa[0]);
    else if constexpr (OP == OP_RP_INV_SBOX) po[0] = rp::lane_inv_sbox(pa[0]);
    else if constexpr (OP == OP_RP_MDS_ROWS) {
        uint64_t s[rp::STATE];
#pragma unroll
        for (int j = 0; j < rp::STATE; j++) s[j] = pa[j];
#pragma unroll
        for (int i = 0; i < rp::STATE; i++) po[i] = rp::mds_row((uint32_t)i, [&](uint32_t j) { return s[j]; });
    } else if constexpr (OP == OP_RPJ_MDS_ROWS) {
        uint64_t s[rpj::STATE];
#pragma unroll
        for (int j = 0; j < rpj::STATE; j++) s[j] = pa[j];
#pragma unroll
        for (int i = 0; i < rpj::STATE; i++) po[i] = rpj::mds_row((uint32_t)i, [&](uint32_t j) { return s[j]; });
    } else if constexpr (OP == OP_GFJ_LINEAR) {
        uint64_t l = 0;  // the product calls linear with a compile-time i: so does every arm here
        switch (pa[0]) {
            case 2: l = gfj::linear(2, pa[1], pa[2], pa[3]); break;
            case 3: l = gfj::linear(3, pa[1], pa[2], pa[3]); break;
            case 4: l = gfj::linear(4, pa[1], pa[2], pa[3]); break;
            case 5: l = gfj::linear(5, pa[1], pa[2], pa[3]); break;
            case 6: l = gfj::linear(6, pa[1], pa[2], pa[3]); break;
            case 7: l = gfj::linear(7, pa[1], pa[2], pa[3]); break;
            default: break;
        }
        po[0] = l;
    } else if constexpr (OP == OP_GFJ_NONLINEAR) {
        uint64_t s[gfj::STATE];
#pragma unroll
        for (int j = 0; j < gfj::STATE; j++) s[j] = pa[j];
        gfj::nonlinear(s);
#pragma unroll
        for (int j = 0; j < gfj::STATE; j++) po[j] = s[j];
    }
}

template <int OP>
void launch_ops(int op, const uint64_t *a, const uint64_t *b, uint64_t *out, size_t n, hipStream_t st) {
    if constexpr (OP < OP_COUNT) {
        if (op == OP) {
            const unsigned blocks = (unsigned)((n + 255) / 256);
            k_probe<OP><<<blocks, 256, 0, st>>>(a, b, out, n);
        } else {
            launch_ops<OP + 1>(op, a, b, out, n, st);
        }
    } else {  // the ops behind the gap
        const unsigned blocks = (unsigned)((n + 255) / 256);
        if (op == OP_GFJ_LINEAR) k_probe<OP_GFJ_LINEAR><<<blocks, 256, 0, st>>>(a, b, out, n);
        else if (op == OP_GFJ_NONLINEAR) k_probe<OP_GFJ_NONLINEAR><<<blocks, 256, 0, st>>>(a, b, out, n);
    }
}

struct Buffers {
    void *a = nullptr, *b = nullptr, *out = nullptr;
    hipStream_t st = nullptr;
    ~Buffers() {
        if (a) (void)hipFree(a);
        if (b) (void)hipFree(b);
        if (out) (void)hipFree(out);
        if (st) (void)hipStreamDestroy(st);
    }
};

}  // namespace

// words per element of (a, b, out) for `op`; 0 for an unknown op
extern "C" int wf_field_probe_words(int op, int *a_words, int *b_words, int *out_words) {
    if (!is_op(op)) return 0;
    const Shape s = shape_of(op);
    *a_words = s.a;
    *b_words = s.b;
    *out_words = s.out;
    return 1;
}

// out[i] = op(a[i], b[i]) for i < n, on `device`, on a stream of this call's own.  `out` holds out_capacity >= n elements: the
// whole of it is copied to the device first and back afterwards, so whatever the caller put behind element n comes back
// unchanged unless the kernel wrote past n.  b is ignored by the one-operand ops.  No buffer may exceed MAX_BYTES, whatever
// the op's words per element (a test helper has no business taking more of a shared device).  Returns a hipError_t.
extern "C" int wf_field_probe(int device, int op, const void *a, const void *b, void *out, size_t n, size_t out_capacity) {
    constexpr size_t MAX_BYTES = (size_t)64 << 20;
    if (!is_op(op) || out_capacity < n) return (int)hipErrorInvalidValue;
    if (n == 0) return (int)hipSuccess;
    const Shape s = shape_of(op);
    if (!a || !out || (s.b && !b)) return (int)hipErrorInvalidValue;
    // out_capacity >= n, s.out >= 1: the first test bounds n as well, so none of the products below can wrap
    if (out_capacity > MAX_BYTES / ((size_t)s.out * 8) || n > MAX_BYTES / ((size_t)s.a * 8) ||
        (s.b && n > MAX_BYTES / ((size_t)s.b * 8)))
        return (int)hipErrorInvalidValue;
    int prev = 0;
    hipError_t e = hipGetDevice(&prev);
    if (e != hipSuccess) return (int)e;
    e = hipSetDevice(device);
    if (e == hipSuccess) {
        Buffers d;
        const size_t na = n * s.a * 8, nb = n * s.b * 8, no = out_capacity * s.out * 8;
        e = hipStreamCreateWithFlags(&d.st, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipMalloc(&d.a, na);
        if (e == hipSuccess && nb) e = hipMalloc(&d.b, nb);
        if (e == hipSuccess) e = hipMalloc(&d.out, no);
        if (e == hipSuccess) e = hipMemcpyAsync(d.a, a, na, hipMemcpyHostToDevice, d.st);
        if (e == hipSuccess && nb) e = hipMemcpyAsync(d.b, b, nb, hipMemcpyHostToDevice, d.st);
        if (e == hipSuccess) e = hipMemcpyAsync(d.out, out, no, hipMemcpyHostToDevice, d.st);
        if (e == hipSuccess) {
            launch_ops<0>(op, (const uint64_t *)d.a, (const uint64_t *)d.b, (uint64_t *)d.out, n, d.st);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(out, d.out, no, hipMemcpyDeviceToHost, d.st);
        const hipError_t es = d.st ? hipStreamSynchronize(d.st) : hipSuccess;
        if (e == hipSuccess) e = es;
    }
    (void)hipSetDevice(prev);
    return (int)e;
}
