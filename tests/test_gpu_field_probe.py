"""GPU: the field primitives of csrc/field.hpp as the device compiler emits them, on carry-edge operands.

libwf_field_probe.so (csrc/field_probe.hip; a test helper like libwf_yardstick.so, not part of the product ABI) runs one
primitive per thread over host arrays.  Here it gets the operands that make the rare branches of the 32-bit carry and
borrow chains fire -- the limb-alphabet pairs and the directed reduction inputs of tests/edge_util.py, the same sets that
tests/cpp/test_field_edges.cpp feeds the host build of these chains -- mixed with uniform ones so that a wave holds both,
and every result is compared bit for bit with Python integer arithmetic (the extension products: with the oracle).

The probe shows the device code of these functions in ONE inlining context (a load, the call, a store), not in every
kernel's: the product kernels inline the same source into other surroundings.  tests/test_gpu_field_edges.py is what
covers the kernels.

No length here is a multiple of the wave (64) or of the work-group (256) -- _ragged() asserts it -- so each launch ends in a
partial work-group and a partial wave, and every output buffer carries a poisoned tail that must come back untouched."""
import ctypes as C

import numpy as np
import pytest

import edge_util as E
from conftest import rand_f64, rand_f128

pytestmark = pytest.mark.gpu

F64, F128 = E.F64, E.F128
P, Q = E.P64, E.P128
(OP_F64_MUL, OP_F64_ADD, OP_F64_SUB, OP_F64_MONT_REDUCE, OP_F64_TO_CANONICAL, OP_F64_FROM_CANONICAL, OP_F64_SHIFTS,
 OP_F128_ADD, OP_F128_SUB, OP_F128_MUL, OP_EXT_MUL_F64_2, OP_EXT_MUL_F64_3, OP_EXT_MUL_F128_2, OP_RP_POW7,
 OP_RP_INV_SBOX, OP_RP_MDS_ROWS, OP_RPJ_MDS_ROWS) = range(17)
POISON = 0xA5A5A5A5A5A5A5A5
TAIL = 333  # poisoned elements behind the n the kernel may write


@pytest.fixture(scope="module")
def probe():
    import starkpack_winterfell_amd.build as b
    import starkpack_winterfell_amd.capi as capi
    capi.load()  # the HIP runtime torch ships, loaded the way the product library needs it
    lib = C.CDLL(b.field_probe_path())
    lib.wf_field_probe.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t]
    lib.wf_field_probe.restype = C.c_int
    lib.wf_field_probe_words.argtypes = [C.c_int] + [C.POINTER(C.c_int)] * 3
    lib.wf_field_probe_words.restype = C.c_int

    def run(op, a, b=None):
        """out[i] = op(a[i], b[i]) as (n, out_words) uint64; asserts that nothing behind element n was written."""
        wa, wb, wo = C.c_int(), C.c_int(), C.c_int()
        assert lib.wf_field_probe_words(op, C.byref(wa), C.byref(wb), C.byref(wo)) == 1
        a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, wa.value)
        n = a.shape[0]
        pb = None
        if wb.value:
            b = np.ascontiguousarray(b, dtype=np.uint64).reshape(-1, wb.value)
            assert b.shape[0] == n
            pb = b.ctypes.data
        out = np.full((n + TAIL, wo.value), POISON, dtype=np.uint64)
        rc = lib.wf_field_probe(0, op, a.ctypes.data, pb, out.ctypes.data, n, n + TAIL)
        assert rc == 0, f"hip error {rc}"
        assert (out[n:] == np.uint64(POISON)).all(), "the kernel wrote behind element n"
        return out[:n]

    return run


def _ragged(n):
    """n as it is, checked: the launch must end in a partial wave and a partial work-group."""
    assert n % 64 != 0 and n % 256 != 0
    return n


@pytest.fixture(scope="module")
def f64_pairs():
    """All 1849 ordered alphabet pairs, then 20 000 uniform pairs, shuffled together: a wave holds both kinds."""
    al = E.f64_alphabet()
    a = [x for x in al for _ in al]
    b = [y for _ in al for y in al]
    rng = np.random.default_rng(64)
    a = np.concatenate([E.u64(a), rand_f64(rng, 20000)])
    b = np.concatenate([E.u64(b), rand_f64(rng, 20000)])
    order = rng.permutation(_ragged(a.size))
    return a[order], b[order]


def test_f64_mul_add_sub(probe, f64_pairs):
    a, b = f64_pairs
    ai, bi = a.tolist(), b.tolist()
    assert probe(OP_F64_MUL, a, b).reshape(-1).tolist() == [x * y * E.R64_INV % P for x, y in zip(ai, bi)]
    assert probe(OP_F64_ADD, a, b).reshape(-1).tolist() == [(x + y) % P for x, y in zip(ai, bi)]
    assert probe(OP_F64_SUB, a, b).reshape(-1).tolist() == [(x - y) % P for x, y in zip(ai, bi)]


def test_f64_mont_reduce_directed(probe):
    """hi next to b(lo): the inputs on which c1, c3 and d1 of F64::mont_reduce fire (a mask from c2 alone is wrong on 4076 of
    these 22 481), followed by uniform (lo, hi < p)."""
    lo, hi = E.directed_reduction_inputs()
    assert len(lo) == 22481
    rng = np.random.default_rng(65)
    lo = np.concatenate([E.u64(lo), rng.integers(0, 2**64 - 1, size=20000, dtype=np.uint64, endpoint=True)])
    hi = np.concatenate([E.u64(hi), rand_f64(rng, 20000)])
    order = rng.permutation(_ragged(lo.size))
    lo, hi = lo[order], hi[order]
    want = [(h + l * E.R64_INV) % P for l, h in zip(lo.tolist(), hi.tolist())]
    assert probe(OP_F64_MONT_REDUCE, lo, hi).reshape(-1).tolist() == want


def test_f64_canonical_forms(probe):
    rng = np.random.default_rng(66)
    x = np.concatenate([E.u64(E.f64_alphabet() + E.SHIFT_EDGES), rand_f64(rng, 1000)])
    _ragged(x.size)
    xi = x.tolist()
    can = probe(OP_F64_TO_CANONICAL, x).reshape(-1)
    assert can.tolist() == [v * E.R64_INV % P for v in xi]
    assert np.array_equal(probe(OP_F64_FROM_CANONICAL, can).reshape(-1), x)
    # from_canonical reduces its argument first: any 64-bit word is legal, the six alphabet words at or above p included
    raw = [(h << 32) | l for h in E.LIMBS64 for l in E.LIMBS64] + [P, P + 1, 2**64 - 1]
    raw = np.concatenate([E.u64(raw), rng.integers(0, 2**64 - 1, size=1000, dtype=np.uint64, endpoint=True)])
    _ragged(raw.size)
    assert probe(OP_F64_FROM_CANONICAL, raw).reshape(-1).tolist() == [v * 2**64 % P for v in raw.tolist()]


def test_f64_every_shift_twiddle(probe):
    """mul_pow2<1..63>, div_pow2<1..32>, neg_div_pow2<1..32>, neg_mul_pow2<33..63>, mul_pow2_192<0..191> of every input."""
    rng = np.random.default_rng(67)
    x = np.concatenate([E.u64(E.f64_alphabet() + E.SHIFT_EDGES), rand_f64(rng, 1000)])
    _ragged(x.size)
    got = probe(OP_F64_SHIFTS, x)
    assert got.shape == (x.size, 350)
    factors = ([pow(2, k, P) for k in range(1, 64)] + [pow(2, -k, P) for k in range(1, 33)]
               + [-pow(2, -k, P) % P for k in range(1, 33)] + [-pow(2, k, P) % P for k in range(33, 64)]
               + [pow(2, e, P) for e in range(192)])
    assert len(factors) == 350
    want = [[v * f % P for f in factors] for v in x.tolist()]
    assert got.tolist() == want


@pytest.fixture(scope="module")
def f128_pairs():
    """A fixed-seed sample of 130 001 of the 42.7 M ordered alphabet pairs, the pairs with p - 1, 0 and 1 on either side, and
    20 000 uniform pairs, shuffled together."""
    al = E.alphabet_array(F128)
    rng = np.random.default_rng(128)
    ends = E.f128_array([Q - 1, 0, 1, Q - 2, 2**127])
    a = [al[rng.integers(0, al.shape[0], size=130001)], rand_f128(rng, 20000)]
    b = [al[rng.integers(0, al.shape[0], size=130001)], rand_f128(rng, 20000)]
    for e in ends:
        a += [np.broadcast_to(e, al.shape), al]
        b += [al, np.broadcast_to(e, al.shape)]
    a, b = np.concatenate(a), np.concatenate(b)
    assert a.shape[0] - 20000 <= 200000   # alphabet pairs: the Python reference stays under a few seconds
    order = rng.permutation(_ragged(a.shape[0]))
    return a[order], b[order]


def test_f128_add_sub_mul(probe, f128_pairs):
    a, b = f128_pairs
    ai, bi = E.f128_ints(a), E.f128_ints(b)
    assert E.f128_ints(probe(OP_F128_MUL, a, b)) == [x * y % Q for x, y in zip(ai, bi)]
    assert E.f128_ints(probe(OP_F128_ADD, a, b)) == [(x + y) % Q for x, y in zip(ai, bi)]
    assert E.f128_ints(probe(OP_F128_SUB, a, b)) == [(x - y) % Q for x, y in zip(ai, bi)]


@pytest.mark.parametrize("field,ext,op", [(F64, 2, OP_EXT_MUL_F64_2), (F64, 3, OP_EXT_MUL_F64_3), (F128, 2, OP_EXT_MUL_F128_2)])
def test_ext_mul(probe, orc, field, ext, op):
    """ext_mul<F, W> of csrc/fri_kernels.hpp against the oracle's product, one call per element.  Operands: every coordinate
    drawn from the limb alphabet, elements with a single non-zero coordinate, and uniform ones."""
    rng = np.random.default_rng(1000 * field + ext)
    w = 1 if field == F64 else 2
    n_alpha, n_uni = 6000, 20000
    a = np.concatenate([E.alphabet_draw(rng, field, n_alpha * ext), (rand_f64 if field == F64 else rand_f128)(rng, n_uni * ext)])
    b = np.concatenate([E.alphabet_draw(rng, field, n_alpha * ext), (rand_f64 if field == F64 else rand_f128)(rng, n_uni * ext)])
    a = a.reshape(-1, ext * w).copy()
    b = b.reshape(-1, ext * w).copy()
    for k in range(ext):  # a single non-zero coordinate on one side, then on both
        a[k:1200:2 * ext, :k * w] = 0
        a[k:1200:2 * ext, (k + 1) * w:] = 0
        b[k:600:ext, :k * w] = 0
        b[k:600:ext, (k + 1) * w:] = 0
    order = rng.permutation(a.shape[0])[:_ragged(a.shape[0] - 1)]
    a, b = np.ascontiguousarray(a[order]), np.ascontiguousarray(b[order])
    got = probe(op, a, b)
    want = np.empty_like(a)
    f, stride = orc.lib().orc_ext_mul, a.strides[0]
    pa, pb, pw = a.ctypes.data, b.ctypes.data, want.ctypes.data
    for i in range(a.shape[0]):
        f(field, ext, pa + i * stride, pb + i * stride, pw + i * stride)
    assert np.array_equal(got, want)


def test_rescue_sboxes(probe):
    """rp::pow7 and rp::lane_inv_sbox (csrc/rescue_dev.hpp) on 0, 1, p - 1, the alphabet and uniform elements.  The stored form is
    Montgomery: x R -> x^alpha R."""
    import rp64_util as R
    rng = np.random.default_rng(7)
    x = np.concatenate([E.u64([0, E.R64, P - 1, (P - 1) * E.R64 % P] + E.f64_alphabet()), rand_f64(rng, 1000)])
    _ragged(x.size)
    can = [v * E.R64_INV % P for v in x.tolist()]
    p7 = probe(OP_RP_POW7, x).reshape(-1)
    assert p7.tolist() == [pow(c, R.ALPHA, P) * 2**64 % P for c in can]
    inv = probe(OP_RP_INV_SBOX, x).reshape(-1)
    assert inv.tolist() == [pow(c, R.INV_ALPHA, P) * 2**64 % P for c in can]
    assert np.array_equal(probe(OP_RP_INV_SBOX, p7).reshape(-1), x)


@pytest.mark.parametrize("entry,op", [("rp_state", OP_RP_MDS_ROWS), ("rpj_state", OP_RPJ_MDS_ROWS)])
def test_rescue_mds_rows_directed(probe, entry, op):
    """rp::mds_row / rpj::mds_row, every row of one state per thread (the one-lane form, no round constants), on the directed
    states of tests/rescue_edge_util.py: for every output row the five cases of the closing canonical addition (the 64-bit
    sum wraps; is 2^64; is p; is p - 1; lies in (p, 2^64)), the two states that give the largest hi and the largest lo,
    mixed with uniform states.  Compared with the integer row product.  The lane form is not probed here (its gathers need
    full waves): tests/test_gpu_rescue_full.py runs it in the sub-tree kernels."""
    import rescue_edge_util as D
    row = D.PARAMS[D.ENTRY[entry][0]]["mds_row"]
    w = len(row)
    assert D.reachable(entry) == D.all_pairs(entry)   # every (row, case): nothing is left out silently
    directed = [D.directed_set(entry)[rc] for rc in D.all_pairs(entry)]
    # a plain + in place of the canonical addition is wrong on the wrapping states, in the row they were built for
    for (i, case), y in zip(D.all_pairs(entry), directed):
        assert (D.mds_row_plain_plus(row, y, i) != D.mds_row_value(row, y, i)) == (case in ("wrap", "wrap0", "p", "above_p"))
    rng = np.random.default_rng(w)
    states = np.concatenate([E.u64([v for y in directed + D.extra_states(w) for v in y]).reshape(-1, w),
                             rand_f64(rng, 1001 * w).reshape(-1, w)])
    order = rng.permutation(_ragged(states.shape[0]))
    states = np.ascontiguousarray(states[order])
    got = probe(op, states)
    assert got.shape == (states.shape[0], w)
    want = [[D.mds_row_value(row, y, i) for i in range(w)] for y in states.tolist()]
    assert got.tolist() == want
    assert probe(OP_F64_ADD, [0], [0]).tolist() == [[0]]   # (the op table is still in step: an old op after the new ones)


def test_probe_words_cover_every_op(probe):
    """wf_field_probe_words knows the two new ops and nothing past them."""
    import starkpack_winterfell_amd.build as b
    lib = C.CDLL(b.field_probe_path())
    wa, wb, wo = C.c_int(), C.c_int(), C.c_int()
    words = {}
    for op in range(-1, 19):
        if lib.wf_field_probe_words(op, C.byref(wa), C.byref(wb), C.byref(wo)) == 1:
            words[op] = (wa.value, wb.value, wo.value)
    assert sorted(words) == list(range(17))
    assert words[OP_RP_MDS_ROWS] == (12, 0, 12) and words[OP_RPJ_MDS_ROWS] == (8, 0, 8) and words[OP_RP_INV_SBOX] == (1, 0, 1)


@pytest.mark.parametrize("n", [1, 63, 65, 255, 257, 1000])
def test_launch_edges(probe, n):
    """One lane, one lane short of / past a wave, one short of / past a work-group, several work-groups with a partial last one:
    exactly n results, nothing behind them (probe() checks the poisoned tail)."""
    al = E.f64_alphabet()
    a = E.u64([al[(7 * i) % 43] for i in range(n)])
    b = E.u64([al[(11 * i + 3) % 43] for i in range(n)])
    assert probe(OP_F64_MUL, a, b).reshape(-1).tolist() == [x * y * E.R64_INV % P for x, y in zip(a.tolist(), b.tolist())]
    a128 = E.alphabet_array(F128)[np.arange(n) * 13 % 6535]
    b128 = E.alphabet_array(F128)[(np.arange(n) * 17 + 5) % 6535]
    assert E.f128_ints(probe(OP_F128_MUL, a128, b128)) == [x * y % Q for x, y in zip(E.f128_ints(a128), E.f128_ints(b128))]
