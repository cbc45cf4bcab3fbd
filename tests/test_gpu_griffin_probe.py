"""GPU: the two Griffin ops of libwf_field_probe.so (csrc/field_probe.hip) -- gfj::linear and gfj::nonlinear of
csrc/griffin_dev.hpp as the DEVICE compiler emits them, one element per thread -- on the directed operands of
tests/griffin_edge_util.py and on operands from the limb alphabet of tests/edge_util.py, mixed with uniform ones, against
Python integers.  Every launch ends in a partial wave in front of a poisoned tail.  Ops 17..31 stay unknown."""
import ctypes as C

import numpy as np
import pytest

import edge_util as E
import griffin_edge_util as D
import griffin_util as G

pytestmark = pytest.mark.gpu
P = G.P
OP_GFJ_LINEAR, OP_GFJ_NONLINEAR = 32, 33
POISON = 0xA5A5A5A5A5A5A5A5
TAIL = 333  # poisoned elements behind the n the kernel may write


@pytest.fixture(autouse=True)
def _budget():
    before = G.PERMUTATIONS
    yield
    assert G.PERMUTATIONS - before <= 2048


@pytest.fixture(scope="module")
def lib():
    import starkpack_winterfell_amd.build as b
    import starkpack_winterfell_amd.capi as capi
    capi.load()  # the HIP runtime torch ships, loaded the way the product library needs it
    lib = C.CDLL(b.field_probe_path())
    lib.wf_field_probe.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t]
    lib.wf_field_probe.restype = C.c_int
    lib.wf_field_probe_words.argtypes = [C.c_int] + [C.POINTER(C.c_int)] * 3
    lib.wf_field_probe_words.restype = C.c_int
    return lib


def _run(lib, op, a, words_in, words_out):
    wa, wb, wo = C.c_int(), C.c_int(), C.c_int()
    assert lib.wf_field_probe_words(op, C.byref(wa), C.byref(wb), C.byref(wo)) == 1
    assert (wa.value, wb.value, wo.value) == (words_in, 0, words_out)
    a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, words_in)
    n = a.shape[0]
    assert n % 64 != 0 and n % 256 != 0, "the launch must end in a partial wave"
    out = np.full((n + TAIL, words_out), POISON, dtype=np.uint64)
    rc = lib.wf_field_probe(0, op, a.ctypes.data, None, out.ctypes.data, n, n + TAIL)
    assert rc == 0, f"hip error {rc}"
    assert (out[n:] == np.uint64(POISON)).all(), "the kernel wrote behind element n"
    return out[:n]


def test_linear_on_directed_and_alphabet_operands(lib):
    """i, z0, z1, t -> l as raw residues: every (i, case) of the function alone in two draws, every triple of a reduced limb
    alphabet for every i, and uniform operands, shuffled."""
    rng = np.random.default_rng(32)
    ops = [(i, *D.operands(i, c, draw)) for draw in (0, 1) for i in range(2, 8) for c in D.cases(i)]
    assert {(i, D.classify(i, *r)) for i, *r in ops} == {(i, c) for i in range(2, 8) for c in D.cases(i)}
    alphabet = [v for v in E.f64_alphabet() if v < P][::max(1, len(E.f64_alphabet()) // 9)][:9] + [0, P - 1, 2**32 - 1]
    ops += [(i, a, b, c) for i in range(2, 8) for a in alphabet for b in alphabet for c in alphabet[::3]]
    uni = rng.integers(0, P, size=(3001, 3), dtype=np.uint64)
    ops += [(2 + k % 6, int(r[0]), int(r[1]), int(r[2])) for k, r in enumerate(uni)]
    ops = [ops[j] for j in rng.permutation(len(ops))]
    if len(ops) % 64 == 0 or len(ops) % 256 == 0:
        ops.append((7, P - 1, P - 1, P - 1))
    got = _run(lib, OP_GFJ_LINEAR, np.array(ops, dtype=np.uint64), 4, 1)[:, 0]
    want = np.array([G.linear(i, a, b, c) for i, a, b, c in ops], dtype=np.uint64)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(ops[j], D.classify(*ops[j])) for j in bad[:5]]
    assert (got < np.uint64(P)).all()


def test_linear_refuses_no_i_silently(lib):
    """An i outside 2..7 is not a step of the layer: the op writes 0 for it (and still nothing behind n)."""
    ops = np.array([[i, 5, 6, 7] for i in (0, 1, 8, 2**40)] + [[2, 5, 6, 7]], dtype=np.uint64)
    assert _run(lib, OP_GFJ_LINEAR, ops, 4, 1)[:, 0].tolist() == [0, 0, 0, 0, 18]


def test_nonlinear_on_directed_and_alphabet_states(lib):
    """8 residues in, 8 out: the states in front of a layer that meets every (i, case) a whole state reaches (two draws),
    states from the limb alphabet, the extreme states, and uniform ones."""
    rng = np.random.default_rng(33)
    R, R_INV = D.R, D.R_INV
    states = [D.stored(s) for draw in (0, 1) for s in D.merge_states(draw).values()]     # as residues
    alphabet = [v for v in E.f64_alphabet() if v < P]
    states += [[alphabet[int(x)] for x in rng.integers(0, len(alphabet), size=8)] for _ in range(120)]
    states += [[0] * 8, [P - 1] * 8, [R] * 8, [2**32 - 1] * 8, [P - 1] * 7 + [0], [0] + [P - 1] * 7]
    states += [[int(x) for x in r] for r in rng.integers(0, P, size=(201, 8), dtype=np.uint64)]
    states = [states[j] for j in rng.permutation(len(states))]
    if len(states) % 64 == 0 or len(states) % 256 == 0:
        states.append([1] * 8)
    got = _run(lib, OP_GFJ_NONLINEAR, np.array(states, dtype=np.uint64), 8, 8)
    want = np.array([[x * R % P for x in G.nonlinear([r * R_INV % P for r in s])] for s in states], dtype=np.uint64)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, [states[j] for j in bad[:3]]
    assert (got < np.uint64(P)).all()


def test_ops_17_to_31_stay_unknown(lib):
    wa, wb, wo = C.c_int(), C.c_int(), C.c_int()
    known = [op for op in range(-1, 40) if lib.wf_field_probe_words(op, C.byref(wa), C.byref(wb), C.byref(wo)) == 1]
    assert known == list(range(17)) + [32, 33]
    a = np.zeros(8, dtype=np.uint64)
    out = np.full(8, POISON, dtype=np.uint64)
    for op in list(range(17, 32)) + [34]:
        assert lib.wf_field_probe(0, op, a.ctypes.data, None, out.ctypes.data, 1, 8) != 0
        assert (out == np.uint64(POISON)).all()
