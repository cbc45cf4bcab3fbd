"""CPU: the GriffinJive64_256 of csrc/griffin_dev.hpp (what the Griffin row, tree and grind kernels run) against its two
references -- tests/griffin_util.py, the function on Python integers, and tests/cpp/griffin_ref.c, the plain C one -- and
against the reference's two literal known answers (tests/golden/griffinjive64_256_kat.json).  The header is built with
plain g++ into a stand-alone, request-driven program (tests/cpp/test_griffin_host.cpp): the functions are __host__
__device__.  `D` requests run gfj::linear alone on the directed operands of tests/griffin_edge_util.py; directed whole
states go through permute, hash_elements, merge and merge_with_int.

Budgets, asserted by counting: at most 2048 Python permutations and 2^18 C-reference permutations per test."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import griffin_edge_util as D
import griffin_util as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = G.P
LENGTHS = [0, 1, 3, 4, 5, 7, 8, 9, 12, 13]  # 5 .. 7 catch "pad by addition", 4 and 8 a wrong state[4]
EDGES = [0, 1, P - 1, 2**32 - 1]
INT_VALUES = [0, P - 1, P, P + 2, 2**64 - 1]
PY_BUDGET, C_BUDGET = 2048, 1 << 18


@pytest.fixture(autouse=True)
def _budget():
    before = G.PERMUTATIONS
    yield
    assert G.PERMUTATIONS - before <= PY_BUDGET, f"{G.PERMUTATIONS - before} Python permutations in one test"


@pytest.fixture()
def cref():
    c = G.CRef()
    yield c
    assert c.spent <= C_BUDGET, f"{c.spent} C-reference permutations in one test"


def _golden(name):
    return json.load(open(os.path.join(ROOT, "tests", "golden", name)))


def _build(tmp_path, extra=()):
    exe = str(tmp_path / "test_griffin_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", *extra, "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_griffin_host.cpp")])
    return exe


def _edge_states():
    """All 0 / 1 / p - 1 / 2^32 - 1, and the four values in rotation."""
    states = [[e] * 8 for e in EDGES]
    for k in range(4):
        states.append([EDGES[(i + k) % 4] for i in range(8)])
    states.append([P - 1] * 7 + [0])
    return states


def _random_states(n, seed=20):
    rng = np.random.default_rng(seed)
    return [[int(x) for x in rng.integers(0, P, size=8, dtype=np.uint64)] for _ in range(n)]


def _merges():
    rng = np.random.default_rng(21)
    m = [[int(x) for x in rng.integers(0, P, size=8, dtype=np.uint64)] for _ in range(2)]
    return m + [[0] * 8, [P - 1] * 8, [P, P + 1, 2**64 - 1, 2**64 - 2**32, 0, 1, P - 1, 2**32 - 1]]


def _seeds():
    rng = np.random.default_rng(22)
    return [[int(x) for x in rng.integers(0, P, size=4, dtype=np.uint64)], [P, 2**64 - 1, 0, P - 1]]


def _rows():
    rng = np.random.default_rng(23)
    rows = [[int(x) for x in rng.integers(0, P, size=n, dtype=np.uint64)] for n in LENGTHS]
    for n in (1, 4, 5, 8, 9):  # the same lengths on edge values: additions that wrap and that land in [p, 2^64)
        rows.append([EDGES[(i + n) % 4] for i in range(n)])
        rows.append([P - 1] * n)
    return rows


def _directed_linear_requests(only=None):
    out = []
    for i, case, (r0, r1, r2) in D.directed_linear():
        if only is not None and not only(i, case, r0, r1, r2):
            continue
        out.append(("D", [i, r0, r1, r2], [G.linear(i, r0, r1, r2)]))
    return out


# the (i, case) pairs each entry point reaches in its first non-linear layer, written out: every i for merge, i = 2, 3, 4 for
# a row of one rate block (only places 0..3 are the caller's), i = 2..5 for merge_with_int (places 0..4)
def _pairs(i_values):
    out = []
    for i in i_values:
        base = ["below_p", "p-1", "p", "above_p", "2^64"]
        if i == 2:   # t = 0: S <= 2 (p - 1), high word 1 at most and no carry under it
            out += [(2, c) for c in base + ["hi1"]]
        else:
            out += [(i, c) for c in base + ["hi%d" % h for h in range(1, i + 1)] + ["hi%dc" % h for h in range(1, i)] + ["all_p-1"]]
    return out


REACHABLE = {"merge": _pairs(range(2, 8)), "row": _pairs([2, 3, 4]), "merge_with_int": _pairs([2, 3, 4, 5])}


def _requests():
    """(request line, expected list of integers) pairs; the expected side is Python integers only."""
    out = []
    kat = _golden("griffinjive64_256_kat.json")
    out.append(("P", kat["permutation"]["input"], kat["permutation"]["expected"]))
    out.append(("H", kat["hash_elements"]["input"], kat["hash_elements"]["expected"]))
    for s in _edge_states() + _random_states(100):
        out.append(("P", s, G.permute(s)))
    for s in _edge_states() + _random_states(8, seed=24):
        out.append(("N", s, G.nonlinear(s)))
    for e in _rows():
        out.append(("H", e, G.hash_elements(e)))
    for m in _merges():
        want = G.merge_words(m)
        assert want == G.merge_words([x % P for x in m])
        out.append(("M", m, want))
    for seed in _seeds():
        for v in INT_VALUES:
            out.append(("I", seed + [v], G.merge_with_int_words(seed, v)))
    out += _directed_linear_requests()
    # directed whole states: each entry point on the states whose first non-linear layer meets each (i, case) it reaches
    for entry in ("merge", "row", "merge_with_int"):
        assert D.reachable(entry) == REACHABLE[entry]
    for rc, s in D.merge_states().items():
        out.append(("P", s, G.permute(s)))
        out.append(("M", s, G.merge_words(s)))
    for rc, e in D.row_states().items():
        out.append(("H", e, G.hash_elements(e)))
        out.append(("H", e + [7], G.hash_elements(e + [7])))   # a row of more than one block: the first block is the same
    for rc, sv in D.seed_states().items():
        assert sv[4] < P
        out.append(("I", sv, G.merge_with_int_words(sv[:4], sv[4])))
    return out


def _ask(exe, lines, env=None):
    res = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    return [[int(x) for x in l.split()] for l in res.stdout.splitlines()]


_CASES = None


def _cases():
    global _CASES
    if _CASES is None:
        _CASES = _requests()  # the Python reference once, shared by the plain and the sanitizer run
    return _CASES


def _run(exe, env=None):
    cases = _cases()
    got = _ask(exe, [" ".join([op] + [str(x) for x in words]) for op, words, _ in cases], env)
    assert len(got) == len(cases)
    for (op, words, want), g in zip(cases, got):
        assert g == want, f"{op} request {words}"
    # the Jive compression is not the sponge: merge(a, b) != hash_elements(a || b)
    words = [str(x) for x in range(11, 19)]
    m, h, z = _ask(exe, ["M " + " ".join(words), "H " + " ".join(words), "H"], env)
    assert m != h and m == G.merge_words(range(11, 19)) and h == G.hash_elements(list(range(11, 19)))
    assert z == [0, 0, 0, 0]  # no element: the zero digest
    # the plan of the tree: every sequence sound (34 sizes x 5 tuning values x 4 CU counts)
    (k,) = _ask(exe, ["K"], env)
    assert k == [34 * 5 * 4, 0]


def test_griffinjive64_256_matches_the_python_reference(tmp_path):
    _run(_build(tmp_path))


def test_griffinjive64_256_under_address_and_ub_sanitizers(tmp_path):
    """The same stand-alone program with -fsanitize=address,undefined (nothing is preloaded: it has its own main)."""
    exe = _build(tmp_path, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    _run(exe, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))


def test_directed_operands_must_tell_the_uncorrected_copy_apart(tmp_path):
    """The program's own guard: D requests none of which needs the last correction end it with exit status 4; so does a set
    that leaves one i without such an operand, and the message names it.  The full set covers every i = 2..7."""
    exe = _build(tmp_path)
    for i in range(2, 8):
        assert any(D.needs_correction(j, *r) for j, _, r in D.directed_linear() if j == i)
        assert [c for j, c, _ in D.directed_linear() if j == i] == D.cases(i)

    def ask(reqs):
        lines = [" ".join([op] + [str(x) for x in words]) for op, words, _ in reqs]
        return subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)

    res = ask(_directed_linear_requests(only=lambda i, c, *r: not D.needs_correction(i, *r)))
    assert res.returncode == 4 and "uncorrected copy" in res.stderr
    res = ask(_directed_linear_requests(only=lambda i, c, *r: i != 7 or not D.needs_correction(i, *r)))
    assert res.returncode == 4 and "i = 7" in res.stderr
    assert ask(_directed_linear_requests()).returncode == 0


def test_header_tables_are_the_fixture_in_montgomery_form(tmp_path):
    prm = _golden("griffinjive64_256_params.json")
    (t,) = _ask(_build(tmp_path), ["T"])
    assert len(t) == 48 + 6 + 6 + 8
    flat = [x for row in prm["ark"] for x in row]
    assert len(prm["ark"]) == 6 and all(len(r) == 8 for r in prm["ark"])
    assert t[:48] == [x * 2**64 % P for x in flat]
    assert t[48:54] == [x * 2**64 % P for x in prm["alpha_i"]]
    assert t[54:60] == [x * 2**64 % P for x in prm["beta_i"]]
    assert t[60:] == prm["mds_row"] == [23, 8, 13, 10, 7, 6, 21, 8]
    assert prm["alpha"] == 7 and 7 * prm["inv_alpha"] % (P - 1) == 1
    assert prm["state_width"] == 8 and prm["num_rounds"] == 7 and prm["rate_range"] == [0, 4] and prm["digest_range"] == [0, 4]


def test_python_reference_reproduces_the_known_answers():
    kat = _golden("griffinjive64_256_kat.json")
    assert G.permute(kat["permutation"]["input"]) == kat["permutation"]["expected"]
    assert G.hash_elements(kat["hash_elements"]["input"]) == kat["hash_elements"]["expected"]
    # the padding is set, not added: the second block of a 5-element input overwrites the first permutation's output
    e = [3, 1, 4, 1, 5]
    first = G.permute([3, 1, 4, 1, 1, 0, 0, 0])
    assert G.hash_elements(e) == G.permute([(first[0] + 5) % P, 1, 0, 0] + first[4:])[:4]
    assert G.hash_elements([]) == [0, 0, 0, 0]
    assert G.hash_elements([1, 2, 3, 4]) == G.permute([1, 2, 3, 4, 0, 0, 0, 0])[:4]   # a multiple of 4: state[4] stays 0
    # helpers of the GPU tests: a tree of four leaves by hand, a path cut from it
    leaves = np.arange(4 * 32, dtype=np.uint8).reshape(4, 32)
    nodes = G.merkle_nodes(leaves)
    assert not nodes[0].any()
    assert bytes(nodes[1]) == G.merge(G.merge(bytes(leaves[0]), bytes(leaves[1])), G.merge(bytes(leaves[2]), bytes(leaves[3])))
    assert G.cut_path(nodes, leaves, 2) == [bytes(leaves[2]), bytes(leaves[3]), bytes(nodes[2])]
    assert G.verify_path(bytes(nodes[1]), 2, G.cut_path(nodes, leaves, 2))
    assert not G.verify_path(bytes(nodes[1]), 1, G.cut_path(nodes, leaves, 2))
    # merge_with_int: both branches differ from each other and from merge
    seed = bytes(range(32))
    assert G.merge_with_int(seed, P - 1) != G.merge_with_int(seed, 2**64 - 1)
    assert G.merge_with_int_words([1, 2, 3, 4], P + 2) == G.merge_words([1, 2, 3, 4, 2, 1, 0, 6])
    assert G.merge_with_int_words([1, 2, 3, 4], 9) == G.merge_words([1, 2, 3, 4, 9, 0, 0, 5])


def test_c_reference_matches_python(cref):
    """tests/cpp/griffin_ref.c against the Python integers: both known answers, 100 random states, the edge states, every
    row length, merges with words >= p, both branches of merge_with_int, a 2^6-leaf tree, a short nonce search, and
    merge != hash_elements of the same words."""
    kat = _golden("griffinjive64_256_kat.json")
    assert cref.permute(kat["permutation"]["input"]) == kat["permutation"]["expected"]
    assert cref.hash_elements(kat["hash_elements"]["input"]) == kat["hash_elements"]["expected"]
    for s in _edge_states() + _random_states(100):
        assert cref.permute(s) == G.permute(s), s
    for e in _rows():
        assert cref.hash_elements(e) == G.hash_elements(e), e
    rows = np.array([D.stored(e) for e in _rows() if len(e) == 5], dtype=np.uint64)
    assert np.array_equal(cref.hash_rows(rows), G.hash_rows(rows))
    assert not cref.hash_rows(np.zeros((3, 0), dtype=np.uint64)).any()   # no element: zero digests
    for m in _merges():
        assert cref.merge_words(m) == G.merge_words(m), m
    for seed in _seeds():
        for v in INT_VALUES:
            sb = G.digest_bytes_raw(seed)
            assert cref.merge_with_int(sb, v) == G.digest_bytes(G.merge_with_int_words(seed, v)), (seed, v)
    leaves = np.random.default_rng(6).integers(0, 2**64, size=(64, 4), dtype=np.uint64).view(np.uint8).reshape(64, 32)
    assert np.array_equal(cref.merkle_nodes(leaves), G.merkle_nodes(leaves))
    words = list(range(11, 19))
    assert cref.merge_words(words) == G.merge_words(words) != G.hash_elements(words) == cref.hash_elements(words)
    seed = bytes(range(32))
    n = G.grind(seed, 6, 1, 400)
    assert n is not None and cref.grind(seed, 6, 1, 400) == (n, G.merge_with_int(seed, n))
    assert cref.grind(seed, 6, 1, n - 1) == (None, None)
    assert cref.grind(seed, 0, P - 3, 8)[0] == P - 3 and cref.grind(seed, 0, 2**64 - 1, 5) == (2**64 - 1, G.merge_with_int(seed, 2**64 - 1))
    # the directed states through the C reference as well
    for rc, s in list(D.merge_states().items())[::3]:
        assert cref.merge_words(s) == G.merge_words(s), rc


def test_params_check_knows_griffinjive64_256(capi):
    lib = capi.load()
    assert capi.GRIFFINJIVE64_256 == 20

    def check(**kw):
        field = kw.pop("field", capi.F64)
        return lib.wf_params_check(ctypes.byref(capi.make_params(field, 1, 10, 3, 8, 1, **kw)), 0)

    assert check(hasher=capi.GRIFFINJIVE64_256) == 0
    for ext in (2, 3):
        assert lib.wf_params_check(ctypes.byref(capi.make_params(capi.F64, ext, 10, 3, 2, 1, hasher=capi.GRIFFINJIVE64_256)), 0) == 0
    assert check(digest_bytes=24, hasher=capi.GRIFFINJIVE64_256) == -31
    assert b"GriffinJive64_256" in lib.wf_last_error()
    assert check(field=capi.F128, hasher=capi.GRIFFINJIVE64_256) == -10
    assert b"GriffinJive64_256" in lib.wf_last_error()
    for unknown in (17, 19, 21):
        assert check(hasher=unknown) == -31
        assert b"hasher" in lib.wf_last_error()
