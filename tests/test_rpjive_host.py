"""CPU: the RpJive64_256 of csrc/rescue_jive_dev.hpp (what the RpJive row, tree and grind kernels run) against
tests/rpjive_util.py, the restatement of the function on Python integers, and against the reference's one literal known
answer (tests/golden/rpjive64_256_kat.json).  Built with plain g++: the functions are __host__ __device__.  Both forms of
the permutation go through every state: `P` is the one-lane-per-permutation code, `Q` the host side of the lane form; `M`
and `L` are the two forms of the Jive compression.
`D` requests run the linear layer alone, in both forms, on the directed states of tests/rescue_edge_util.py (the closing
addition of mds_row in each of its five cases, for every output row)."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import rescue_edge_util as D
import rpjive_util as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = R.P
LENGTHS = [0, 1, 3, 4, 5, 7, 8, 9, 12, 13]  # 5 .. 7 catch "pad by addition", 4 and 8 a wrong state[0]
EDGES = [0, 1, P - 1, 2**32 - 1]
INT_VALUES = [0, P - 1, P, P + 2, 2**64 - 1]


def _golden(name):
    return json.load(open(os.path.join(ROOT, "tests", "golden", name)))


def _build(tmp_path, extra=()):
    exe = str(tmp_path / "test_rpjive_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", *extra, "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_rpjive_host.cpp")])
    return exe


def _edge_states():
    states = [[e] * 8 for e in EDGES]
    for k in range(4):
        states.append([EDGES[(i + k) % 4] for i in range(8)])
    states.append([P - 1] * 7 + [0])
    return states


def _requests():
    """(request line, expected list of integers) pairs; the expected side is Python integers only.  ~120 permutations."""
    rng = np.random.default_rng(18)
    out = []
    kat = _golden("rpjive64_256_kat.json")
    for op in "PQ":
        out.append((op, kat["input"], kat["expected"]))
    for s in _edge_states() + [[int(x) for x in rng.integers(0, P, size=8, dtype=np.uint64)] for _ in range(3)]:
        want = R.permute(s)
        for op in "PQ":
            out.append((op, s, want))
    for n in LENGTHS:
        e = [int(x) for x in rng.integers(0, P, size=n, dtype=np.uint64)]
        out.append(("H", e, R.hash_elements(e)))
    for n in (1, 4, 5, 8, 9):  # the same lengths on edge values: additions that wrap and that land in [p, 2^64)
        e = [EDGES[(i + n) % 4] for i in range(n)]
        out.append(("H", e, R.hash_elements(e)))
        e = [P - 1] * n
        out.append(("H", e, R.hash_elements(e)))
    # merge: canonical random words; words >= p (read as BaseElement::new reads them: reduced); all-zero digests
    merges = [[int(x) for x in rng.integers(0, P, size=8, dtype=np.uint64)] for _ in range(2)]
    merges += [[0] * 8, [P - 1] * 8, [P, P + 1, 2**64 - 1, 2**64 - 2**32, 0, 1, P - 1, 2**32 - 1]]
    for m in merges:
        want = R.merge_words(m)
        assert want == R.merge_words([x % P for x in m])
        out.append(("M", m, want))
        out.append(("L", m, want))
    seeds = [[int(x) for x in rng.integers(0, P, size=4, dtype=np.uint64)], [P, 2**64 - 1, 0, P - 1]]
    for seed in seeds:
        for v in INT_VALUES:
            out.append(("I", seed + [v], R.merge_with_int_words(seed, v)))
    # the directed states: the linear layer alone in both forms, and the whole permutation from the state in front of the
    # first S-box (its first linear layer meets the case)
    out += _directed_requests()
    for rc in D.all_pairs("rpj_state")[::5]:   # case 1 of every row
        c = D.preimage("rpjive64_256", D.directed_set("rpj_state")[rc])
        want = R.permute(c)
        for op in "PQ":
            out.append((op, c, want))
    return out


def _directed_requests(only=None):
    """`D` requests: the directed states of tests/rescue_edge_util.py -- for every output row the five cases of mds_row's closing
    addition, flagged where the 64-bit sum wraps (case 1) -- and the two extreme states, through both forms of the linear
    layer (expected: the integer row product plus ARK1 of round 0, as residues)."""
    row = D.PARAMS["rpjive64_256"]["mds_row"]
    w = len(row)
    ark1 = [x * 2**64 % P for x in D.PARAMS["rpjive64_256"]["ark1"][0]]
    assert D.reachable("rpj_state") == D.all_pairs("rpj_state")
    out = []
    for (i, case), y in [(rc, D.directed_set("rpj_state")[rc]) for rc in D.all_pairs("rpj_state")] + \
            [((0, "extra"), y) for y in D.extra_states(w)]:
        if only is not None and case not in only:
            continue
        want = [(D.mds_row_value(row, y, r) + ark1[r]) % P for r in range(w)]
        out.append(("D", [i, int(case == "wrap")] + list(y), want + want))
    return out


def _ask(exe, lines, env=None):
    res = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    return [[int(x) for x in l.split()] for l in res.stdout.splitlines()]


_CASES = None


def _run(exe, env=None):
    global _CASES
    if _CASES is None:
        _CASES = _requests()  # the Python reference once, shared by the plain and the sanitizer run
    got = _ask(exe, [" ".join([op] + [str(x) for x in words]) for op, words, _ in _CASES], env)
    assert len(got) == len(_CASES)
    for (op, words, want), g in zip(_CASES, got):
        assert g == want, f"{op} request of {len(words)} words"
    # the Jive compression is not the sponge: merge(a, b) != hash_elements(a || b)
    words = [str(x) for x in range(11, 19)]
    m, h, z = _ask(exe, ["M " + " ".join(words), "H " + " ".join(words), "H"], env)
    assert m != h and m == R.merge_words(range(11, 19)) and h == R.hash_elements(list(range(11, 19)))
    assert z == [0, 0, 0, 0]  # no element: the zero digest
    # the plan of the tree: every sequence sound (34 sizes x 5 tuning values x 4 CU counts)
    (k,) = _ask(exe, ["K"], env)
    assert k == [34 * 5 * 4, 0]


def test_rpjive64_256_matches_the_python_reference(tmp_path):
    _run(_build(tmp_path))


def test_rpjive64_256_under_address_and_ub_sanitizers(tmp_path):
    """The same stand-alone program with -fsanitize=address,undefined (nothing is preloaded: it has its own main)."""
    try:
        exe = _build(tmp_path, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    except subprocess.CalledProcessError:
        pytest.skip("this g++ has no sanitizer runtime")
    _run(exe, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))


def test_directed_states_must_tell_the_plain_plus_copy_apart(tmp_path):
    """The program's own guard: D requests without the wrapping states of some row end it with exit status 4."""
    exe = _build(tmp_path)
    reqs = _directed_requests(only=("p", "p-1", "above_p", "extra"))
    lines = [" ".join([op] + [str(x) for x in words]) for op, words, _ in reqs]
    res = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert res.returncode == 4 and "plain-+ copy" in res.stderr
    # the wrapping states of every row but the last: still refused, and the message names the row
    w = len(D.PARAMS["rpjive64_256"]["mds_row"])
    some = [r for r in _directed_requests(only=("wrap",)) if r[1][0] != w - 1]
    lines = [" ".join([op] + [str(x) for x in words]) for op, words, _ in some]
    res = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert res.returncode == 4 and f"row {w - 1}" in res.stderr


def test_header_tables_are_the_fixture_in_montgomery_form(tmp_path):
    prm = _golden("rpjive64_256_params.json")
    (t,) = _ask(_build(tmp_path), ["T"])
    assert len(t) == 56 + 56 + 8
    flat1 = [x for row in prm["ark1"] for x in row]
    flat2 = [x for row in prm["ark2"] for x in row]
    assert t[:56] == [x * 2**64 % P for x in flat1]
    assert t[56:112] == [x * 2**64 % P for x in flat2]
    assert t[112:] == prm["mds_row"] == [23, 8, 13, 10, 7, 6, 21, 8]
    assert prm["alpha"] == 7 and prm["alpha"] * prm["inv_alpha"] % (P - 1) == 1
    assert prm["state_width"] == 8 and sum(prm["mds_row"]) == 96


def test_python_reference_reproduces_the_known_answer():
    kat = _golden("rpjive64_256_kat.json")
    assert R.permute(kat["input"]) == kat["expected"]
    # the padding is set, not added: the second block of a 5-element input overwrites the first permutation's output
    e = [3, 1, 4, 1, 5]
    first = R.permute([1, 0, 0, 0, 3, 1, 4, 1])
    assert R.hash_elements(e) == R.permute(first[:4] + [(first[4] + 5) % P, 1, 0, 0])[4:8]
    assert R.hash_elements([]) == [0, 0, 0, 0]
    # helpers of the GPU tests: a tree of four leaves by hand, the sampled set within its budget
    leaves = np.arange(4 * 32, dtype=np.uint8).reshape(4, 32)
    nodes = R.merkle_nodes(leaves)
    assert not nodes[0].any()
    assert bytes(nodes[1]) == R.merge(R.merge(bytes(leaves[0]), bytes(leaves[1])), R.merge(bytes(leaves[2]), bytes(leaves[3])))
    R.check_tree_sampled(nodes, leaves, [1, 2, 3])
    assert R.verify_path(bytes(nodes[1]), 2, [bytes(leaves[2]), bytes(leaves[3]), bytes(nodes[2])])
    for log_n in (9, 16, 17, 18):
        idx = R.sample_indices(1 << log_n, spans=(128,))
        assert len(idx) == len(set(idx)) <= 2048 and all(1 <= i < (1 << log_n) for i in idx)
    # merge_with_int: both branches differ from each other and from merge
    seed = bytes(range(32))
    assert R.merge_with_int(seed, P - 1) != R.merge_with_int(seed, 2**64 - 1)
    assert R.merge_with_int_words([1, 2, 3, 4], P + 2) == R.merge_words([1, 2, 3, 4, 2, 1, 0, 6])
    assert R.merge_with_int_words([1, 2, 3, 4], 9) == R.merge_words([1, 2, 3, 4, 9, 0, 0, 5])


def test_params_check_knows_rpjive64_256(capi):
    lib = capi.load()
    assert capi.RPJIVE64_256 == 18

    def check(**kw):
        field = kw.pop("field", capi.F64)
        return lib.wf_params_check(ctypes.byref(capi.make_params(field, 1, 10, 3, 8, 1, **kw)), 0)

    assert check(hasher=capi.RPJIVE64_256) == 0
    for ext in (2, 3):
        assert lib.wf_params_check(ctypes.byref(capi.make_params(capi.F64, ext, 10, 3, 2, 1, hasher=capi.RPJIVE64_256)), 0) == 0
    assert check(digest_bytes=24, hasher=capi.RPJIVE64_256) == -31
    assert b"RpJive64_256" in lib.wf_last_error()
    assert check(field=capi.F128, hasher=capi.RPJIVE64_256) == -10
    assert b"RpJive64_256" in lib.wf_last_error()
    for unknown in (17, 19):
        assert check(hasher=unknown) == -31
        assert b"hasher" in lib.wf_last_error()
