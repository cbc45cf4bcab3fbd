"""Test helper: what a GriffinJive64_256 commitment must contain -- the references of every GriffinJive64_256 test (never the
library, never csrc/griffin_dev.hpp).  Two of them, both from tests/golden/griffinjive64_256_params.json:

  * the function on Python integers (this file), 0.2 ms per permutation: callers keep to at most 2048 per test (PERMUTATIONS
    counts them);
  * tests/cpp/griffin_ref.c through ctypes (class CRef): canonical integers, 128-bit products reduced with %, square-and-
    multiply S-boxes.  It is built with `cc -O2 -shared -fPIC` into a temporary directory on first use; callers keep to at
    most 2^18 of its permutations per test (CRef.spent counts them).  tests/test_griffin_host.py pins it to the Python one.

The function restated (GriffinJive64_256 of the reference, crypto/src/hash/griffin/griffin64_256_jive/mod.rs):

  state: 8 elements of GF(p), p = 2^64 - 2^32 + 1; rate 0..4, capacity 4..8, digest 0..4
  permutation: for r in 0..6 { non-linear; MDS; + ARK[r] }; non-linear; MDS  (six constant rows, none behind the last round)
  non-linear: s0 = s0^inv_alpha; s1 = s1^7; for i = 2..7: l = (i-1) s0 + s1 + t, s_i *= l^2 + alpha_i[i-2] l + beta_i[i-2],
               with the new s0, s1, t = 0 for i = 2 and the new s_{i-1} behind it
  MDS circulant: out[i] = sum_j row[(j - i) mod 8] * in[j]
  hash_elements: state[4] = 1 iff the number of base elements is no multiple of 4; elements added into places 0..3 four at a
               time, a permutation behind every full block; a partial block of i elements: place i SET to 1, the places
               behind it up to 3 SET to 0, one more permutation; no elements: the zero digest
  merge(a, b): init = a || b, fin = permute(init), out[i] = init[i] + init[4+i] + fin[i] + fin[4+i]
  merge_with_int(seed, v): init = seed || v mod p, [v // p], 0, 5 [6]; then as merge
  digest bytes = the four elements as canonical little-endian u64; digest words read are reduced mod p"""
import ctypes
import json
import os
import subprocess
import tempfile

import numpy as np

from rp64_util import canonical, digest_bytes, digest_words, sample_indices  # noqa: F401  (shared with the Rescue tests)

F64 = 1
P = 2**64 - 2**32 + 1
W = 8
HERE = os.path.dirname(os.path.abspath(__file__))
PARAMS_JSON = os.path.join(HERE, "golden", "griffinjive64_256_params.json")
_PRM = json.load(open(PARAMS_JSON))
ALPHA, INV_ALPHA, ROW, ARK = _PRM["alpha"], _PRM["inv_alpha"], _PRM["mds_row"], _PRM["ark"]
ALPHA_I, BETA_I = _PRM["alpha_i"], _PRM["beta_i"]
PERMUTATIONS = 0  # counted, so that a test can assert its budget


def linear(i, z0, z1, t):
    return ((i - 1) * z0 + z1 + t) % P


def quad(i, l):
    """The factor of the quadratic step on state element i (2..7)."""
    return (l * l + ALPHA_I[i - 2] * l + BETA_I[i - 2]) % P


def nonlinear(state):
    s = [int(x) % P for x in state]
    s[0] = pow(s[0], INV_ALPHA, P)
    s[1] = pow(s[1], ALPHA, P)
    for i in range(2, W):
        s[i] = s[i] * quad(i, linear(i, s[0], s[1], s[i - 1] if i > 2 else 0)) % P
    return s


def _mds(s):
    return [sum(ROW[(j - i) % W] * s[j] for j in range(W)) % P for i in range(W)]


def permute(state):
    global PERMUTATIONS
    PERMUTATIONS += 1
    s = [int(x) % P for x in state]
    assert len(s) == W
    for r in range(7):
        s = _mds(nonlinear(s))
        if r < 6:
            s = [(x + k) % P for x, k in zip(s, ARK[r])]
    return s


def hash_elements(elems):
    """elems: canonical integers (any integer is reduced mod p) -> the digest as 4 canonical integers."""
    s = [0] * W
    if len(elems) % 4 != 0:
        s[4] = 1
    i = 0
    for e in elems:
        s[i] = (s[i] + int(e)) % P
        i += 1
        if i == 4:
            s = permute(s)
            i = 0
    if i:
        s[i] = 1
        for k in range(i + 1, 4):
            s[k] = 0
        s = permute(s)
    return s[0:4]


def _jive(init):
    init = [int(x) % P for x in init]
    fin = permute(init)
    return [(init[i] + init[4 + i] + fin[i] + fin[4 + i]) % P for i in range(4)]


def merge_words(words):
    """The 8 digest words of a || b (any u64) -> the digest as 4 canonical integers."""
    assert len(words) == 8
    return _jive(words)


def merge(a: bytes, b: bytes) -> bytes:
    return digest_bytes(merge_words(digest_words(a) + digest_words(b)))


def merge_with_int_words(seed_words, v):
    v = int(v)
    assert 0 <= v < 2**64
    init = [int(x) % P for x in seed_words] + [v % P, 0, 0, 0]
    if v < P:
        init[7] = 5
    else:
        init[5] = v // P
        init[7] = 6
    return _jive(init)


def merge_with_int(seed: bytes, v: int) -> bytes:
    return digest_bytes(merge_with_int_words(digest_words(seed), v))


def hash_row(row) -> bytes:
    """One row of stored (Montgomery) base elements -> digest bytes."""
    return digest_bytes(hash_elements(canonical(row)))


def hash_rows(rows) -> np.ndarray:
    rows = np.asarray(rows, dtype=np.uint64)
    return np.array([np.frombuffer(hash_row(rows[j]), dtype=np.uint8) for j in range(rows.shape[0])]).reshape(-1, 32)


def perms_of_row(k):
    return -(-k // 4)


def combined_row(ldes, epr, j) -> list:
    """Row j of every trace's LDE, the first epr elements of each (padding lanes are not hashed), canonical."""
    out = []
    for m in ldes:
        out += canonical(np.asarray(m, dtype=np.uint64)[j, :epr])
    return out


def merkle_nodes(leaves) -> np.ndarray:
    """MerkleTree::nodes for (n, 32) leaves: nodes[0] = zero digest, nodes[1] = root, nodes[i] = merge(nodes[2i], nodes[2i+1])."""
    lv = np.asarray(leaves, dtype=np.uint8).reshape(-1, 32)
    n = lv.shape[0]
    dig = [b""] * n + [bytes(x) for x in lv]
    for i in range(n - 1, 0, -1):
        dig[i] = merge(dig[2 * i], dig[2 * i + 1])
    dig[0] = bytes(32)
    return np.frombuffer(b"".join(dig[:n]), dtype=np.uint8).reshape(n, 32).copy()


def verify_path(root: bytes, index: int, proof, merge_fn=None) -> bool:
    """MerkleTree::verify: proof = leaf, sibling leaf, siblings bottom-up."""
    m = merge_fn or merge
    r = index & 1
    v = m(proof[r], proof[1 - r])
    index = (index + 2 ** (len(proof) - 1)) >> 1
    for p in proof[2:]:
        v = m(v, p) if index & 1 == 0 else m(p, v)
        index >>= 1
    return v == root


def cut_path(nodes, leaves, index):
    """MerkleTree::prove from a whole tree: leaf, sibling leaf, siblings bottom-up."""
    n = leaves.shape[0]
    proof = [bytes(leaves[index]), bytes(leaves[index ^ 1])]
    k = (index + n) >> 1
    while k > 1:
        proof.append(bytes(nodes[k ^ 1]))
        k >>= 1
    return proof


def trailing_zeros_ok(digest: bytes, factor: int) -> bool:
    """DefaultRandomCoin::check_leading_zeros: the first little-endian u64 of the digest has `factor` trailing zero bits."""
    return int.from_bytes(digest[:8], "little") & ((1 << factor) - 1) == 0


def grind(seed: bytes, factor: int, begin: int, max_nonces: int):
    """The smallest nonce of [begin, begin + max_nonces) (clipped at 2^64 - 1) that qualifies, or None."""
    end = min(begin + max_nonces, 2**64)
    for v in range(begin, end):
        if trailing_zeros_ok(merge_with_int(seed, v), factor):
            return v
    return None


# ------------------------------------------------------------------------------------------------ the C reference
_TMP = None
_LIB = None


def _c_lib():
    global _TMP, _LIB
    if _LIB is None:
        _TMP = tempfile.TemporaryDirectory(prefix="griffin_ref_")
        so = os.path.join(_TMP.name, "libgriffin_ref.so")
        subprocess.check_call(["cc", "-O2", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "cpp", "griffin_ref.c")])
        lib = ctypes.CDLL(so)
        u64p, u8p = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint8)
        lib.gfr_load.argtypes, lib.gfr_load.restype = [ctypes.c_char_p], ctypes.c_int
        lib.gfr_permute.argtypes, lib.gfr_permute.restype = [u64p], None
        lib.gfr_hash_rows.argtypes, lib.gfr_hash_rows.restype = [u64p, ctypes.c_uint64, ctypes.c_uint64, u8p], None
        lib.gfr_merge.argtypes, lib.gfr_merge.restype = [u8p, u8p, u8p], None
        lib.gfr_merkle_nodes.argtypes, lib.gfr_merkle_nodes.restype = [u8p, ctypes.c_uint64, u8p], None
        lib.gfr_merge_with_int.argtypes, lib.gfr_merge_with_int.restype = [u8p, ctypes.c_uint64, u8p], None
        lib.gfr_grind.argtypes = [u8p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, u64p, u8p]
        lib.gfr_grind.restype = ctypes.c_int
        rc = lib.gfr_load(PARAMS_JSON.encode())
        assert rc == 0, f"griffin_ref.c could not read its parameters ({rc})"
        _LIB = lib
    return _LIB


def _u8(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))


def _u64(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))


class CRef:
    """tests/cpp/griffin_ref.c.  Rows are STORED (Montgomery) elements, as the library takes them; digests are bytes.  `spent`
    counts the permutations asked for since it was last set to 0."""

    def __init__(self):
        self.lib = _c_lib()
        self.spent = 0

    def permute(self, state):
        a = np.array([int(x) % P for x in state], dtype=np.uint64)
        assert a.shape == (W,)
        self.spent += 1
        self.lib.gfr_permute(_u64(a))
        return [int(x) for x in a]

    def hash_rows(self, rows) -> np.ndarray:
        a = np.ascontiguousarray(rows, dtype=np.uint64)
        n, k = a.shape
        out = np.zeros((n, 32), dtype=np.uint8)
        self.spent += n * perms_of_row(k)
        if n:
            self.lib.gfr_hash_rows(_u64(a), n, k, _u8(out))
        return out

    def hash_elements(self, elems):
        """Canonical integers -> the digest as 4 canonical integers."""
        row = np.array([[int(e) % P * 2**64 % P for e in elems]], dtype=np.uint64).reshape(1, len(elems))
        return digest_words(bytes(self.hash_rows(row)[0]))

    def merge(self, a: bytes, b: bytes) -> bytes:
        x, y = np.frombuffer(a, dtype=np.uint8).copy(), np.frombuffer(b, dtype=np.uint8).copy()
        out = np.zeros(32, dtype=np.uint8)
        self.spent += 1
        self.lib.gfr_merge(_u8(x), _u8(y), _u8(out))
        return bytes(out)

    def merge_words(self, words):
        b = digest_bytes_raw(words)
        return digest_words(self.merge(b[:32], b[32:]))

    def merkle_nodes(self, leaves) -> np.ndarray:
        lv = np.ascontiguousarray(leaves, dtype=np.uint8).reshape(-1, 32)
        n = lv.shape[0]
        out = np.zeros((n, 32), dtype=np.uint8)
        self.spent += n - 1
        self.lib.gfr_merkle_nodes(_u8(lv), n, _u8(out))
        return out

    def merge_with_int(self, seed: bytes, v: int) -> bytes:
        s = np.frombuffer(seed, dtype=np.uint8).copy()
        out = np.zeros(32, dtype=np.uint8)
        self.spent += 1
        self.lib.gfr_merge_with_int(_u8(s), int(v), _u8(out))
        return bytes(out)

    def grind(self, seed: bytes, factor: int, begin: int, max_nonces: int):
        """(smallest qualifying nonce, its digest) of [begin, begin + max_nonces) clipped at 2^64 - 1, or (None, None)."""
        s = np.frombuffer(seed, dtype=np.uint8).copy()
        nonce = ctypes.c_uint64(0)
        out = np.zeros(32, dtype=np.uint8)
        span = min(int(max_nonces), 2**64 - int(begin))
        found = self.lib.gfr_grind(_u8(s), factor, int(begin), span, ctypes.byref(nonce), _u8(out))
        self.spent += (nonce.value - begin + 1) if found else span
        return (nonce.value, bytes(out)) if found else (None, None)


def digest_bytes_raw(words) -> bytes:
    """Any u64 words as little-endian bytes (NOT reduced: what a caller may hand in)."""
    return b"".join(int(w).to_bytes(8, "little") for w in words)
