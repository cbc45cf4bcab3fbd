"""Test helper: what an RpJive64_256 commitment must contain, from Python integers alone -- the reference for every
RpJive64_256 test (never the library, never csrc/rescue_jive_dev.hpp).  The function restated (RpJive64_256 of the reference,
crypto/src/hash/rescue/rp64_256_jive/mod.rs; parameters from tests/golden/rpjive64_256_params.json):

  state: 8 elements of GF(p), p = 2^64 - 2^32 + 1; capacity 0..4, rate 4..8, digest 4..8
  permutation: 7 rounds of  x^7 | MDS | + ARK1[r] | x^inv_alpha | MDS | + ARK2[r],  MDS circulant:
               out[i] = sum_j row[(j - i) mod 8] * in[j]
  hash_elements: state[0] = 1 iff the number of base elements is no multiple of 4; elements added into the rate four at a
               time, a permutation behind every full block; a partial block of i elements: rate place i SET to 1, the
               places behind it SET to 0, one more permutation; no elements: the zero digest
  merge(a, b): init = a || b, fin = permute(init), out[i] = init[i] + init[4+i] + fin[i] + fin[4+i]
  merge_with_int(seed, v): init = seed || v mod p, [v // p], 0, 5 [6]; then as merge
  digest bytes = the four elements as canonical little-endian u64; digest words read are reduced mod p

A permutation costs a few milliseconds here: callers keep to at most 2048 of them per test (sample_indices)."""
import json
import os

import numpy as np

from rp64_util import canonical, digest_bytes, digest_words, sample_indices  # noqa: F401  (shared with the Rp64_256 tests)

F64 = 1
P = 2**64 - 2**32 + 1
W = 8
_PRM = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rpjive64_256_params.json")))
ALPHA, INV_ALPHA, ROW, ARK1, ARK2 = _PRM["alpha"], _PRM["inv_alpha"], _PRM["mds_row"], _PRM["ark1"], _PRM["ark2"]
PERMUTATIONS = 0  # counted, so that a test can assert its budget


def _mds(s):
    return [sum(ROW[(j - i) % W] * s[j] for j in range(W)) % P for i in range(W)]


def permute(state):
    global PERMUTATIONS
    PERMUTATIONS += 1
    s = [int(x) % P for x in state]
    assert len(s) == W
    for r in range(7):
        s = [pow(x, ALPHA, P) for x in s]
        s = [(x + k) % P for x, k in zip(_mds(s), ARK1[r])]
        s = [pow(x, INV_ALPHA, P) for x in s]
        s = [(x + k) % P for x, k in zip(_mds(s), ARK2[r])]
    return s


def hash_elements(elems):
    """elems: canonical integers (any integer is reduced mod p) -> the digest as 4 canonical integers."""
    s = [0] * W
    if len(elems) % 4 != 0:
        s[0] = 1
    i = 0
    for e in elems:
        s[4 + i] = (s[4 + i] + int(e)) % P
        i += 1
        if i == 4:
            s = permute(s)
            i = 0
    if i:
        s[4 + i] = 1
        for k in range(i + 1, 4):
            s[4 + k] = 0
        s = permute(s)
    return s[4:8]


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
    return np.array([np.frombuffer(hash_row(rows[j]), dtype=np.uint8) for j in range(rows.shape[0])])


def combined_row(ldes, epr, j) -> list:
    """Row j of every trace's LDE, the first epr elements of each (padding lanes are not hashed), canonical."""
    out = []
    for m in ldes:
        out += canonical(np.asarray(m, dtype=np.uint64)[j, :epr])
    return out


def combined_leaves(ldes, epr) -> np.ndarray:
    n = np.asarray(ldes[0]).shape[0]
    return np.array([np.frombuffer(digest_bytes(hash_elements(combined_row(ldes, epr, j))), dtype=np.uint8) for j in range(n)])


def merkle_nodes(leaves) -> np.ndarray:
    """MerkleTree::nodes for (n, 32) leaves: nodes[0] = zero digest, nodes[1] = root, nodes[i] = merge(nodes[2i], nodes[2i+1])."""
    lv = np.asarray(leaves, dtype=np.uint8).reshape(-1, 32)
    n = lv.shape[0]
    dig = [b""] * n + [bytes(x) for x in lv]
    for i in range(n - 1, 0, -1):
        dig[i] = merge(dig[2 * i], dig[2 * i + 1])
    dig[0] = bytes(32)
    return np.frombuffer(b"".join(dig[:n]), dtype=np.uint8).reshape(n, 32).copy()


def check_tree_sampled(nodes: np.ndarray, leaves: np.ndarray, indices) -> None:
    """node[i] == merge(node[2i], node[2i+1]) on the device's own children (leaves for the last level), for every sampled i."""
    n = leaves.shape[0]

    def child(k):
        return bytes(nodes[k]) if k < n else bytes(leaves[k - n])

    for i in indices:
        assert bytes(nodes[i]) == merge(child(2 * i), child(2 * i + 1)), f"node {i} of a {n}-leaf tree"


def verify_path(root: bytes, index: int, proof) -> bool:
    """MerkleTree::verify: proof = leaf, sibling leaf, siblings bottom-up."""
    r = index & 1
    v = merge(proof[r], proof[1 - r])
    index = (index + 2 ** (len(proof) - 1)) >> 1
    for p in proof[2:]:
        v = merge(v, p) if index & 1 == 0 else merge(p, v)
        index >>= 1
    return v == root


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
