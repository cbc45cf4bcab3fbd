"""Test helper: what an Rp64_256 commitment must contain, from Python integers alone -- the reference for every Rp64_256
test (never the library, never csrc/rescue_dev.hpp).  The function restated (Rp64_256 of the reference,
crypto/src/hash/rescue/rp64_256/mod.rs; parameters from tests/golden/rp64_256_params.json):

  state: 12 elements of GF(p), p = 2^64 - 2^32 + 1; capacity 0..4, rate 4..12, digest 4..8
  permutation: 7 rounds of  x^7 | MDS | + ARK1[r] | x^inv_alpha | MDS | + ARK2[r],  MDS circulant:
               out[i] = sum_j row[(j - i) mod 12] * in[j]
  hash_elements: state[0] = number of base elements; elements added into the rate eight at a time, a permutation behind
               every full block and behind a partial last one
  merge(a, b) = hash_elements(the 8 elements of a || b), digest words read as BaseElement::new (reduced mod p)
  digest bytes = the four elements as canonical little-endian u64

A permutation costs a few milliseconds here: callers keep to at most 2048 of them per test (sample_indices)."""
import json
import os

import numpy as np

F64 = 1
P = 2**64 - 2**32 + 1
_R_INV = pow(2**64, -1, P)
_PRM = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rp64_256_params.json")))
ALPHA, INV_ALPHA, ROW, ARK1, ARK2 = _PRM["alpha"], _PRM["inv_alpha"], _PRM["mds_row"], _PRM["ark1"], _PRM["ark2"]
PERMUTATIONS = 0  # counted, so that a test can assert its budget


def _mds(s):
    return [sum(ROW[(j - i) % 12] * s[j] for j in range(12)) % P for i in range(12)]


def permute(state):
    global PERMUTATIONS
    PERMUTATIONS += 1
    s = [int(x) % P for x in state]
    for r in range(7):
        s = [pow(x, ALPHA, P) for x in s]
        s = [(x + k) % P for x, k in zip(_mds(s), ARK1[r])]
        s = [pow(x, INV_ALPHA, P) for x in s]
        s = [(x + k) % P for x, k in zip(_mds(s), ARK2[r])]
    return s


def hash_elements(elems):
    """elems: canonical integers (any integer is reduced mod p) -> the digest as 4 canonical integers."""
    s = [0] * 12
    s[0] = len(elems) % P
    i = 0
    for e in elems:
        s[4 + i] = (s[4 + i] + int(e)) % P
        i += 1
        if i == 8:
            s = permute(s)
            i = 0
    if i:
        s = permute(s)
    return s[4:8]


def digest_bytes(d) -> bytes:
    return b"".join(int(x).to_bytes(8, "little") for x in d)


def digest_words(b) -> list:
    b = bytes(b)
    return [int.from_bytes(b[8 * i:8 * i + 8], "little") for i in range(4)]


def merge(a: bytes, b: bytes) -> bytes:
    return digest_bytes(hash_elements(digest_words(a) + digest_words(b)))


def canonical(mont) -> list:
    """f64 Montgomery residues (the library's stored form, any shape) -> flat list of canonical integers."""
    return [(int(v) * _R_INV) % P for v in np.asarray(mont, dtype=np.uint64).reshape(-1)]


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


def sample_indices(n_leaves: int, spans=(), budget=2048, seed=0) -> list:
    """The fixed set of at most `budget` node indices (heap order, 1 <= i < n_leaves) a sampled tree check visits, taken in
    this order until the budget is reached:
      1. the whole top eight levels (nodes 1 .. 255);
      2. the first and last two nodes of every lower level;
      3. both sides (m - 1 and m, position within the level) of every multiple m of 256 in every level;
      4. both sides of every multiple of each of `spans` (the subtree kernel's work-group span) in every level, narrow
         levels first; where a level's multiples no longer all fit, evenly spaced ones of them (with span 64 everything
         fits up to 2^15 leaves; 2^16 leaves ask for 2307 nodes in all, so the widest levels of 2^16 and 2^17 are thinned);
      5. seeded random indices for the rest."""
    picked, seen = [], set()

    def take(i):
        if 1 <= i < n_leaves and i not in seen and len(picked) < budget:
            seen.add(i)
            picked.append(i)

    for i in range(1, min(n_leaves, 256)):
        take(i)
    widths = []
    width = 256
    while width < n_leaves:  # the level of `width` nodes is nodes[width .. 2 width)
        widths.append(width)
        width *= 2
    for width in widths:
        for k in (0, 1, width - 2, width - 1):
            take(width + k)
    for width in widths:
        for m in range(256, width, 256):
            take(width + m - 1)
            take(width + m)
    for span in spans:
        for width in widths:
            todo = [m for m in range(span, width, span) if width + m not in seen or width + m - 1 not in seen]
            room = (budget - len(picked)) // 2
            if len(todo) > room:
                todo = [todo[(k * len(todo)) // room] for k in range(room)] if room else []
            for m in todo:
                take(width + m - 1)
                take(width + m)
    rng = np.random.default_rng(seed)
    while len(picked) < min(budget, n_leaves - 1):
        take(int(rng.integers(1, n_leaves)))
    return picked


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
