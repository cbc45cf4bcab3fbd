"""Test helper: what a Sha3_256 commitment must contain, from hashlib.sha3_256 and Python integers alone (the reference's
Sha3_256::hash_elements / merge, crypto/src/hash/sha/mod.rs:17-57, and MerkleTree::new, crypto/src/merkle/mod.rs:117-136)."""
import hashlib

import numpy as np

F64, F128 = 1, 2
F64_P = 2**64 - 2**32 + 1
_R_INV = pow(2**64, -1, F64_P)  # Montgomery residue x * 2^64 mod p -> canonical x


def canonical_u64(mont: np.ndarray) -> np.ndarray:
    """f64 Montgomery residues -> canonical values (same shape), with Python integers."""
    a = np.asarray(mont, dtype=np.uint64)
    flat = [(int(v) * _R_INV) % F64_P for v in a.reshape(-1)]
    return np.array(flat, dtype=np.uint64).reshape(a.shape)


def row_bytes(field: int, row: np.ndarray) -> bytes:
    """Canonical little-endian bytes of the elements of one row, as hash_elements serialises them: f64 = canonical value,
    8 bytes; f128 = the 16 bytes as stored (lo, hi)."""
    if field == F64:
        return canonical_u64(row).tobytes()
    return np.ascontiguousarray(row, dtype=np.uint64).tobytes()


def hash_rows(field: int, rows: np.ndarray) -> np.ndarray:
    """rows: (n, row_elems[, 2]) -> (n, 32) digests."""
    rows = np.asarray(rows, dtype=np.uint64)
    canon = canonical_u64(rows) if field == F64 else rows
    return np.array([np.frombuffer(hashlib.sha3_256(canon[j].tobytes()).digest(), dtype=np.uint8) for j in range(canon.shape[0])])


def combined_leaves(field: int, ldes, epr: int) -> np.ndarray:
    """Leaf j of a commitment of several traces: SHA3-256 of row j of trace 0 || row j of trace 1 || .., each row's first
    epr elements (the padding lanes of the stored rows are not hashed).  ldes: one (n_rows, row_width[, 2]) matrix per trace."""
    mats = [np.asarray(m, dtype=np.uint64)[:, :epr] for m in ldes]
    canon = [canonical_u64(m) if field == F64 else np.ascontiguousarray(m) for m in mats]
    out = np.empty((canon[0].shape[0], 32), dtype=np.uint8)
    for j in range(out.shape[0]):
        out[j] = np.frombuffer(hashlib.sha3_256(b"".join(m[j].tobytes() for m in canon)).digest(), dtype=np.uint8)
    return out


def merge(a: bytes, b: bytes) -> bytes:
    return hashlib.sha3_256(bytes(a) + bytes(b)).digest()


def merkle_nodes(leaves: np.ndarray) -> np.ndarray:
    """MerkleTree::nodes for (n, 32) leaves: nodes[0] = zero digest, nodes[1] = root, nodes[i] = merge(nodes[2i], nodes[2i+1])."""
    lv = np.asarray(leaves, dtype=np.uint8).reshape(-1, 32)
    n = lv.shape[0]
    dig = [b""] * n + [bytes(x) for x in lv]  # heap order: node i's children at 2i, 2i + 1; leaves at n .. 2n
    for i in range(n - 1, 0, -1):
        dig[i] = hashlib.sha3_256(dig[2 * i] + dig[2 * i + 1]).digest()
    dig[0] = bytes(32)
    return np.frombuffer(b"".join(dig[:n]), dtype=np.uint8).reshape(n, 32).copy()


def verify_path(root: bytes, index: int, proof) -> bool:
    """MerkleTree::verify (crypto/src/merkle/mod.rs:295-317): proof = leaf, sibling leaf, siblings bottom-up."""
    r = index & 1
    v = merge(proof[r], proof[1 - r])
    index = (index + 2 ** (len(proof) - 1)) >> 1
    for p in proof[2:]:
        v = merge(v, p) if index & 1 == 0 else merge(p, v)
        index >>= 1
    return v == root


def verify_batch(root: bytes, positions, leaves, node_vectors, depth: int) -> bool:
    """A BatchMerkleProof (leaves at the queried positions, one vector of missing nodes per distinct leaf pair, as
    MerkleTree::prove_batch lays them out, crypto/src/merkle/mod.rs:222-284) folded back to the root."""
    n = 1 << depth
    index_map = {int(p): i for i, p in enumerate(positions)}
    if len(index_map) != len(positions):
        return False
    norm = sorted({p - (p & 1) for p in index_map})
    if len(node_vectors) != len(norm):
        return False
    used = [0] * len(norm)
    values, nxt = {}, []
    for k, index in enumerate(norm):
        pair = []
        for i in (index, index + 1):
            if i in index_map:
                pair.append(leaves[index_map[i]])
            else:
                pair.append(node_vectors[k][used[k]])
                used[k] += 1
        parent = (index + n) >> 1
        values[parent] = merge(pair[0], pair[1])
        nxt.append(parent)
    for _ in range(1, depth):
        cur, nxt = nxt, []
        i = 0
        while i < len(cur):
            node, sib = cur[i], cur[i] ^ 1
            if i + 1 < len(cur) and cur[i + 1] == sib:
                i += 1
                sib_value = values[sib]
            else:
                if used[i] >= len(node_vectors[i]):
                    return False
                sib_value = node_vectors[i][used[i]]
                used[i] += 1
            parent = node >> 1
            values[parent] = merge(values[node], sib_value) if node & 1 == 0 else merge(sib_value, values[node])
            nxt.append(parent)
            i += 1
    return nxt == [1] and values[1] == root and all(u == len(v) for u, v in zip(used, node_vectors))
