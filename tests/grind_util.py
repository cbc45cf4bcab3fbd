"""Test helper: ProverChannel::grind_query_seed restated on the CPU, for every hasher, from sources that are never the
library: BLAKE3 through the oracle's merge_with_int (under digest_size(24) for Blake3_192), Sha3_256 through hashlib,
Rp64_256 through rp64_util (Python integers).  A seed is a 32-byte slot (a 24-byte digest in front, zeros behind), and so
is every digest returned here.

  merge_with_int(orc, hasher, seed, v)   the coin's seed after reseed_with_int(v)
  head(slot)                             the first 8 digest bytes as a little-endian integer; a nonce qualifies for
                                         grinding factor g when head & (2^g - 1) == 0 (check_leading_zeros)
  search(orc, hasher, seed, g, begin, max_nonces)
                                         the smallest qualifying nonce of [begin, begin + max_nonces), the range ending at
                                         2^64 - 1 at the latest -> (nonce, new seed), or (None, None)

The search has a try budget per call -- 2^19 hashes for the byte hashers, 2048 permutations for Rp64_256 (rp64_util's
convention) -- and FAILS the test when it is exceeded: seeds are chosen so that it never is.  Results are kept, so tests
that ask the same question share one search."""
import hashlib

import pytest

import rp64_util as R

P = R.P
HASHERS = ["blake3_256", "blake3_192", "sha3_256", "rp64_256"]
BUDGET = {"blake3_256": 1 << 19, "blake3_192": 1 << 19, "sha3_256": 1 << 19, "rp64_256": 2048}
EDGE_VALUES = [0, 1, 2**32 - 1, 2**32, 2**32 + 1, P - 1, P, P + 1, 2**64 - 1]


def configure(ctx, capi, hasher):
    """Sets the context's hasher pair for one of HASHERS."""
    ctx.set_hasher(capi.BLAKE3)
    ctx.set_digest_bytes(24 if hasher == "blake3_192" else 32)
    if hasher == "sha3_256":
        ctx.set_hasher(capi.SHA3_256)
    elif hasher == "rp64_256":
        ctx.set_hasher(capi.RP64_256)


def merge_with_int(orc, hasher, seed: bytes, v: int) -> bytes:
    seed = bytes(seed)
    assert len(seed) == 32 and 0 <= v < 2**64
    if hasher == "blake3_256":
        return orc.merge_with_int(seed, v)
    if hasher == "blake3_192":
        with orc.digest_size(24):
            return orc.merge_with_int(seed[:24], v) + bytes(8)
    if hasher == "sha3_256":
        return hashlib.sha3_256(seed + v.to_bytes(8, "little")).digest()
    assert hasher == "rp64_256"
    words = [w % P for w in R.digest_words(seed)]
    return R.digest_bytes(R.hash_elements(words + [v % P] + ([v // P] if v >= P else [])))


def head(slot: bytes) -> int:
    return int.from_bytes(bytes(slot)[:8], "little")


def qualifies(slot: bytes, g: int) -> bool:
    return head(slot) & ((1 << g) - 1) == 0


def slot(hasher, seed_hex: str) -> bytes:
    """A seed literal as the hasher's 32-byte slot (Blake3_192: the first 24 bytes, zeros behind)."""
    s = bytes.fromhex(seed_hex)
    assert len(s) == 32
    return s[:24] + bytes(8) if hasher == "blake3_192" else s


# (hasher, seed, g, begin) -> [next nonce to try, the first qualifying nonce from `begin` or None, its digest]: a search
# with a shorter range is answered from a longer one, a longer one goes on where the shorter one stopped
_SEARCHES = {}


def search(orc, hasher, seed: bytes, g: int, begin: int = 1, max_nonces: int = 2**64 - 1):
    end = min(begin + max_nonces, 2**64)  # one past the last nonce
    st = _SEARCHES.setdefault((hasher, bytes(seed), g, begin), [begin, None, None])
    while st[1] is None and st[0] < end:
        if st[0] - begin >= BUDGET[hasher]:
            pytest.fail(f"CPU search for {hasher} g={g} from {begin} went beyond its budget of {BUDGET[hasher]} tries: "
                        f"pick another seed")
        d = merge_with_int(orc, hasher, seed, st[0])
        if qualifies(d, g):
            st[1], st[2] = st[0], d
        st[0] += 1
    return (st[1], st[2]) if st[1] is not None and st[1] < end else (None, None)
