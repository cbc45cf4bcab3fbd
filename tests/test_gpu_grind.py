"""GPU: wf_grind_seeds (ProverChannel::grind_query_seed, prover/src/channel.rs:182-198) for every hasher against the CPU
search of tests/grind_util.py, whose digests come from the oracle (BLAKE3), hashlib (Sha3_256) and rp64_util (Rp64_256) --
never from the library.  The answer is the SMALLEST qualifying nonce of the range (the serial reference's find), so every
comparison is exact: nonce, new seed and the found byte.

Seeds are fixed literals (SHA-256 of the ASCII text "grind seed <k>"), picked on the CPU so that every search stays inside
the helper's try budget; the comments give each seed's answers from nonce 1.  Windows of the tuned contexts (first 2^4,
cap 2^6, from nonce 1): [1,16] [17,48] [49,112], then 64 nonces each: [113,176] [177,240] [241,304] [305,368] [369,432]."""

import numpy as np
import pytest

import grind_util as G

pytestmark = pytest.mark.gpu

P = G.P
K = {  # k -> SHA-256("grind seed k")
    0: "405552217d62f4901368693998dc7bcb6fc5892652f76f76fb2c8594b70c48b4",
    1: "b2461b3950f9038d973ccbabc376fe7ffbaa5de8004302a5cfa387b08d016239",
    2: "aade78a85297f3d5164939609175e00a25d268ee065dfde6f9eabcbf25197884",
    3: "48e0dd46ed564b0c667bc758f1ab1d047c5b46d7152c915c2b53f2ba3fad8124",
    4: "d2af2ce567df6ab3e3da7578c061cf987dcdb41273b8789f028d7b8ee3fa3cd8",
    5: "a8a378814588e979fbc8758e36688e1be1950a58d5c9381bd081b21323076152",
    7: "24c1722cd93d9bf5149ecdf10f78afd1db4ebd674d507852038a03b41296503f",
    8: "744bc887ea30fb46c59faf0cfd04b182f1cc19012ee18b08e32d31a381fe915e",
    9: "9d1dbab05f0fc836705c26f983097d5f9be50f78c8cc946a558992236ce07604",
    10: "612f897cbd931f01b9153e6a6c3d618d49f98794b96b659c5fa77bbb447f1167",
    13: "6c1d81378ea1fd976142978370ad13f0e0c307b625790343467b3bebf4b94bf3",
    14: "9a0527ed8f3fe2d01b17612b4b7a59f38a27867a8f6eceb309f45d0cc18309c9",
    17: "dde7ad0deebe66f309346ba28f95117a30a6efa0b5530c040658ea5de1a56929",
    21: "8ebdd3669b31e37493532edaa30d209ec357d7b496064c7177a9ab48b8286212",
    22: "9623ac117fcae1e9e809af860f05f20c5b7f2a5bfbbf1a6cd6c5b47e0dc45019",
}
# A seed whose 64-bit words are p, 2^64 - 1, p + 1 and an ordinary one: Rp64_256 reads them reduced mod p.
EDGE_SEED = b"".join(w.to_bytes(8, "little") for w in (P, 2**64 - 1, P + 1, 0x0123456789ABCDEF)).hex()

# Per hasher: grinding factors of the "real factors" case and its three seeds (answers from nonce 1 per factor, in order);
# the seed of the window and range-end cases (its g = 8 answer `a`); the five seeds of the batch with its range length (the
# first four answers lie in different windows of the tuned context, the last seed's lies beyond the range).
CASES = {
    "blake3_256": dict(factors=(8, 12, 16), real=(0, 1, 22),    # k0: 345, 9756, 13351; k1: 246, 3040, 19752; k22: 688, 1665, 83954
                       edge=0,                                  # a = 345
                       batch=(4, 8, 3, 1, 7), batch_range=400),  # g = 8: 7, 35, 104, 246; k7: 475
    "blake3_192": dict(factors=(8, 12, 16), real=(0, 7, 2),     # k0: 251, 2316, 27622; k7: 111, 356, 2155; k2: 503, 11243, 81829
                       edge=0,                                  # a = 251
                       batch=(17, 21, 9, 4, 2), batch_range=400),  # g = 8: 5, 20, 67, 165; k2: 503
    "sha3_256": dict(factors=(8, 12, 16), real=(0, 1, 14),      # k0: 420, 1720, 15948; k1: 235, 5246, 29367; k14: 443, 3917, 96034
                     edge=0,                                    # a = 420
                     batch=(4, 7, 13, 1, 5), batch_range=400),  # g = 8: 26, 51, 146, 235; k5: 547
    "rp64_256": dict(factors=(4, 8), real=(2, 4, 1),            # k2: 4, 4; k4: 12, 35; k1: 7, 202
                     edge=1,                                    # a = 202
                     batch=(2, 4, 3, 10, 1), batch_range=150),  # g = 8: 4, 35, 66, 141; k1: 202
}


@pytest.fixture(scope="module", params=G.HASHERS)
def hctx(request, capi):
    """(hasher, a context of its own set to that hasher): the session's shared context keeps its hasher."""
    c = capi.Context(0)
    G.configure(c, capi, request.param)
    yield request.param, c
    c.close()


def tuned_context(capi, monkeypatch, hasher, first_log2=4, cap_log2=6):
    monkeypatch.setenv("WF_EXP_ENABLE", "1")  # the library reads its WF_EXP_* switches only under this one
    monkeypatch.setenv("WF_EXP_GRIND_WINDOW_LOG2", str(first_log2))
    monkeypatch.setenv("WF_EXP_GRIND_WINDOW_CAP_LOG2", str(cap_log2))
    c = capi.Context(0)
    G.configure(c, capi, hasher)
    return c


def grind_one(c, seed, g, begin=1, max_nonces=2**64 - 1):
    nonces, new_seeds, found = c.grind(np.frombuffer(seed, dtype=np.uint8), g, begin, max_nonces)
    return int(nonces[0]), bytes(new_seeds[0]), int(found[0])


def expect(orc, hasher, seed, g, begin=1, max_nonces=2**64 - 1):
    n, d = G.search(orc, hasher, seed, g, begin, max_nonces)
    return (0, bytes(32), 0) if n is None else (n, d, 1)


def test_merge_with_int(hctx, orc):
    """g = 0 accepts every nonce and max_nonces = 1 leaves one: the call returns merge_with_int(seed, v).  Both nonce words,
    both branches of Rp64_256 (v < p, v >= p), a seed with words >= p, and v = 2^64 - 1, which is also the value best[] holds
    while nothing has been found."""
    hasher, c = hctx
    for seed_hex in (EDGE_SEED, K[0]):
        seed = G.slot(hasher, seed_hex)
        for v in G.EDGE_VALUES:
            assert grind_one(c, seed, 0, v, 1) == (v, G.merge_with_int(orc, hasher, seed, v), 1), (seed_hex, v)


@pytest.mark.parametrize("g", [1, 4])
def test_smallest_not_first(hctx, orc, g):
    """The first window holds thousands of qualifying nonces, found by many waves in no particular order: the answer is the
    smallest one, call after call."""
    hasher, c = hctx
    seed = G.slot(hasher, K[0])
    want = expect(orc, hasher, seed, g)
    assert want[2] == 1 and want[0] < 200
    for _ in range(3):
        assert grind_one(c, seed, g) == want


def test_real_factors(hctx, orc):
    hasher, c = hctx
    for g in CASES[hasher]["factors"]:
        for k in CASES[hasher]["real"]:
            seed = G.slot(hasher, K[k])
            want = expect(orc, hasher, seed, g)
            got = grind_one(c, seed, g)
            assert got == want, (g, k)
            assert got[2] == 1 and G.head(got[1]) % (1 << g) == 0


def test_window_edges(hctx, orc, capi, monkeypatch):
    """First window 2^4, cap 2^6: the answer `a` of a g = 8 search as the first nonce of a window, as its last, one behind it
    and one window further; and from nonce 1 through the three doubling windows and the capped ones."""
    hasher, _ = hctx
    seed = G.slot(hasher, K[CASES[hasher]["edge"]])
    a, d, _ = expect(orc, hasher, seed, 8)
    assert a > 176, "the search from 1 must run through more than one capped window"
    c = tuned_context(capi, monkeypatch, hasher)
    try:
        for begin in (a, a - 15, a - 16, a - 17, 1):
            # (a is the smallest qualifying nonce from 1: no begin in 1..a has a qualifying nonce in front of a)
            begin = max(begin, 1)
            assert expect(orc, hasher, seed, 8, begin) == (a, d, 1)
            assert grind_one(c, seed, 8, begin) == (a, d, 1), begin
    finally:
        c.close()


def test_range_end(hctx, orc):
    hasher, c = hctx
    seed = G.slot(hasher, K[CASES[hasher]["edge"]])
    a, d, _ = expect(orc, hasher, seed, 8)
    assert expect(orc, hasher, seed, 8, 1, a - 1) == (0, bytes(32), 0)
    assert grind_one(c, seed, 8, 1, a - 1) == (0, bytes(32), 0)
    assert grind_one(c, seed, 8, 1, a) == (a, d, 1)
    # the range ends at 2^64 - 1, whatever max_nonces says: 40 nonces, nothing wraps round to the small ones
    begin = 2**64 - 40
    want = expect(orc, hasher, seed, 3, begin, 2**64 - 1)
    assert want[2] == 0 or begin <= want[0] < 2**64
    assert grind_one(c, seed, 3, begin, 2**64 - 1) == want
    # and a factor nothing in those 40 nonces reaches: not found, the call still ends
    want = expect(orc, hasher, seed, 32, begin, 2**64 - 1)
    assert want == (0, bytes(32), 0)
    assert grind_one(c, seed, 32, begin, 2**64 - 1) == want


def test_batch(hctx, orc, capi, monkeypatch):
    """Five seeds in one call on the tuned context: the answers lie in different windows (seeds that are done sit out the later
    launches), the last seed has none in the range.  Every output equals the single-seed call's; nothing is written behind
    n_seeds entries."""
    hasher, _ = hctx
    ks, rng = CASES[hasher]["batch"], CASES[hasher]["batch_range"]
    seeds = [G.slot(hasher, K[k]) for k in ks]
    want = [expect(orc, hasher, s, 8, 1, rng) for s in seeds]
    assert [w[2] for w in want] == [1, 1, 1, 1, 0]
    windows = [0 if w[0] <= 16 else 1 if w[0] <= 48 else 2 if w[0] <= 112 else 3 + (w[0] - 113) // 64 for w in want[:4]]
    assert len(set(windows)) == 4, windows
    c = tuned_context(capi, monkeypatch, hasher)
    try:
        n, tail = len(seeds), 3
        nonces = np.full(n + tail, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        new_seeds = np.full((n + tail, 32), 0xA5, dtype=np.uint8)
        found = np.full(n + tail, 0xA5, dtype=np.uint8)
        flat = np.frombuffer(b"".join(seeds), dtype=np.uint8)
        rc = capi.load().wf_grind_seeds(c._h, flat.ctypes.data, n, 8, 1, rng, nonces.ctypes.data, new_seeds.ctypes.data,
                                        found.ctypes.data)
        assert rc == 0, capi.load().wf_last_error()
        for i in range(n):
            got = (int(nonces[i]), bytes(new_seeds[i]), int(found[i]))
            assert got == want[i], i
            assert got == grind_one(c, seeds[i], 8, 1, rng), i
        assert (nonces[n:] == 0xA5A5A5A5A5A5A5A5).all() and (new_seeds[n:] == 0xA5).all() and (found[n:] == 0xA5).all()
    finally:
        c.close()


def test_refusals_and_stream_order(hctx, orc, capi):
    hasher, c = hctx
    lib = capi.load()
    seed = G.slot(hasher, K[0])
    want = expect(orc, hasher, seed, 4)
    buf = np.frombuffer(seed * 257, dtype=np.uint8)
    nonces, new_seeds, found = np.zeros(257, dtype=np.uint64), np.zeros((257, 32), dtype=np.uint8), np.zeros(257, dtype=np.uint8)

    def call(seeds=buf.ctypes.data, n=1, g=4, begin=1, max_nonces=1000, out=nonces.ctypes.data):
        return lib.wf_grind_seeds(c._h, seeds, n, g, begin, max_nonces, out, new_seeds.ctypes.data, found.ctypes.data)

    for bad in (dict(g=33), dict(n=0), dict(n=257), dict(max_nonces=0), dict(out=None), dict(seeds=None)):
        assert call(**bad) == -19, bad  # WF_ERR_ARG
        assert grind_one(c, seed, 4) == want  # the context works afterwards
    assert lib.wf_grind_seeds(None, buf.ctypes.data, 1, 4, 1, 1000, nonces.ctypes.data, new_seeds.ctypes.data, found.ctypes.data) == -19
    assert call(n=256) == 0 and (nonces[:256] == want[0]).all() and found[:256].all()

    # the call is queued behind a commitment on the same context, and a commitment behind it
    rng = np.random.default_rng(5)
    cols = [rng.integers(0, P, size=1 << 10, dtype=np.uint64) for _ in range(8)]
    params = capi.make_params(capi.F64, 1, 10, 3, 8, 1, digest_bytes=c.digest_bytes, hasher=c.hasher)
    first = c.trace_commit(params, cols, want_lde=False, want_polys=False)["root"]
    assert grind_one(c, seed, 4) == want
    again = c.trace_commit(params, cols, want_lde=False, want_polys=False)["root"]
    assert again == first
    assert grind_one(c, seed, 4) == want
