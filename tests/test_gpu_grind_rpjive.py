"""GPU: wf_grind_seeds (ProverChannel::grind_query_seed) under RpJive64_256 against a CPU search on tests/rpjive_util.py
(Python integers; never the library).  The answer is the SMALLEST qualifying nonce of the range, so every comparison is
exact: nonce, new seed and the found byte.

Seeds are SHA-256 of the ASCII text "grind seed <k>", picked on the CPU so that every search stays inside 2048 reference
permutations (one per nonce tried); `expect` FAILS the test when a search goes beyond that, and the comments give each
seed's answers.  From nonce 1, smallest nonce for g = 4 / g = 8:
  k0: 11 / 61    k2: 4 / 538    k7: 13 / 160    k10: 21 / 146    k13: 6 / 14    k22: 24 / 24    k25: 71 / none below 700
EDGE_SEED (words p, 2^64 - 1, p + 1 and an ordinary one): 3 / 307 from nonce 1; 2^64 - 289 / 2^64 - 205 from 2^64 - 301."""
import hashlib

import numpy as np
import pytest

import rpjive_util as R

pytestmark = pytest.mark.gpu

P = R.P
BUDGET = 2048
EDGE_SEED = b"".join(w.to_bytes(8, "little") for w in (P, 2**64 - 1, P + 1, 0x0123456789ABCDEF))
EDGE_VALUES = [0, 1, 2**32, P - 1, P, P + 2, 2**64 - 1]
NOT_FOUND = (0, bytes(32), 0)


def K(k):
    return hashlib.sha256(b"grind seed %d" % k).digest()


@pytest.fixture(autouse=True)
def _permutation_budget():
    before = R.PERMUTATIONS
    yield
    assert R.PERMUTATIONS - before <= BUDGET, "the Python reference ran more permutations than a test may need"


@pytest.fixture(scope="module")
def jctx(capi):
    c = capi.Context(0)
    c.set_hasher(capi.RPJIVE64_256)
    yield c
    c.close()


def tuned_context(capi, monkeypatch, first_log2=4, cap_log2=6):
    monkeypatch.setenv("WF_EXP_ENABLE", "1")  # the library reads its WF_EXP_* switches only under this one
    monkeypatch.setenv("WF_EXP_GRIND_WINDOW_LOG2", str(first_log2))
    monkeypatch.setenv("WF_EXP_GRIND_WINDOW_CAP_LOG2", str(cap_log2))
    c = capi.Context(0)
    c.set_hasher(capi.RPJIVE64_256)
    return c


def grind_one(c, seed, g, begin=1, max_nonces=2**64 - 1):
    nonces, new_seeds, found = c.grind(np.frombuffer(seed, dtype=np.uint8), g, begin, max_nonces)
    return int(nonces[0]), bytes(new_seeds[0]), int(found[0])


def expect(seed, g, begin=1, max_nonces=2**64 - 1, must_find=True):
    """The smallest qualifying nonce of [begin, begin + max_nonces) clipped at 2^64 - 1, with its digest.  A search that is
    meant to find something and has not after BUDGET tries fails the test: the reference never gives up silently."""
    end = min(begin + max_nonces, 2**64)
    assert must_find or end - begin <= BUDGET
    for tries, v in enumerate(range(begin, end)):
        if tries >= BUDGET:
            pytest.fail(f"CPU search g={g} from {begin} went beyond its budget of {BUDGET} tries: pick another seed")
        d = R.merge_with_int(seed, v)
        if R.trailing_zeros_ok(d, g):
            return v, d, 1
    assert not must_find, "the range holds no qualifying nonce"
    return NOT_FOUND


def test_merge_with_int_and_factor_zero(jctx):
    """g = 0 accepts every nonce and max_nonces = 1 leaves one: the call returns merge_with_int(seed, v).  Both branches
    (v < p: place 7 = 5; v >= p: v / p in place 5 and place 7 = 6), a seed with words >= p, and v = 2^64 - 1, which is also
    the value best[] holds while nothing has been found."""
    for seed in (EDGE_SEED, K(0)):
        for v in EDGE_VALUES:
            assert grind_one(jctx, seed, 0, v, 1) == (v, R.merge_with_int(seed, v), 1), v
        assert grind_one(jctx, seed, 0) == (1, R.merge_with_int(seed, 1), 1)   # factor 0 from nonce 1: the first nonce


@pytest.mark.parametrize("g", [4, 8])
def test_search_below_p(jctx, g):
    for k in (0, 13, 7):
        seed = K(k)
        want = expect(seed, g)
        assert want[2] == 1
        for _ in range(2):   # many waves find qualifying nonces in no particular order: the smallest one, call after call
            assert grind_one(jctx, seed, g) == want, k


@pytest.mark.parametrize("g", [4, 8])
def test_search_above_p(jctx, g):
    """nonce_begin = 2^64 - 1 - 300: every nonce of the range is >= p (the two-element branch), and the range ends at
    2^64 - 1 whatever max_nonces says."""
    begin = 2**64 - 1 - 300
    want = expect(EDGE_SEED, g, begin)
    assert want[2] == 1 and begin <= want[0] < 2**64 and want[0] >= P
    assert grind_one(jctx, EDGE_SEED, g, begin) == want
    assert grind_one(jctx, EDGE_SEED, g, begin, 301) == want


def test_search_across_p(jctx):
    """A range that starts below p and ends above it: the answers on either side."""
    begin = P - 20
    seed = K(0)
    want = expect(seed, 4, begin)
    assert grind_one(jctx, seed, 4, begin) == want
    want = expect(seed, 4, P)       # from p itself: the first nonce of the other branch
    assert want[0] >= P
    assert grind_one(jctx, seed, 4, P) == want


@pytest.mark.parametrize("g", [4, 8])
def test_seed_with_words_above_p(jctx, g):
    want = expect(EDGE_SEED, g)
    assert grind_one(jctx, EDGE_SEED, g) == want
    # the same seed reduced mod p is the same seed
    reduced = b"".join((w % P).to_bytes(8, "little") for w in R.digest_words(EDGE_SEED))
    assert reduced != EDGE_SEED and grind_one(jctx, reduced, g) == want


def test_nothing_found_inside_max_nonces(jctx):
    seed = K(25)
    want = expect(seed, 8, 1, 300, must_find=False)
    assert want == NOT_FOUND
    assert grind_one(jctx, seed, 8, 1, 300) == NOT_FOUND
    a, d, _ = expect(K(7), 8)                       # one nonce short of the answer, and just enough
    assert grind_one(jctx, K(7), 8, 1, a - 1) == NOT_FOUND
    assert grind_one(jctx, K(7), 8, 1, a) == (a, d, 1)
    # a factor nothing in the last 40 nonces reaches: not found, the call still ends
    begin = 2**64 - 40
    assert expect(seed, 32, begin, 2**64 - 1, must_find=False) == NOT_FOUND
    assert grind_one(jctx, seed, 32, begin, 2**64 - 1) == NOT_FOUND


def test_batch(capi, monkeypatch):
    """Five seeds in one call on a context with windows [1,16] [17,48] [49,112] [113,176] ..: the answers lie in different
    windows (the first seed finishes in the first one and sits out the later launches), the last seed has none in the range.
    Every output equals the single-seed call's; nothing is written behind n_seeds entries."""
    ks, rng = (13, 22, 0, 10, 2), 400
    seeds = [K(k) for k in ks]
    want = [expect(s, 8, 1, rng, must_find=False) for s in seeds]
    assert [w[2] for w in want] == [1, 1, 1, 1, 0]
    windows = [0 if w[0] <= 16 else 1 if w[0] <= 48 else 2 if w[0] <= 112 else 3 + (w[0] - 113) // 64 for w in want[:4]]
    assert windows == [0, 1, 2, 3]
    c = tuned_context(capi, monkeypatch)
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
