"""GPU: wf_grind_seeds under GriffinJive64_256 against the search of the plain C reference (tests/cpp/griffin_ref.c through
tests/griffin_util.py): the smallest qualifying nonce, its digest, the found flag -- at grinding factors 0, 8 and 16, across
p (both branches of merge_with_int), batched, with max_nonces exact and one short, with answers in the first three windows
of the product's own plan, and on directed seeds.  No reference search may try more than 2^18 nonces: it fails the test
beyond that, and the count is asserted."""
import hashlib
import os

import numpy as np
import pytest

import griffin_edge_util as D
import griffin_util as G

pytestmark = pytest.mark.gpu
P = G.P
C_BUDGET = 1 << 18
W0 = 1 << 16   # the first window of GRIND_PLAN_GRIFFIN (csrc/grind_plan.hpp: first_log2 = 16); then 2 W0, 4 W0
NOT_FOUND = (0, bytes(32), 0)
GRIND_G = 16
# (k, answer): the seed is SHA-256 of "griffin grind seed <k>"; its smallest factor-16 nonce from 1, late in the first window
# [1, W0], in the second [W0 + 1, 3 W0] and in the third [3 W0 + 1, 7 W0] (within the reference's budget: below 4 W0)
GRIND_SEEDS = ((11, 55295), (0, 139683), (20, 229061))


def K(k):
    return hashlib.sha256(b"griffin grind seed %d" % k).digest()


@pytest.fixture(scope="module")
def cref():
    return G.CRef()


@pytest.fixture(scope="module")
def gctx(capi):
    assert not any(k.startswith("WF_EXP_GRIND") for k in os.environ), "this file runs the product's own window plan"
    c = capi.Context(0)
    c.set_hasher(capi.GRIFFINJIVE64_256)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _budget(cref):
    cref.spent = 0
    yield
    assert cref.spent <= C_BUDGET, f"{cref.spent} C-reference permutations in one test"


def expect(cref, seed, g, begin=1, max_nonces=2**64 - 1, budget=C_BUDGET):
    """The reference search: the smallest qualifying nonce of the range with its digest.  It tries at most `budget` nonces and
    FAILS the test when a longer range has nothing within them: it never gives up silently."""
    span = min(max_nonces, 2**64 - begin)
    n, d = cref.grind(seed, g, begin, min(span, budget))
    if n is None:
        if span > budget:
            pytest.fail(f"CPU search g={g} from {begin} went beyond its budget of {budget} tries: pick another seed")
        return NOT_FOUND
    return n, d, 1


def grind_one(c, seed, g, begin=1, max_nonces=2**64 - 1):
    nonces, new_seeds, found = c.grind(np.frombuffer(seed, dtype=np.uint8), g, begin, max_nonces)
    return int(nonces[0]), bytes(new_seeds[0]), int(found[0])


@pytest.mark.parametrize("g", [0, 8])
def test_grind_small_factors(gctx, cref, g):
    for k in range(6):
        want = expect(cref, K(k), g, budget=1 << 13)
        assert want[2] == 1 and G.trailing_zeros_ok(want[1], g)
        assert grind_one(gctx, K(k), g) == want
        assert want[1] == G.merge_with_int(K(k), want[0])   # the Python integers agree on the digest


def test_grind_range_crossing_p(gctx, cref):
    """nonce_begin = p - 3: nonces p - 3, p - 2, p - 1 take the narrow branch of merge_with_int, p, p + 1, .. the wide one.  At
    factor 0 the first nonce is the answer; at factor 2 some of the first ones fail, whichever side they are on."""
    seed = K(7)
    for begin in range(P - 3, P + 2):
        want = (begin, cref.merge_with_int(seed, begin), 1)
        assert want[1] == G.merge_with_int(seed, begin)
        assert grind_one(gctx, seed, 0, begin, 1) == want
    for k in range(8):
        want = expect(cref, K(k), 2, P - 3, 64)
        assert grind_one(gctx, K(k), 2, P - 3, 64) == want
    wide = [expect(cref, K(k), 3, P, 64) for k in range(4)]
    assert all(w[2] == 1 and w[0] >= P for w in wide)
    assert [grind_one(gctx, K(k), 3, P, 64) for k in range(4)] == wide


@pytest.mark.parametrize("window", [0, 1, 2])
def test_grind_in_each_production_window(gctx, cref, window):
    k, answer = GRIND_SEEDS[window]
    want = expect(cref, K(k), GRIND_G)
    assert want[0] == answer and want[2] == 1
    assert (3 * W0 // 4, W0 + 1, 3 * W0 + 1)[window] <= answer <= (W0, 3 * W0, 7 * W0)[window]
    got = grind_one(gctx, K(k), GRIND_G)
    assert got == want
    assert int.from_bytes(got[1][:8], "little") % (1 << GRIND_G) == 0


def test_grind_max_nonces_exact_and_one_short(gctx, cref):
    """max_nonces one short of the second-window answer: not found; exactly at it: found."""
    k, answer = GRIND_SEEDS[1]
    want = expect(cref, K(k), GRIND_G, 1, answer)
    assert want[0] == answer
    assert grind_one(gctx, K(k), GRIND_G, 1, answer - 1) == NOT_FOUND
    assert grind_one(gctx, K(k), GRIND_G, 1, answer) == want


def test_grind_three_seeds_batched(capi, gctx, cref):
    """Three seeds in one call at factor 12 (the three factor-16 answers together would cost the reference more than a test
    may spend): each leaves the search at its own nonce; nothing is written behind n_seeds entries."""
    ks = [GRIND_SEEDS[0][0], GRIND_SEEDS[1][0], 3]
    g = 12
    seeds = [K(k) for k in ks]
    want = [expect(cref, s, g, budget=1 << 16) for s in seeds]
    assert all(w[2] == 1 for w in want) and len({w[0] for w in want}) == 3
    n, tail = len(seeds), 3
    nonces = np.full(n + tail, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    new_seeds = np.full((n + tail, 32), 0xA5, dtype=np.uint8)
    found = np.full(n + tail, 0xA5, dtype=np.uint8)
    flat = np.frombuffer(b"".join(seeds), dtype=np.uint8)
    rc = capi.load().wf_grind_seeds(gctx._h, flat.ctypes.data, n, g, 1, 2**64 - 1, nonces.ctypes.data,
                                    new_seeds.ctypes.data, found.ctypes.data)
    assert rc == 0, capi.load().wf_last_error()
    for i in range(n):
        assert (int(nonces[i]), bytes(new_seeds[i]), int(found[i])) == want[i], i
    assert (nonces[n:] == 0xA5A5A5A5A5A5A5A5).all() and (new_seeds[n:] == 0xA5).all() and (found[n:] == 0xA5).all()


def test_grind_on_directed_seeds(gctx, cref):
    """Factor 0 and max_nonces = 1 return merge_with_int(seed, nonce): directed seed words with a directed nonce, so that the
    first non-linear layer of k_grind / k_grind_finish meets every (i, case) of gfj::linear its caller can reach: i = 2..5."""
    ins = D.seed_states()
    assert sorted(ins) == sorted(D.reachable("merge_with_int")) and {i for i, _ in ins} == {2, 3, 4, 5}
    for rc in D.reachable("merge_with_int"):
        *words, nonce = ins[rc]
        assert len(words) == 4 and nonce < P
        seed = G.digest_bytes_raw(words)
        want = cref.merge_with_int(seed, nonce)
        assert want == G.merge_with_int(seed, nonce)
        assert grind_one(gctx, seed, 0, nonce, 1) == (nonce, want, 1), rc
