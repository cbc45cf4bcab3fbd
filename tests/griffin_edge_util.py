"""Test helper: directed operands for gfj::linear of csrc/griffin_dev.hpp, the one carry chain GriffinJive64_256 adds, on Python
integers alone.

linear(i, z0, z1, t) forms S = (i - 1) r0 + r1 + r2 on the operands' Montgomery residues (each below p), splits it into its
high word h = S >> 64 and its low 64 bits, folds with 2^64 = 2^32 - 1 (mod p) into lo + h (2^32 - 1), and corrects once.  The
cases, by S:

  below_p     S < p - 1: nothing to correct
  p-1, p      S exactly p - 1 (the largest value left alone) / exactly p (the smallest one corrected, to 0)
  above_p     p < S < 2^64: the sum fits 64 bits but is not canonical
  2^64        S exactly 2^64: high word 1 over a zero low word
  hi<h>       high word h, and lo + h (2^32 - 1) stays below 2^64      (h = 1 .. i: S <= (i + 1)(p - 1) < (i + 1) 2^64)
  hi<h>c      high word h, and lo + h (2^32 - 1) carries out of 64 bits (h = 1 .. i - 1: under the top high word the low
              word cannot get that large)
  all_p-1     r0 = r1 = r2 = p - 1, the largest S

operands(i, case, draw) returns residues (r0, r1, r2) for the function alone, where t is free.  Inside the permutation t is
0 for i = 2 and the new s_{i-1} behind it; state(i, case, free, draw) solves the first non-linear layer forward -- choose
the new s0, s1, s2' .. s7', then s_i = s_i' / q(l_i) -- and returns the canonical state IN FRONT of the layer whose first
non-linear layer meets (i, case), given which places the entry point controls:

  merge            every place                         -> every i, every case but those that need t != 0 at i = 2
  row of >= 4      places 0..3 (4..7 are 0 / 1, 0, 0, 0) -> i = 2, 3, 4 (l_4 reads the new s3; l_5 reads the new s4, not free)
  merge_with_int   places 0..4 (nonce < p)              -> i = 2 .. 5"""
import random

import griffin_util as G

P = G.P
R = 2**64 % P
R_INV = pow(R, P - 2, P)
INV7 = G.INV_ALPHA
BASE_CASES = ["below_p", "p-1", "p", "above_p", "2^64"]
ENTRIES = {"merge": list(range(8)), "row": [0, 1, 2, 3], "merge_with_int": [0, 1, 2, 3, 4]}


def cases(i, t_free=True):
    """The cases linear() can meet for state element i; with t forced to 0 (i = 2 inside the permutation) S <= 2 (p - 1)."""
    top = i if t_free else i - 1          # the largest high word: (copies of p - 1) - 1
    out = list(BASE_CASES) + ["hi%d" % h for h in range(1, top + 1)] + ["hi%dc" % h for h in range(1, top)]
    return out + (["all_p-1"] if t_free else [])


def classify(i, r0, r1, r2):
    s = (i - 1) * r0 + r1 + r2
    if r0 == r1 == r2 == P - 1:
        return "all_p-1"
    if s < P - 1:
        return "below_p"
    if s < 2**64:
        return {P - 1: "p-1", P: "p"}.get(s, "above_p")
    if s == 2**64:
        return "2^64"
    h, lo = s >> 64, s & (2**64 - 1)
    return "hi%d%s" % (h, "c" if lo + h * (2**32 - 1) >= 2**64 else "")


def needs_correction(i, r0, r1, r2):
    """Whether a copy of linear() without its last correction gives another word than linear() here."""
    s = (i - 1) * r0 + r1 + r2
    h, lo = s >> 64, s & (2**64 - 1)
    return lo + h * (2**32 - 1) >= P


def _target(i, case, rng):
    k = i - 1
    if case == "all_p-1":
        return (k + 2) * (P - 1)
    if case == "below_p":
        return rng.randrange(0, P - 1)
    if case == "p-1":
        return P - 1
    if case == "p":
        return P
    if case == "above_p":
        return rng.randrange(P + 1, 2**64)
    if case == "2^64":
        return 2**64
    carry = case.endswith("c")
    h = int(case[2:].rstrip("c"))
    z = h * (2**32 - 1)
    lo = rng.randrange(2**64 - z, 2**64) if carry else rng.randrange(1, 2**64 - z)
    return (h << 64) + lo


def operands(i, case, draw=0, t_free=True):
    """Residues (r0, r1, r2), each below p, with (i - 1) r0 + r1 + r2 in `case`; r2 = 0 unless t_free."""
    k = i - 1
    rng = random.Random("linear %d %d %s" % (i, draw, case))
    s = _target(i, case, rng)
    rest_max = (2 if t_free else 1) * (P - 1)
    assert s <= k * (P - 1) + rest_max, (i, case)
    lo0, hi0 = max(0, -(-(s - rest_max) // k)), min(P - 1, s // k)
    r0 = rng.randrange(lo0, hi0 + 1)
    rem = s - k * r0
    lo1, hi1 = (max(0, rem - (P - 1)), min(P - 1, rem)) if t_free else (rem, rem)
    r1 = rng.randrange(lo1, hi1 + 1)
    r2 = rem - r1
    assert 0 <= r0 < P and 0 <= r1 < P and 0 <= r2 < P and k * r0 + r1 + r2 == s
    assert classify(i, r0, r1, r2) == case, (i, case, classify(i, r0, r1, r2))
    return r0, r1, r2


def directed_linear():
    """[(i, case, (r0, r1, r2))] for every i = 2..7 and every case of the function alone."""
    return [(i, c, operands(i, c)) for i in range(2, 8) for c in cases(i)]


def reachable(entry):
    """[(i, case)] that the first non-linear layer of a state from `entry` can meet."""
    free = ENTRIES[entry]
    out = []
    for i in range(2, 8):
        # l_i reads the new s0, s1 (places 0, 1) and, from i = 3 on, the new s_{i-1}, which is free iff place i - 1 is
        if i > 2 and (i - 1) not in free:
            continue
        out += [(i, c) for c in cases(i, t_free=i > 2)]
    return out


def state(i, case, entry, draw=0):
    """The canonical state in front of a non-linear layer that meets (i, case): places outside ENTRIES[entry] are left to the
    caller (returned as None); the free places hold canonical integers below p."""
    free = ENTRIES[entry]
    assert (i, case) in reachable(entry)
    for attempt in range(16):
        rng = random.Random("state %d %d %d %s %s" % (i, draw, attempt, case, entry))
        r0, r1, r2 = operands(i, case, draw + 97 * attempt, t_free=i > 2)
        new = [r * R_INV % P for r in (r0, r1)]                      # the new s0, s1 as field values
        old = [pow(new[0], 7, P), pow(new[1], INV7, P)] + [None] * 6
        ok, prev = True, 0
        for j in range(2, i):                                         # the places in front of i - 1 .. i: any value; track new s_j
            want = r2 * R_INV % P if j == i - 1 else rng.randrange(0, P)
            q = G.quad(j, G.linear(j, new[0], new[1], prev))
            if q == 0:
                ok = False
                break
            old[j] = want * pow(q, P - 2, P) % P
            prev = want
        if not ok:
            continue
        for j in range(i, 8):
            if j in free:
                old[j] = rng.randrange(0, P)
        assert all(old[j] is not None for j in free) and all(old[j] is None for j in range(8) if j not in free)
        return old
    raise AssertionError("no state found")


def first_layer_operands(s, i):
    """The residues linear() sees for state element i in the first non-linear layer of canonical state s."""
    n = G.nonlinear(s)
    return n[0] * R % P, n[1] * R % P, (n[i - 1] * R % P if i > 2 else 0)


def merge_states(draw=0):
    """{(i, case): 8 canonical words} for merge: the whole state is the caller's."""
    out = {}
    for rc in reachable("merge"):
        s = state(rc[0], rc[1], "merge", draw)
        assert classify(rc[0], *first_layer_operands(s, rc[0])) == rc[1]
        out[rc] = s
    return out


def row_states(draw=0):
    """{(i, case): 4 canonical elements}: a row of exactly one rate block (state[4..8] = 0)."""
    out = {}
    for rc in reachable("row"):
        s = state(rc[0], rc[1], "row", draw)
        full = s[:4] + [0, 0, 0, 0]
        assert classify(rc[0], *first_layer_operands(full, rc[0])) == rc[1]
        out[rc] = s[:4]
    return out


def seed_states(draw=0):
    """{(i, case): 4 seed words + the nonce (below p)} for merge_with_int: state = seed || nonce, 0, 0, 5."""
    out = {}
    for rc in reachable("merge_with_int"):
        s = state(rc[0], rc[1], "merge_with_int", draw)
        full = s[:5] + [0, 0, 5]
        assert classify(rc[0], *first_layer_operands(full, rc[0])) == rc[1]
        out[rc] = s[:5]
    return out


def stored(words):
    """Canonical integers -> the stored (Montgomery) form the library's rows hold."""
    return [int(w) * R % P for w in words]


LIMB_ALPHABET = [0, 1, 2**32 - 1, 2**32, 2**32 + 1, P - 1, P - 2, P - 2**32, 2**63, 0xFFFFFFFE00000001, 0xFFFFFFFF]
