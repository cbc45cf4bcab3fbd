"""Test helper: directed operands for the linear layer of the two Rescue hashers, on Python integers only.

rp::mds_row / rpj::mds_row (csrc/rescue_dev.hpp, csrc/rescue_jive_dev.hpp) sum a row of the MDS product in two 64-bit
accumulators and end with ONE canonical addition.  With y the state behind the first S-box (raw Montgomery residues, each
below p), h_j / l_j the high / low 32-bit words of y[j], and for output row i

    hi  = sum_k row[k] * h[(i + k) mod w]        lo = sum_k row[k] * l[(i + k) mod w]
    top = hi >> 32        b = (hi mod 2^32) << 32        a = lo + top * (2^32 - 1)

the result is b + a reduced once.  The cases a state can be asked to meet in row i:

    1  "wrap"     b + a >= 2^64          the 64-bit sum wraps: a function ending in a plain + is wrong here
    2  "wrap0"    b + a == 2^64          wraps to exactly zero
    3  "p"        b + a == p             the smallest sum that needs the subtraction
    4  "p-1"      b + a == p - 1         the largest sum that needs nothing
    5  "above_p"  p < b + a < 2^64       subtraction without a wrap

A state is built by drawing every caller-controlled word at random and solving two of them -- one high word and one low
word whose coefficients in row i are odd -- through the inverse mod 2^32; the case is asserted on Python integers for every
state handed out.  An entry point controls only some places of the state (`ENTRY`); the others hold the values the sponge
puts there.  `preimage` turns the state behind the S-box into the state in front of it (the S-box is a bijection), as
canonical integers; `stored` gives the Montgomery residues a row holds."""
import json
import os

import numpy as np

P = 2**64 - 2**32 + 1
M32 = 2**32
R = 2**64 % P
R_INV = pow(2**64, -1, P)
CASES = ("wrap", "wrap0", "p", "p-1", "above_p")

_G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PARAMS = {"rp64_256": json.load(open(os.path.join(_G, "rp64_256_params.json"))),
          "rpjive64_256": json.load(open(os.path.join(_G, "rpjive64_256_params.json")))}

# entry point -> (hasher, {place: canonical value the sponge puts there}, the places the caller controls)
ENTRY = {
    "rp_state": ("rp64_256", {}, list(range(12))),                         # the probe and the host program: every place
    "rp_rows": ("rp64_256", {0: 8, 1: 0, 2: 0, 3: 0}, list(range(4, 12))),  # hash_elements of 8 elements, and merge
    "rp_seed": ("rp64_256", {0: 5, 1: 0, 2: 0, 3: 0, 9: 0, 10: 0, 11: 0}, list(range(4, 9))),  # merge_with_int, nonce < p
    "rpj_state": ("rpjive64_256", {}, list(range(8))),
    "rpj_rows": ("rpjive64_256", {0: 0, 1: 0, 2: 0, 3: 0}, list(range(4, 8))),  # hash_elements of 4 elements
    "rpj_merge": ("rpjive64_256", {}, list(range(8))),
    "rpj_seed": ("rpjive64_256", {5: 0, 6: 0, 7: 5}, list(range(0, 5))),    # merge_with_int, nonce < p
}


def sbox(c: int) -> int:
    """canonical c in front of the first S-box -> the raw Montgomery residue behind it."""
    return pow(c, 7, P) * R % P


def preimage(hasher: str, y) -> list:
    """The state behind the first S-box (raw residues) -> the canonical integers in front of it."""
    inv_alpha = PARAMS[hasher]["inv_alpha"]
    out = [pow(v * R_INV % P, inv_alpha, P) for v in y]
    assert [sbox(c) for c in out] == list(y)
    return out


def stored(canon) -> list:
    """canonical integers -> the residues a row stores."""
    return [c * R % P for c in canon]


def sums(row, y, i):
    """(hi, lo, top, b, a) of output row i, as the comments of mds_row name them."""
    w = len(row)
    hi = sum(row[k] * (y[(i + k) % w] >> 32) for k in range(w))
    lo = sum(row[k] * (y[(i + k) % w] & (M32 - 1)) for k in range(w))
    top = hi >> 32
    return hi, lo, top, (hi % M32) << 32, lo + top * (M32 - 1)


def case_of(row, y, i):
    """The case row i of state y meets, or None."""
    _, _, _, b, a = sums(row, y, i)
    s = b + a
    if s == 2**64:
        return "wrap0"
    if s > 2**64:
        return "wrap"
    if s == P:
        return "p"
    if s == P - 1:
        return "p-1"
    if s > P:
        return "above_p"
    return None


def meets(row, y, i, case) -> bool:
    got = case_of(row, y, i)
    return got == case or (case == "wrap" and got == "wrap0")


def mds_row_value(row, y, i) -> int:
    """What mds_row must return: the row product of the residues, canonical residue of the sum."""
    w = len(row)
    return sum(row[k] * y[(i + k) % w] for k in range(w)) % P


def mds_row_plain_plus(row, y, i) -> int:
    """The mutant: the two accumulators joined by a 64-bit + without the canonical addition's corrections."""
    _, _, _, b, a = sums(row, y, i)
    return (b + a) % 2**64


def directed_state(entry: str, i: int, case: str, rng, tries: int = 400):
    """A state y (raw residues behind the first S-box) whose row i meets `case` at entry point `entry`, or None when the
    entry point cannot reach it (no controlled place with an odd coefficient, or no draw met the case)."""
    hasher, fixed, ctl = ENTRY[entry]
    row = PARAMS[hasher]["mds_row"]
    w = len(row)
    assert case in CASES and 0 <= i < w
    coef = {j: row[(j - i) % w] for j in range(w)}
    odd = [j for j in ctl if coef[j] % 2 == 1]
    if not odd:
        return None
    base = [0] * w
    for j, c in fixed.items():
        base[j] = sbox(c)
    total = sum(row)
    for _ in range(tries):
        f_hi, f_lo = (odd[int(rng.integers(0, len(odd)))] for _ in range(2))
        h = {j: base[j] >> 32 for j in range(w)}
        lw = {j: base[j] & (M32 - 1) for j in range(w)}
        for j in ctl:
            h[j] = int(rng.integers(0, M32 - 1))      # < 2^32 - 1: the residue is below p whatever its low word
            lw[j] = int(rng.integers(0, M32))
        rest_hi = sum(coef[j] * h[j] for j in range(w) if j != f_hi)
        rest_lo = sum(coef[j] * lw[j] for j in range(w) if j != f_lo)
        for delta in rng.permutation(2 * total):
            delta = int(delta)
            # hi mod 2^32 = 2^32 - 1 - delta, so b = 2^64 - (delta + 1) 2^32
            h_f = (M32 - 1 - delta - rest_hi) * pow(coef[f_hi], -1, M32) % M32
            if h_f == M32 - 1:
                continue
            top = (rest_hi + coef[f_hi] * h_f) >> 32
            # a = lo + top 2^32 - top: its low word is (lo - top) mod 2^32; the high word comes out as the draw has it
            want_low = {"wrap": int(rng.integers(0, M32)), "wrap0": 0, "p": 1, "p-1": 0,
                        "above_p": int(rng.integers(2, M32))}[case]
            l_f = (want_low + top - rest_lo) * pow(coef[f_lo], -1, M32) % M32
            y = [(h[j] << 32) | lw[j] for j in range(w)]
            y[f_hi] = (h_f << 32) | (y[f_hi] & (M32 - 1))
            y[f_lo] = (y[f_lo] & ~(M32 - 1)) | l_f
            if meets(row, y, i, case) and (case != "wrap" or case_of(row, y, i) == "wrap"):
                assert all(0 <= v < P for v in y) and all(y[j] == base[j] for j in fixed)
                assert mds_row_value(row, y, i) == (sums(row, y, i)[3] + sums(row, y, i)[4]) % P
                if case in ("wrap", "wrap0"):
                    assert mds_row_plain_plus(row, y, i) != mds_row_value(row, y, i)
                return y
    return None


def extra_states(w: int):
    """Every element p - 1 (the largest hi) and every element 0xFFFFFFFEFFFFFFFF (the largest lo): the bounds in the comments
    of mds_row."""
    return [[P - 1] * w, [0xFFFFFFFEFFFFFFFF] * w]


_CACHE = {}


def directed_set(entry: str, seed: int = 0):
    """{(row, case): state} for every pair the entry point reaches (fixed for a seed; kept, so that tests share one set)."""
    key = (entry, seed)
    if key not in _CACHE:
        rng = np.random.default_rng([seed, sorted(ENTRY).index(entry)])
        w = PARAMS[ENTRY[entry][0]]["state_width"]
        out = {}
        for i in range(w):
            for case in CASES:
                y = directed_state(entry, i, case, rng)
                if y is not None:
                    out[(i, case)] = y
        _CACHE[key] = out
    return _CACHE[key]


def reachable(entry: str, seed: int = 0):
    return sorted(directed_set(entry, seed), key=lambda rc: (rc[0], CASES.index(rc[1])))


def all_pairs(entry: str):
    w = PARAMS[ENTRY[entry][0]]["state_width"]
    return [(i, case) for i in range(w) for case in CASES]


def inputs(entry: str, seed: int = 0):
    """The directed set as what the entry point's caller hands in: per (row, case) the canonical integers of the controlled
    places, in place order."""
    hasher, _, ctl = ENTRY[entry]
    out = {}
    for rc, y in directed_set(entry, seed).items():
        c = preimage(hasher, y)
        out[rc] = [c[j] for j in ctl]
    return out
