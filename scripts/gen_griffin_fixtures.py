"""Writes tests/golden/griffinjive64_256_params.json and tests/golden/griffinjive64_256_kat.json: the published parameters of
GriffinJive64_256 (Griffin of state width 8 over p = 2^64 - 2^32 + 1 with the Jive compression mode: alpha, its inverse, the
first row of the circulant MDS matrix, the 6 x 8 round constants, the alpha_i / beta_i of the quadratic steps) and the two
literal known answers the reference's tests hold for it (the permutation of 0..7 and hash_elements of 0..7), parsed as
numbers out of a checkout of the reference:

    python scripts/gen_griffin_fixtures.py <reference checkout> [--header]

  crypto/src/hash/griffin/griffin64_256_jive/mod.rs    MDS, ARK, ALPHA, BETA
  crypto/src/hash/griffin/griffin64_256_jive/tests.rs  fn apply_permutation, fn hash: input and expected values

Only numbers leave the reference.  The S-box exponents are not literals there (exp7, and an addition chain whose comment
names 10540996611094048183): they are stated here and checked, 7 * inv_alpha = 1 mod (p - 1).  Every number is checked
before it is written: the matrix is circulant (row i = row 0 rotated right by i), every constant is below p, and the
function restated on Python integers (tests/griffin_util.py holds the same restatement) reproduces both known answers.

--header prints the tables of csrc/griffin_dev.hpp (the same numbers in the library's Montgomery form, x * 2^64 mod p)
instead of writing the fixtures; tests/test_griffin_host.py pins that header to the fixture."""
import json
import os
import re
import sys

P = 2**64 - 2**32 + 1
W, ROUNDS = 8, 7
ALPHA, INV_ALPHA = 7, 10540996611094048183
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = re.compile(r"BaseElement::new\(\s*(\d+)\s*\)")


def _section(text, start, end=None):
    a = text.index(start)
    b = text.index(end, a + len(start)) if end else len(text)
    return [int(x) for x in NEW.findall(text[a:b])]


def permute(state, prm):
    row, al, be = prm["mds_row"], prm["alpha_i"], prm["beta_i"]
    s = [x % P for x in state]
    for r in range(ROUNDS):
        s[0] = pow(s[0], prm["inv_alpha"], P)
        s[1] = pow(s[1], prm["alpha"], P)
        for i in range(2, W):
            l = ((i - 1) * s[0] + s[1] + (s[i - 1] if i > 2 else 0)) % P
            s[i] = s[i] * (l * l + al[i - 2] * l + be[i - 2]) % P
        s = [sum(row[(j - i) % W] * s[j] for j in range(W)) % P for i in range(W)]
        if r < ROUNDS - 1:
            s = [(x + k) % P for x, k in zip(s, prm["ark"][r])]
    return s


def hash_elements(elems, prm):
    s = [0] * W
    s[4] = int(len(elems) % 4 != 0)
    i = 0
    for e in elems:
        s[i] = (s[i] + e) % P
        i += 1
        if i == 4:
            s, i = permute(s, prm), 0
    if i:
        s[i:4] = [1] + [0] * (3 - i)
        s = permute(s, prm)
    return s[:4]


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if len(args) != 1:
        sys.exit(__doc__)
    base = os.path.join(args[0], "crypto", "src", "hash", "griffin", "griffin64_256_jive")
    mod = open(os.path.join(base, "mod.rs")).read()
    tests = open(os.path.join(base, "tests.rs")).read()

    mds = _section(mod, "\nconst MDS:", "const INV_MDS:")
    ark = _section(mod, "\nconst ARK:")
    alpha_i = _section(mod, "const ALPHA:", "const BETA:")
    beta_i = _section(mod, "const BETA:", "// GRIFFIN PERMUTATION")
    assert len(mds) == W * W and len(ark) == (ROUNDS - 1) * W and len(alpha_i) == W - 2 and len(beta_i) == W - 2
    prm = {
        "modulus": P, "state_width": W, "rate_range": [0, 4], "capacity_range": [4, 8], "digest_range": [0, 4],
        "num_rounds": ROUNDS, "alpha": ALPHA, "inv_alpha": INV_ALPHA, "mds_row": mds[:W],
        "ark": [ark[W * r:W * r + W] for r in range(ROUNDS - 1)], "alpha_i": alpha_i, "beta_i": beta_i,
    }
    assert prm["alpha"] * prm["inv_alpha"] % (P - 1) == 1
    assert str(INV_ALPHA) in mod, "the reference's addition chain names another exponent"
    for i in range(W):
        assert mds[W * i:W * i + W] == [mds[(j - i) % W] for j in range(W)], "the matrix is not circulant"
    assert all(0 <= x < P for x in ark + alpha_i + beta_i)

    perm = _section(tests, "fn apply_permutation()", "assert_eq!(expected, state)")
    hsh = _section(tests, "fn hash()", "assert_eq!(expected, result.as_elements())")
    assert len(perm) == 2 * W and len(hsh) == W + 4
    where = "crypto/src/hash/griffin/griffin64_256_jive/tests.rs, "
    kat = {"permutation": {"where": where + "fn apply_permutation", "input": perm[:W], "expected": perm[W:]},
           "hash_elements": {"where": where + "fn hash", "input": hsh[:W], "expected": hsh[W:]}}
    assert permute(kat["permutation"]["input"], prm) == kat["permutation"]["expected"], "the restated permutation misses the known answer"
    assert hash_elements(kat["hash_elements"]["input"], prm) == kat["hash_elements"]["expected"], "the restated sponge misses the known answer"

    if "--header" in sys.argv:
        def words(r):
            return ["0x%016xull" % (x * 2**64 % P) for x in r]
        print("    // ARK")
        for r in prm["ark"]:
            w = words(r)
            print("        {%s," % ", ".join(w[:4]))
            print("         %s}," % ", ".join(w[4:]))
        for name in ("alpha_i", "beta_i"):
            w = words(prm[name])
            print("    // %s" % name)
            print("        %s," % ", ".join(w[:3]))
            print("        %s," % ", ".join(w[3:]))
        print("    MDS_ROW = {%s}" % ", ".join(str(x) for x in prm["mds_row"]))
        return
    out = os.path.join(ROOT, "tests", "golden")
    for name, obj in (("griffinjive64_256_params.json", prm), ("griffinjive64_256_kat.json", kat)):
        with open(os.path.join(out, name), "w") as f:
            json.dump(obj, f, indent=1)
            f.write("\n")
        print("wrote", os.path.join(out, name))


if __name__ == "__main__":
    main()
