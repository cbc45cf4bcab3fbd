"""Writes tests/golden/rpjive64_256_params.json and tests/golden/rpjive64_256_kat.json: the published parameters of
RpJive64_256 (Rescue Prime of state width 8 over p = 2^64 - 2^32 + 1 with the Jive compression mode: alpha, its inverse, the
first row of the circulant MDS matrix, the 2 x 7 x 8 round constants) and the one literal known answer the reference's
tests hold for it (the permutation of 0..7), parsed as numbers out of a checkout of the reference:

    python scripts/gen_rpjive_fixtures.py <reference checkout> [--header]

  crypto/src/hash/rescue/rp64_256_jive/mod.rs    ALPHA, INV_ALPHA, MDS, ARK1, ARK2
  crypto/src/hash/rescue/rp64_256_jive/tests.rs  fn apply_permutation: input state and expected state

Only numbers leave the reference.  Every number is checked before it is written: alpha * inv_alpha = 1 mod (p - 1), the
matrix is circulant (row i = row 0 rotated right by i), and the permutation restated on Python integers
(tests/rpjive_util.py holds the same restatement) turns the known answer's input into its expected state.

--header prints the tables of csrc/rescue_jive_dev.hpp (the same numbers in the library's Montgomery form, x * 2^64 mod p)
instead of writing the fixtures; tests/test_rpjive_host.py pins that header to the fixture."""
import json
import os
import re
import sys

P = 2**64 - 2**32 + 1
W, ROUNDS = 8, 7
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = re.compile(r"BaseElement::new\(\s*(\d+)\s*\)")


def _section(text, start, end=None):
    a = text.index(start)
    b = text.index(end, a + len(start)) if end else len(text)
    return [int(x) for x in NEW.findall(text[a:b])]


def _const(text, name):
    return int(re.search(r"const\s+%s\s*:\s*u64\s*=\s*(\d+)\s*;" % name, text).group(1))


def permute(state, prm):
    row = prm["mds_row"]

    def mds(s):
        return [sum(row[(j - i) % W] * s[j] for j in range(W)) % P for i in range(W)]

    s = [x % P for x in state]
    for r in range(ROUNDS):
        s = [pow(x, prm["alpha"], P) for x in s]
        s = [(x + k) % P for x, k in zip(mds(s), prm["ark1"][r])]
        s = [pow(x, prm["inv_alpha"], P) for x in s]
        s = [(x + k) % P for x, k in zip(mds(s), prm["ark2"][r])]
    return s


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if len(args) != 1:
        sys.exit(__doc__)
    base = os.path.join(args[0], "crypto", "src", "hash", "rescue", "rp64_256_jive")
    mod = open(os.path.join(base, "mod.rs")).read()
    tests = open(os.path.join(base, "tests.rs")).read()

    mds = _section(mod, "\nconst MDS:", "\nconst INV_MDS:")
    ark1 = _section(mod, "\nconst ARK1:", "\nconst ARK2:")
    ark2 = _section(mod, "\nconst ARK2:")
    assert len(mds) == W * W and len(ark1) == ROUNDS * W and len(ark2) == ROUNDS * W
    prm = {
        "modulus": P, "state_width": W, "rate_range": [4, 8], "capacity_range": [0, 4], "digest_range": [4, 8],
        "num_rounds": ROUNDS, "alpha": _const(mod, "ALPHA"), "inv_alpha": _const(mod, "INV_ALPHA"), "mds_row": mds[:W],
        "ark1": [ark1[W * r:W * r + W] for r in range(ROUNDS)], "ark2": [ark2[W * r:W * r + W] for r in range(ROUNDS)],
    }
    assert prm["alpha"] * prm["inv_alpha"] % (P - 1) == 1
    for i in range(W):
        assert mds[W * i:W * i + W] == [mds[(j - i) % W] for j in range(W)], "the matrix is not circulant"
    assert all(0 <= x < P for x in ark1 + ark2)

    kat = _section(tests, "fn apply_permutation()", "assert_eq!(expected, state)")
    assert len(kat) == 2 * W
    kat = {"where": "crypto/src/hash/rescue/rp64_256_jive/tests.rs, fn apply_permutation", "input": kat[:W], "expected": kat[W:]}
    assert permute(kat["input"], prm) == kat["expected"], "the restated permutation misses the known answer"

    if "--header" in sys.argv:
        def table(name, rows):
            print("            {   // %s" % name)
            for r in rows:
                words = ["0x%016xull" % (x * 2**64 % P) for x in r]
                print("                {%s," % ", ".join(words[:4]))
                print("                 %s}," % ", ".join(words[4:]))
            print("            },")
        table("ARK1", prm["ark1"])
        table("ARK2", prm["ark2"])
        print("    MDS_ROW = {%s}" % ", ".join(str(x) for x in prm["mds_row"]))
        return
    out = os.path.join(ROOT, "tests", "golden")
    for name, obj in (("rpjive64_256_params.json", prm), ("rpjive64_256_kat.json", kat)):
        with open(os.path.join(out, name), "w") as f:
            json.dump(obj, f, indent=1)
            f.write("\n")
        print("wrote", os.path.join(out, name))


if __name__ == "__main__":
    main()
